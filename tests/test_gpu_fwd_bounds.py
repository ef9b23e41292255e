"""The forward's per-tile bounds table (csrc/jet_common.hpp act_bounds) and the saved-stream reverse
sweep that reads it (policy 5: csrc/jet_fb.hpp with SAVED = true).

A forward that saves the streams of a jet that sweep serves (W = 128: the 2-d Laplacian jet, the 2-d
gradient jet) leaves, per tile and layer j = 0 .. L - 1, two floats at the start of layer 0's stream-1
slot of that tile (layer 0 saves its value stream only):
the tile's maximum of w |t| over the tangent streams of z_j and (Laplacian jets) of w |q| + w^2 sum t^2.
The sweep forms the fp16 scales of its h planes from them instead of bounding the saved streams itself.

(a) the table against the saved streams themselves, recomputed in torch fp32 (layer 0 from W_0), within
    4 x 2^-23 relative (two fp32 roundings plus one fma-versus-mul-add difference), for the f16x3, the
    bf16x6 and the exact-fp32 forward; layer 0's value-stream region is the forward's z_0;
(b) parameter gradients of the sweep against the CPU oracle, normwise max|hip - ref| <= 1e-5 max|ref|:
    default weights; first-layer weights x 4000 at points / 4000 (a hidden layer's tangent bound past
    2^15: the forward's rare branch; the sine arguments stay where the oracle's fp32 is a reference);
    a batch whose tiles' bounds differ by more than 2^4 (a per-block value in place of a per-tile one
    overflows the other tiles' planes);
(c) a mixed launch of an act-saving Laplacian job beside a gradient job without act.

Shapes: 2 -> 1, 4 x 128 Laplacian jets at 16 points (one tile), 17 (one ragged point), 81 (5 tiles + 1);
2 -> 2, 5 x 128 gradient jets at 33 points (tiles in pairs per forward block).
"""
import ctypes
import math

import pytest
import torch

from oracle import siren_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5
RTOL_TABLE = 4 * 2.0 ** -23
V, G, LAP = 0, 1, 2
W, NT = 128, 8
LAP_NET, GRAD_NET = (2, 1, 4), (2, 2, 5)  # (d_in, d_out, hidden layers)


@pytest.fixture(scope="module")
def B():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import base
    base._native.load()
    with base._native.knobs(policy=5):
        yield base


def nerr(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def points(n, seed):
    return torch.rand(n, 2, generator=torch.Generator().manual_seed(seed)) * 2 - 1


# ---------------------------------------------------------------------------------------------------
# (a) the table
# ---------------------------------------------------------------------------------------------------
def forward_act(B, net, x, mode, prec_bits=0, fill=-3.0):
    """One insr_siren_jet_fwd with saved streams: (act as [layer][tile][S * NT * 256], outputs)."""
    nat = B._native
    lib = nat.lib()
    din, dout, L = net.in_features, net.out_features, net.num_hidden_layers
    n = x.shape[0]
    net.refresh_wsplit()
    flat = net.flat_params()
    cm = mode | nat.MODE_WSPLIT | nat.jet_policy(5) | prec_bits
    assert lib.insr_jet_bwd_path(n, din, dout, L, W, cm) == 2 and lib.insr_jet_bwd_kernel(n, din, dout, L, W, cm) == 1
    S = {G: 1 + din, LAP: 2 + din}[mode]
    nbytes = lib.insr_jet_act_bytes(n, din, L, W, cm)
    ntiles = (n + 63) // 64 * 4
    assert nbytes == (L + 1) * ntiles * S * NT * 256 * 4
    act = torch.full((nbytes // 4,), fill, device="cuda")
    y = torch.empty(n, dout, device="cuda")
    dy = torch.empty(n, dout, din, device="cuda")
    lp = torch.empty(n, dout, device="cuda") if mode == LAP else None
    nat.check(lib.insr_siren_jet_fwd(nat.ptr(x), n, din, dout, L, W, cm, nat.ptr(flat), nat.ptr(y), nat.ptr(dy),
                                     nat.ptr(lp), nat.ptr(act), nat.stream_of(x.device)), "fwd")
    torch.cuda.synchronize()
    return act.view(L + 1, ntiles, S * NT * 256).cpu(), S, (y, dy, lp)


def streams(act, S, layer, tile):
    """z-streams of (layer, tile) as [S][16 points][128 neurons] ([s][row tile][g][c][r] in act)."""
    z = act[layer, tile].view(S, NT, 4, 16, 4)
    return z.permute(0, 3, 1, 2, 4).reshape(S, 16, W)


def expected_pair(z, lap):
    """fp32, from the z-streams [S][16][128] of one tile and layer."""
    ntan = z.shape[0] - (2 if lap else 1)
    t = z[1:1 + ntan]
    bt = 30.0 * t.abs().max()
    bl = (30.0 * z[-1].abs() + 900.0 * (t * t).sum(0)).max() if lap else torch.zeros(())
    return float(bt), float(bl)


def check_table(B, shape, mode, n, prec_bits, tag):
    din, dout, L = shape
    torch.manual_seed(91)
    net = B.MLP(din, dout, L, W, nonlinearity="sine").cuda()
    x = points(n, n).cuda()
    act, S, _ = forward_act(B, net, x, mode, prec_bits)
    w0 = net.net[0].weight.detach().float().cpu()
    b0 = net.net[0].bias.detach().float().cpu()
    tiles = (n + 15) // 16
    worst = 0.0
    for tile in range(tiles):
        table = act[0, tile, NT * 256:NT * 256 + 2 * L].view(L, 2)
        for j in range(L):
            if j == 0:  # tangents: the W_0 columns, Laplacian stream 0
                z = torch.zeros(S, 16, W)
                for k in range(din):
                    z[1 + k] = w0[:, k]
            else:
                z = streams(act, S, j, tile)
            for cl, want in enumerate(expected_pair(z, mode == LAP)):
                got = float(table[j, cl])
                if want == 0.0:
                    assert got == 0.0, (tag, tile, j, cl, got)
                    continue
                e = abs(got - want) / want
                worst = max(worst, e)
                assert e <= RTOL_TABLE, (tag, tile, j, cl, got, want, e)
        # layer 0: the value stream is the forward's z_0 (points past the batch: x = 0), the rest of the
        # stream-1 slot and the other streams' slots stay untouched
        xt = torch.zeros(16, din)
        m = min(16, n - 16 * tile)
        xt[:m] = x[16 * tile:16 * tile + m].cpu()
        z0 = (xt.double() @ w0.double().t() + b0.double())
        got0 = streams(act, S, 0, tile)[0].double()
        assert float((got0 - z0).abs().max()) <= RTOL_TABLE * float(z0.abs().max()), (tag, tile)
        assert bool((act[0, tile, NT * 256 + 2 * L:] == -3.0).all()), (tag, tile)
    print(tag, f"table worst rel {worst:.3e}")


PRECS = {"f16x3": None, "bf16x6": 1, "fp32": 0}  # forward precision (INSR_PREC_*); the backward stays bf16x6


def prec_bits(B, name):
    nat = B._native
    return 0 if PRECS[name] is None else (nat.jet_prec(PRECS[name]) | nat.jet_bprec(nat.PREC_BF16X6))


@pytest.mark.parametrize("n", [16, 17, 81])
def test_table_laplace_jet(B, n):
    check_table(B, LAP_NET, LAP, n, 0, ("lap", n))


def test_table_gradient_jet(B):
    check_table(B, GRAD_NET, G, 33, 0, ("grad5", 33))


@pytest.mark.parametrize("prec", ["bf16x6", "fp32"])
def test_table_other_forwards(B, prec):
    """The split-bf16 and the exact-fp32 forwards leave the same table (their sweep is the same one)."""
    check_table(B, LAP_NET, LAP, 17, prec_bits(B, prec), ("lap", prec))
    check_table(B, GRAD_NET, G, 33, prec_bits(B, prec), ("grad5", prec))


# ---------------------------------------------------------------------------------------------------
# (b) the sweep on the table, against the oracle
# ---------------------------------------------------------------------------------------------------
def pair(B, shape, seed, edit=None):
    din, dout, L = shape
    torch.manual_seed(seed)
    ref = O.OracleSiren(din, dout, L, W)
    torch.manual_seed(seed)
    net = B.MLP(din, dout, L, W, nonlinearity="sine")
    if edit is not None:
        with torch.no_grad():
            edit(next(iter(ref.parameters())), list(ref.parameters())[1])
            edit(net.net[0].weight, net.net[0].bias)
    for a, b in zip(ref.parameters(), net.parameters()):
        assert torch.equal(a.detach(), b.detach())
    return ref, net.cuda()


def grads_of(params):
    return [(p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone() for p in params]


def check_grads(ref, net, tag):
    for (k, _), a, b in zip(ref.named_parameters(), grads_of(ref.parameters()), grads_of(net.parameters())):
        assert torch.isfinite(b).all(), (tag, k)
        e = nerr(b, a)
        print(tag, k, f"{e:.3e}")
        assert e < TOL, (tag, k, e)


def hidden_tangent_bounds(ref, x):
    """w max|t_1| per 16-point tile: the tangent streams of the first hidden layer's z (fp64)."""
    ps = [p.detach().double() for p in ref.parameters()]
    w0, b0, w1 = ps[0], ps[1], ps[2]
    z0 = x.double() @ w0.t() + b0
    out = []
    for k in range(x.shape[1]):
        t1 = (30.0 * torch.cos(30.0 * z0) * w0[:, k]) @ w1.t()
        out.append(30.0 * t1.abs())
    b = torch.stack(out).amax(0).amax(1)
    pad = (-len(b)) % 16
    return torch.cat([b, b.new_zeros(pad)]).view(-1, 16).amax(1)


def laplace_case(B, x, tag, edit=None, seed=92):
    n = x.shape[0]
    assert B._native.lib().insr_jet_bwd_path(n, 2, 1, 4, W, LAP | B._native.scope_bits()) == 2
    ref, net = pair(B, LAP_NET, seed, edit)
    xr = x.clone().requires_grad_(True)
    yr = ref(xr)
    gr, lr_ = O.op_gradient(yr, xr), O.op_laplace(yr, xr)
    g = torch.Generator().manual_seed(n + 1)
    Ry, Rg, Rl = torch.randn(yr.shape, generator=g), torch.randn(gr.shape, generator=g), torch.randn(lr_.shape, generator=g)
    # the output bias's gradient is the plain sum of the value adjoints, one number: adjoints of mean 1 keep it
    # from cancelling (zero-mean ones can leave a sum that either side's fp32 additions resolve to 1e-4 only)
    Ry = 1.0 + 0.5 * Ry
    # adjoints of comparable weight on the three outputs whatever the scale of the first layer
    sy, sg, sl = (1.0 / float(v.detach().abs().max().clamp_min(1e-30)) for v in (yr, gr, lr_))
    ((yr * Ry).sum() * sy + (gr * Rg).sum() * sg + (lr_ * Rl).sum() * sl).backward()
    xg = x.cuda().requires_grad_(True)
    y = net(xg)
    lp, gp = B.laplace(y, xg, return_grad=True)
    ((y * Ry.cuda()).sum() * sy + (gp * Rg.cuda()).sum() * sg + (lp * Rl.cuda()).sum() * sl).backward()
    torch.cuda.synchronize()
    check_grads(ref, net, tag)
    return ref


def gradient_case(B, x, tag, edit=None, seed=93):
    n = x.shape[0]
    assert B._native.lib().insr_jet_bwd_path(n, 2, 2, 5, W, G | B._native.scope_bits()) == 2
    ref, net = pair(B, GRAD_NET, seed, edit)
    xr = x.clone().requires_grad_(True)
    Jr = O.op_jacobian(ref(xr) + xr, xr)[0]
    R = torch.randn(Jr.shape, generator=torch.Generator().manual_seed(n + 3))
    s = 1.0 / float(Jr.detach().abs().max())
    ((Jr * R).sum() * s).backward()
    xg = x.cuda().requires_grad_(True)
    ((B.jacobian(net(xg) + xg, xg)[0] * R.cuda()).sum() * s).backward()
    torch.cuda.synchronize()
    check_grads(ref, net, tag)
    return ref


@pytest.mark.parametrize("n", [16, 17, 81])
def test_sweep_laplace_jet_default_weights(B, n):
    laplace_case(B, points(n, n), ("lap", n))


def test_sweep_gradient_jet_default_weights(B):
    gradient_case(B, points(33, 33), ("grad5", 33))


def scale_first_layer(w, b):
    w.mul_(4000.0)


@pytest.mark.parametrize("n", [17, 81])
def test_sweep_laplace_jet_tangents_past_the_window(B, n):
    """W_0 x 4000 at points / 4000: z_0 as with default weights, every tangent stream 4000 times larger --
    the first hidden layer's bound w |t| passes 2^15 (the forward scales its tangent planes too)."""
    x = points(n, n) / 4000.0
    ref = laplace_case(B, x, ("lap-big", n), edit=scale_first_layer)
    assert float(hidden_tangent_bounds(ref, x).max()) >= 32768.0


def test_sweep_gradient_jet_tangents_past_the_window(B):
    x = points(33, 33) / 4000.0
    ref = gradient_case(B, x, ("grad5-big", 33), edit=scale_first_layer)
    assert float(hidden_tangent_bounds(ref, x).max()) >= 32768.0


def quarter_period_bias(w, b):
    b.fill_(math.pi / 60.0)  # w z_0 = pi / 2 at x = 0: cos = 0, the tangents of h_0 vanish there


def uneven_points(n_tiles_live):
    """Tiles of points at the origin around tiles of random points, and one ragged point."""
    parts = [torch.zeros(16, 2)]
    for k in range(n_tiles_live):
        parts += [points(16, 40 + k), torch.zeros(16, 2)]
    parts.append(points(1, 7))
    return torch.cat(parts)


def test_sweep_laplace_jet_uneven_tiles(B):
    x = uneven_points(2)  # 81 points: tiles 0, 2, 4 at the origin
    ref = laplace_case(B, x, ("lap-uneven", x.shape[0]), edit=quarter_period_bias)
    b = hidden_tangent_bounds(ref, x)
    assert float(b[1] / b[0]) >= 16.0 and float(b[3] / b[2]) >= 16.0 and float(b[3] / b[4]) >= 16.0, b


def test_sweep_gradient_jet_uneven_tiles(B):
    x = uneven_points(1)  # 49 points: tiles 0 and 2 at the origin (tiles 0, 1 share a forward block)
    ref = gradient_case(B, x, ("grad5-uneven", x.shape[0]), edit=quarter_period_bias)
    b = hidden_tangent_bounds(ref, x)
    assert float(b[1] / b[0]) >= 16.0 and float(b[1] / b[2]) >= 16.0, b


# ---------------------------------------------------------------------------------------------------
# (c) mixed launch
# ---------------------------------------------------------------------------------------------------
def test_mixed_launch_table_only_where_act(B):
    """An act-saving Laplacian job beside a gradient job with act == NULL in one insr_siren_jet_fwd_mixed
    launch: the Laplacian job's act (streams and table) and both jobs' outputs equal their own launches'."""
    nat = B._native
    lib = nat.lib()
    n = 81
    torch.manual_seed(94)
    pres = B.MLP(2, 1, 4, W, nonlinearity="sine").cuda()
    vel = B.MLP(2, 2, 4, W, nonlinearity="sine").cuda()
    x = points(n, 5).cuda()
    act1, S, (y1, dy1, lp1) = forward_act(B, pres, x, LAP)
    vel.refresh_wsplit()
    vflat = vel.flat_params()
    pbits = nat.MODE_WSPLIT | nat.jet_policy(5)
    st = nat.stream_of(x.device)
    vy1, vdy1 = torch.empty(n, 2, device="cuda"), torch.empty(n, 2, 2, device="cuda")
    nat.check(lib.insr_siren_jet_fwd(nat.ptr(x), n, 2, 2, 4, W, G | pbits, nat.ptr(vflat), nat.ptr(vy1), nat.ptr(vdy1),
                                     None, None, st), "fwd")
    pflat = pres.flat_params()
    act = torch.full((act1.numel(),), -3.0, device="cuda")
    y, dy, lp = torch.empty_like(y1), torch.empty_like(dy1), torch.empty_like(lp1)
    vy, vdy = torch.empty_like(vy1), torch.empty_like(vdy1)
    jobs = (nat.JetJob * 2)(nat.JetJob(nat.ptr(x), nat.ptr(pflat), nat.ptr(y), nat.ptr(dy), nat.ptr(lp), nat.ptr(act), n, 1),
                            nat.JetJob(nat.ptr(x), nat.ptr(vflat), nat.ptr(vy), nat.ptr(vdy), None, None, n, 2))
    modes = (ctypes.c_int * 2)(LAP, G)
    sc = (ctypes.c_float * 6)()
    nat.check(lib.insr_siren_jet_fwd_mixed(jobs, modes, sc, 2, 2, 1, 4, W, pbits, st), "insr_siren_jet_fwd_mixed")
    torch.cuda.synchronize()
    assert torch.equal(act.cpu().view_as(act1), act1)
    for a, b in ((y, y1), (dy, dy1), (lp, lp1), (vy, vy1), (vdy, vdy1)):
        assert torch.equal(a, b)
    tiles = (n + 15) // 16
    assert bool((act1[0, :tiles, NT * 256:NT * 256 + 8] > 0).all())  # the table is there
