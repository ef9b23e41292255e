"""Coordinate gradients on the GPU (csrc/jet_xadj.hpp, base/_jet.py _x_adjoint): with MLP.coord_grad a
plain loss.backward() leaves the adjoint of the sample coordinates in x.grad and sends it on through x.

Judge: an fp64 deep copy of the oracle network (oracle/siren_oracle.py), differentiated with the
reference's own operators; bound max |hip - ref64| <= 1e-5 max |ref64| over the (n, d_in) tensor (the
project's contract) -- the fp32 oracle's own x-adjoint error against fp64 is 0.7e-6 .. 4.7e-6
on these shapes, so fp64 judges, not fp32.  Single points (n = 1, where "normwise" is pointwise) follow the
existing rule: within 3x the fp32 oracle's own error, or 1e-5.  The figures each case observed are printed
(lines starting with XGRAD-FIG; profiles/xgrad/gpu_tests_figures.txt keeps one run's)."""
import copy

import pytest
import torch

from oracle import siren_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5
ORDER = 2e-6  # the project's allowance for a different fp32 summation order
SHAPES = [(1, 1, 2, 32), (2, 1, 4, 128), (2, 2, 3, 64), (3, 3, 4, 128), (3, 3, 2, 256), (2, 2, 4, 128)]
MODES = {"value": 0, "grad": 1, "lap": 2}
SIZES = [1, 15, 17, 64, 65, 300, 1029]


@pytest.fixture(scope="module")
def B():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import base
    base._native.load()
    return base


def nerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def fig(*parts):
    print("XGRAD-FIG " + " ".join(str(p) for p in parts))


_NETS = {}


def nets(B, shape, seed=1, precision=None):
    """(fp32 oracle, its fp64 copy, the HIP net with the flag on, its flag-off twin) of one shape and seed,
    built once: the same init stream gives all of them the oracle's weights."""
    key = (shape, seed, precision)
    if key not in _NETS:
        din, dout, L, W = shape
        torch.manual_seed(seed)
        ref = O.OracleSiren(din, dout, L, W)
        made = []
        for flag in (True, False):
            torch.manual_seed(seed)
            made.append(B.MLP(din, dout, L, W, nonlinearity="sine", precision=precision, coord_grad=flag).cuda())
        _NETS[key] = (ref, copy.deepcopy(ref).double(), made[0], made[1])
    return _NETS[key]


def points(n, din, seed=3):
    return torch.rand(n, din, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def weights(n, din, dout, seed=5):
    """Adjoints of (y, J, lap): the value adjoint of one sign (uniform in [0.5, 1.5]), the others random
    (test_gpu_hess_jet.py weights)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, dout, generator=g) + 0.5, torch.randn(n, dout, din, generator=g),
            torch.randn(n, dout, generator=g))


def oracle_loss(ref, xr, adj, mode):
    """sum(Ry y + RJ J + RL lap) of an oracle network (in its dtype) with the reference's operators; lap
    per output channel."""
    Ry, RJ, RL = (a.to(xr.dtype) for a in adj)
    y = ref(xr)
    loss = (y * Ry).sum()
    if mode != "value":
        loss = loss + (O.op_jacobian(y, xr)[0] * RJ).sum()
    if mode == "lap":
        lap = torch.cat([O.op_laplace(y[:, o:o + 1], xr) for o in range(y.shape[1])], dim=-1)
        loss = loss + (lap * RL).sum()
    return loss


def oracle_xgrad(ref, x, adj, mode):
    """(x.grad, [parameter gradients]) of oracle_loss, in ref's dtype."""
    ref.zero_grad(set_to_none=True)
    xr = x.to(next(ref.parameters()).dtype).clone().requires_grad_(True)
    oracle_loss(ref, xr, adj, mode).backward()
    return xr.grad.detach(), [None if p.grad is None else p.grad.detach().clone() for p in ref.parameters()]


_JUDGE = {}


def judge(B, shape, mode, n):
    """The fp64 judge's x-adjoint of one parity case, computed once and shared (never modified)."""
    key = (shape, mode, n)
    if key not in _JUDGE:
        din, dout, _, _ = shape
        _JUDGE[key] = oracle_xgrad(nets(B, shape)[1], points(n, din, seed=n), weights(n, din, dout), mode)[0]
    return _JUDGE[key]


def hip_loss(B, net, xg, adj, mode):
    y, J, lap = B._jet.run_jet(net, xg, MODES[mode])
    Ry, RJ, RL = (a.cuda() for a in adj)
    loss = (y * Ry).sum()
    if mode != "value":
        loss = loss + (J * RJ).sum()
    if mode == "lap":
        loss = loss + (lap * RL).sum()
    return loss, (y, J, lap)


def hip_run(B, net, x, adj, mode):
    """One forward + backward: (x.grad or None, the flat parameter gradient, the outputs)."""
    net.zero_grad(set_to_none=True)
    xg = x.cuda().requires_grad_(True)
    loss, outs = hip_loss(B, net, xg, adj, mode)
    loss.backward()
    torch.cuda.synchronize()
    pg = net.flat_grad_buffer().detach()[:net.param_count].clone() if any(
        p.requires_grad for p in net.parameters()) else None
    return xg.grad, pg, outs


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_fp64_judge(B, shape, mode, n):
    """x.grad of sum(Ry y + RJ J + RL lap) against the fp64 judge; the parameter gradients of the same
    call equal those of a flag-off twin bit for bit (they come from the same kernels)."""
    din, dout, L, W = shape
    ref, ref64, net, twin = nets(B, shape)
    x, adj = points(n, din, seed=n), weights(n, din, dout)
    want = judge(B, shape, mode, n)
    gx, pg, _ = hip_run(B, net, x, adj, mode)
    gx_off, pg_off, _ = hip_run(B, twin, x, adj, mode)
    assert gx is not None and gx.shape == (n, din) and gx_off is None
    assert bool(torch.isfinite(gx).all())
    e = nerr(gx, want)
    fig("parity", "shape=%s" % (shape,), "mode=" + mode, "n=%d" % n, "err=%.2e" % e)
    assert torch.equal(pg, pg_off)
    if n > 1:
        assert e <= TOL, e
        return
    g32 = oracle_xgrad(ref, x, adj, mode)[0]
    e_ref = (g32.double() - want).abs()
    e_hip = (gx.detach().cpu().double() - want).abs()
    bound = torch.maximum(3 * e_ref, TOL * want.abs().max().expand_as(want))
    fig("parity-n1", "shape=%s" % (shape,), "mode=" + mode, "hip=%.2e" % float(e_hip.max()),
        "oracle32=%.2e" % float(e_ref.max()))
    assert bool((e_hip <= bound).all()), (float(e_hip.max()), float(e_ref.max()))


@pytest.mark.parametrize("mode", list(MODES))
def test_frozen_network(B, mode):
    """Every parameter frozen, x requires grad: the forward saves its streams for the x-adjoint alone."""
    shape, n = (2, 1, 4, 128), 65
    din, dout, L, W = shape
    ref, ref64, _, _ = nets(B, shape)
    torch.manual_seed(1)
    net = B.MLP(din, dout, L, W, nonlinearity="sine", coord_grad=True).cuda()
    for p in net.parameters():
        p.requires_grad_(False)
    x, adj = points(n, din, seed=n), weights(n, din, dout)
    gx, pg, _ = hip_run(B, net, x, adj, mode)
    assert gx is not None and pg is None and all(p.grad is None for p in net.parameters())
    e = nerr(gx, judge(B, shape, mode, n))
    fig("frozen", "mode=" + mode, "err=%.2e" % e)
    assert e <= TOL, e


def _through_coords_nets(B, frozen_g):
    fs, gs = (2, 2, 3, 64), (2, 1, 4, 128)
    torch.manual_seed(21)
    fr = O.OracleSiren(*fs)
    torch.manual_seed(22)
    gr = O.OracleSiren(*gs)
    torch.manual_seed(21)
    f = B.MLP(*fs, nonlinearity="sine").cuda()  # coord_grad off: nothing asks for the adjoint of ITS x
    torch.manual_seed(22)
    g = B.MLP(*gs, nonlinearity="sine", coord_grad=True).cuda()
    if frozen_g:
        for p in list(g.parameters()) + list(gr.parameters()):
            p.requires_grad_(False)
    return fr, gr, f, g


def _through_coords_body(f, g, x):
    return torch.mean(g(x + 0.05 * f(x)) ** 2)


@pytest.mark.parametrize("frozen_g", [False, True])
def test_gradient_through_coordinates(B, frozen_g):
    """loss = mean(g(x + 0.05 f(x))^2): f's parameter gradients flow through the coordinates of g's call
    (a learned deformation).  Every parameter tensor of f and g against the fp64 judge; then the same body
    under the training loop's lowering() + deferred_jets() scopes, and with each network call in a
    fused_forwards scope of its own (a scope takes calls, not consumers of their values): x.grad and the
    parameter gradients equal the plain run's to 2e-6."""
    from base import lower
    fr, gr, f, g = _through_coords_nets(B, frozen_g)
    x = points(300, 2, seed=23)
    f64, g64 = copy.deepcopy(fr).double(), copy.deepcopy(gr).double()
    _through_coords_body(f64, g64, x.double()).backward()

    def grads():
        torch.cuda.synchronize()
        return [None if p.grad is None else p.grad.detach().clone() for p in list(f.parameters()) + list(g.parameters())]

    def run(scope):
        f.zero_grad(set_to_none=True)
        g.zero_grad(set_to_none=True)
        xg = x.cuda().requires_grad_(True)
        if scope == "plain":
            loss = _through_coords_body(f, g, xg)
        elif scope == "lowering":
            with lower.lowering(), lower.deferred_jets():
                losses = {"main": _through_coords_body(f, g, xg)}
            loss = lower.lower_losses(losses)["main"]
        else:
            with B.fused_forwards():
                fx = f(xg)
            xw = xg + 0.05 * fx
            with B.fused_forwards():
                y = g(xw)
            loss = torch.mean(y ** 2)
        loss.backward()
        return grads(), xg.grad.detach().clone(), float(loss.detach())

    plain, gx_plain, loss_plain = run("plain")
    names = ["f." + k for k, _ in fr.named_parameters()] + ["g." + k for k, _ in gr.named_parameters()]
    want = [p.grad for p in list(f64.parameters()) + list(g64.parameters())]
    for k, a, b in zip(names, plain, want):
        if b is None:
            assert a is None, k
            continue
        assert a is not None, k + ": no gradient reached this tensor"
        e = nerr(a, b)
        fig("through-coords", "frozen_g=%s" % frozen_g, k, "err=%.2e" % e)
        assert e <= TOL, (k, e)
    for scope in ("lowering", "fused"):
        got, gx, loss = run(scope)
        assert abs(loss - loss_plain) <= ORDER * abs(loss_plain), scope
        e = nerr(gx, gx_plain)
        fig("through-coords", "frozen_g=%s" % frozen_g, scope, "x.grad vs plain %.2e" % e)
        assert e <= ORDER, (scope, e)
        for k, a, b in zip(names, got, plain):
            assert (a is None) == (b is None), (scope, k)
            if b is not None:
                e = nerr(a, b)
                assert e <= ORDER, (scope, k, e)


@pytest.mark.parametrize("mode", list(MODES))
def test_flag_off_changes_nothing(B, mode):
    """Flag off: x.grad stays None; outputs and parameter gradients are the flag-on run's bit for bit."""
    shape, n = (2, 2, 3, 64), 300
    _, _, net, twin = nets(B, shape)
    x, adj = points(n, 2, seed=n), weights(n, 2, 2)
    gx, pg, outs = hip_run(B, net, x, adj, mode)
    gx_off, pg_off, outs_off = hip_run(B, twin, x, adj, mode)
    assert gx is not None and gx_off is None
    assert torch.equal(pg, pg_off)
    for a, b in zip(outs, outs_off):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)


def test_batched_backward_deferred_sums_and_adam_step(B):
    """Inside batched_backward + defer_reductions with a FusedAdam step: x.grad is the immediate run's bit
    for bit (the x-launch joins no queue), and the updated parameters are the flag-off run's bit for bit."""
    shape, n, mode = (2, 1, 4, 128), 300, "lap"
    x, adj = points(n, 2, seed=31), weights(n, 2, 1, seed=32)

    def run(flag, scoped):
        torch.manual_seed(33)
        net = B.MLP(*shape, nonlinearity="sine", coord_grad=flag).cuda()
        opt = B.FusedAdam([{"params": list(net.parameters()), "lr": 1e-3, "module": net}])
        opt.zero_grad()
        xg = x.cuda().requires_grad_(True)
        if scoped:
            with B._jet.defer_reductions():
                loss, _ = hip_loss(B, net, xg, adj, mode)
                with B._jet.batched_backward():
                    loss.backward()
                opt.step()
        else:
            loss, _ = hip_loss(B, net, xg, adj, mode)
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        return xg.grad, net.flat_params().detach()[:net.param_count].clone()

    gx_scoped, p_scoped = run(True, True)
    gx_now, _ = run(True, False)
    gx_off, p_off = run(False, True)
    assert gx_off is None and gx_scoped is not None
    assert torch.equal(gx_scoped, gx_now)
    assert torch.equal(p_scoped, p_off)


def test_two_runs_are_bit_identical(B):
    shape, n = (3, 3, 4, 128), 300
    _, _, net, _ = nets(B, shape)
    x, adj = points(n, 3, seed=41), weights(n, 3, 3, seed=42)
    a, pa, _ = hip_run(B, net, x, adj, "lap")
    b, pb, _ = hip_run(B, net, x, adj, "lap")
    assert torch.equal(a, b) and torch.equal(pa, pb)


def test_graph_capture_replay_equals_eager(B):
    """One forward + backward captured with torch.cuda.graph: the replay's x.grad and parameter gradients
    are the eager run's bit for bit (the x-launch allocates nothing outside torch's pool and keeps no state)."""
    shape, n, mode = (2, 1, 4, 128), 300, "lap"
    torch.manual_seed(51)
    net = B.MLP(*shape, nonlinearity="sine", coord_grad=True).cuda()
    x, adj = points(n, 2, seed=52), weights(n, 2, 1, seed=53)
    adj_d = tuple(a.cuda() for a in adj)
    gx_eager, pg_eager, _ = hip_run(B, net, x, adj, mode)
    xs = x.cuda().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up on the capture stream: scratch and pools exist before the capture
            net.zero_grad(set_to_none=True)
            xs.grad = None
            hip_loss(B, net, xs, adj_d, mode)[0].backward()
        torch.cuda.synchronize()
        net.zero_grad(set_to_none=True)
        xs.grad = None
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            hip_loss(B, net, xs, adj_d, mode)[0].backward()
    torch.cuda.current_stream().wait_stream(s)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(xs.grad, gx_eager)
    assert torch.equal(net.flat_grad_buffer().detach()[:net.param_count], pg_eager)


def test_c_abi_direct_call(B):
    """insr_siren_jet_bwd_x at n = 17, d_in = 2 into a (32, 2) buffer of sentinels, the saved streams
    NaN-filled before the forward: rows 0..16 are written (finite, the judge's), rows 17..31 keep the
    sentinel; with every adjoint NULL the 17 rows are zero."""
    nat = B._native
    lib = nat.lib()
    shape, n, mode = (2, 1, 4, 128), 17, "lap"
    din, dout, L, W = shape
    _, _, net, _ = nets(B, shape)
    x, adj = points(n, din, seed=n), weights(n, din, dout)
    dev = torch.device("cuda")
    xg = x.cuda().contiguous()
    net.ensure_packed()
    net.ensure_wsplit()
    cmode = net.call_mode(MODES[mode])
    assert lib.insr_siren_jet_bwd_x_supported(din, dout, L, W, cmode) == 1
    flat = net.flat_params()
    y = torch.empty(n, dout, device=dev)
    J = torch.empty(n, dout, din, device=dev)
    lap = torch.empty(n, dout, device=dev)
    act = torch.full((lib.insr_jet_act_bytes(n, din, L, W, cmode) // 4,), float("nan"), device=dev)
    st = nat.stream_of(dev)
    assert lib.insr_siren_jet_fwd(nat.ptr(xg), n, din, dout, L, W, cmode, nat.ptr(flat), nat.ptr(y), nat.ptr(J),
                                  nat.ptr(lap), nat.ptr(act), st) == 0
    gy, gJ, gl = (a.cuda().contiguous() for a in adj)
    sentinel = -12345.5
    gx = torch.full((32, din), sentinel, device=dev)
    assert lib.insr_siren_jet_bwd_x(n, din, dout, L, W, cmode, nat.ptr(flat), nat.ptr(act), nat.ptr(gy), nat.ptr(gJ),
                                    nat.ptr(gl), nat.ptr(gx), st) == 0
    torch.cuda.synchronize()
    assert bool((gx[n:] == sentinel).all())
    assert bool(torch.isfinite(gx[:n]).all()) and not bool((gx[:n] == sentinel).any())
    e = nerr(gx[:n], judge(B, shape, mode, n))
    fig("c-abi", "err=%.2e" % e)
    assert e <= TOL, e
    assert lib.insr_siren_jet_bwd_x(n, din, dout, L, W, cmode, nat.ptr(flat), nat.ptr(act), None, None, None,
                                    nat.ptr(gx), st) == 0
    torch.cuda.synchronize()
    assert bool((gx[:n] == 0).all()) and bool((gx[n:] == sentinel).all())


def test_fallback_recompute_policy(B):
    """Knob policy 4 (the recompute backward: the forward saves no streams): the x-adjoint takes the torch
    route, counted in REF_STATS["x_backward"], and matches the judge."""
    nat = B._native
    shape, n, mode = (2, 1, 4, 128), 65, "lap"
    _, _, net, _ = nets(B, shape)
    x, adj = points(n, 2, seed=n), weights(n, 2, 1)
    before = B._jet.REF_STATS["x_backward"]
    B._jet._X_WARNED.clear()  # (the warning is once per shape and process)
    with nat.knobs(policy=4):
        assert nat.lib().insr_jet_bwd_path(n, 2, 1, 4, 128, net.call_mode(2)) == 3
        with pytest.warns(UserWarning, match="coordinate gradient"):
            gx, _, _ = hip_run(B, net, x, adj, mode)
    assert B._jet.REF_STATS["x_backward"] == before + 1
    e = nerr(gx, judge(B, shape, mode, n))
    fig("fallback-recompute", "err=%.2e" % e)
    assert e <= TOL, e


def test_fallback_hessian_jet(B):
    """The second-order jet node with the flag on: the (third-order) x-adjoint through torch ops."""
    shape, n = (2, 1, 2, 32), 17
    din, dout, L, W = shape
    torch.manual_seed(61)
    ref = O.OracleSiren(*shape)
    torch.manual_seed(61)
    net = B.MLP(*shape, nonlinearity="sine", hessian_jet=True, coord_grad=True).cuda()
    x = points(n, din, seed=62)
    g = torch.Generator().manual_seed(63)
    Ry, RJ, RH = torch.rand(n, dout, generator=g) + 0.5, torch.randn(n, dout, din, generator=g), torch.randn(
        n, dout, din, din, generator=g)
    ref64 = copy.deepcopy(ref).double()
    xr = x.double().requires_grad_(True)
    yr = ref64(xr)
    ((yr * Ry.double()).sum() + (O.op_jacobian(yr, xr)[0] * RJ.double()).sum()
     + (O.op_hessian(yr, xr)[0] * RH.double()).sum()).backward()
    before = B._jet.REF_STATS["x_backward"]
    B._jet._X_WARNED.clear()
    xg = x.cuda().requires_grad_(True)
    y, J, H = B._hess.run_hess_jet(net, xg)
    with pytest.warns(UserWarning, match="coordinate gradient"):
        ((y * Ry.cuda()).sum() + (J * RJ.cuda()).sum() + (H * RH.cuda()).sum()).backward()
        torch.cuda.synchronize()
    assert B._jet.REF_STATS["x_backward"] == before + 1
    e = nerr(xg.grad, xr.grad)
    fig("fallback-hess", "err=%.2e" % e)
    assert e <= TOL, e
    # the parameter gradients of the same call: the reverse second-order jet's, as with the flag off
    for (k, p), q in zip(net.named_parameters(), ref64.parameters()):
        assert nerr(p.grad, q.grad) <= TOL, k


@pytest.mark.parametrize("precision", [None, "fp32"])
@pytest.mark.parametrize("shape", [(3, 3, 4, 128), (3, 1, 2, 256)])
def test_laplace_adjoint_at_the_largest_state(B, shape, precision):
    """x.grad of sum(R laplace(net(x), x)) through the public operators, five streams (d_in = 3), at the
    network's default precision and at precision='fp32' (whose width-256 five-stream jets are not compiled:
    diff_ops takes its reference-semantics route there, which returns the adjoint of x itself)."""
    din, dout, L, W = shape
    n = 65
    ref, ref64, net, _ = nets(B, shape, seed=2, precision=precision)
    x = points(n, din, seed=71)
    R = torch.randn(n, 1, generator=torch.Generator().manual_seed(72))
    xr = x.double().requires_grad_(True)
    (O.op_laplace(ref64(xr), xr) * R.double()).sum().backward()
    net.zero_grad(set_to_none=True)
    xg = x.cuda().requires_grad_(True)
    (B.laplace(net(xg), xg) * R.cuda()).sum().backward()
    torch.cuda.synchronize()
    e = nerr(xg.grad, xr.grad)
    fig("laplace-adjoint", "shape=%s" % (shape,), "precision=%s" % precision, "err=%.2e" % e)
    assert e <= TOL, e
