"""Second-order jets on the GPU (csrc/jet_hess.hpp, base/_hess.py): y, J and the full Hessian of
d_in = 2 / 3 SIRENs from one forward launch, every parameter gradient from one reverse launch.
Judge: the oracle (oracle/siren_oracle.py, the reference's autograd operators in fp32 on the CPU) at the
project's 1e-5 normwise contract, per output field and per parameter tensor; single
points and the off-domain / high-frequency stress are judged against fp64 relative to the oracle's
own fp32 error, as the existing Laplacian and polarisation tests are."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import siren_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5
GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_ops.npz")
NETS = [(2, 1, 2, 32), (2, 2, 3, 64), (3, 1, 2, 32), (3, 3, 4, 128), (2, 1, 4, 128)]


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


def pair(B, shape, seed=0):
    din, dout, L, W = shape
    torch.manual_seed(seed)
    ref = O.OracleSiren(din, dout, L, W)
    torch.manual_seed(seed)
    net = B.MLP(din, dout, L, W, nonlinearity="sine", hessian_jet=True).cuda()
    return ref, net


def grads_of(net):
    return [(p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().cpu() for p in net.parameters()]


def check_grads(ref, net, tol=TOL):
    names = [k for k, _ in ref.named_parameters()]
    for k, ga, gb in zip(names, grads_of(ref), grads_of(net)):
        if float(ga.abs().max()) == 0.0:
            assert float(gb.abs().max()) == 0.0, k
            continue
        e = nerr(gb, ga)
        print(f"  grad {k}: {e:.2e}")
        assert e < tol, (k, e)


def points(n, din, seed=3):
    return torch.rand(n, din, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def weights(n, din, dout, seed=5):
    """Adjoints of (y, J, H): random, H's not symmetric.  The value adjoint is of one sign (uniform in
    [0.5, 1.5]): the output bias's gradient is the plain sum of the value adjoints over the points, a tensor
    of d_out elements, and a signed random adjoint makes its "normwise" error the cancellation error of a
    near-zero fp32 sum (which the fp32 oracle has as much as the kernel), not a property of the jet."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, dout, generator=g) + 0.5, torch.randn(n, dout, din, generator=g),
            torch.randn(n, dout, din, din, generator=g))


def oracle_fields(ref, x):
    xr = x.clone().requires_grad_(True)
    y = ref(xr)
    return y, O.op_jacobian(y, xr)[0], O.op_hessian(y, xr)[0], xr


@pytest.mark.parametrize("n", [1, 15, 17, 64, 65, 300])
@pytest.mark.parametrize("shape", NETS)
def test_parity_with_oracle(B, shape, n):
    """y, J, H (H with a non-symmetric weight) and every parameter tensor's gradient of
    sum(Ry y + RJ J + RH H): 1e-5 normwise against the fp32 oracle.  n = 1 makes "normwise" pointwise: there
    the judge is fp64 and the HIP error must stay within 3x the oracle's own fp32 error (or 1e-5)."""
    din, dout, L, W = shape
    ref, net = pair(B, shape, seed=1)
    x = points(n, din, seed=n)
    Ry, RJ, RH = weights(n, din, dout)
    yr, Jr, Hr, _ = oracle_fields(ref, x)
    ((yr * Ry).sum() + (Jr * RJ).sum() + (Hr * RH).sum()).backward()
    xg = x.cuda().requires_grad_(True)
    y, J, H = B._hess.run_hess_jet(net, xg)
    assert y.shape == (n, dout) and J.shape == (n, dout, din) and H.shape == (n, dout, din, din)
    ((y * Ry.cuda()).sum() + (J * RJ.cuda()).sum() + (H * RH.cuda()).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(H, H.transpose(-1, -2))  # both triangles written from one stream
    if n > 1:
        for name, a, b in (("y", y, yr), ("J", J, Jr), ("H", H, Hr)):
            e = nerr(a, b)
            print(f"  {name}: {e:.2e}")
            assert e < TOL, (name, e)
        check_grads(ref, net)
        return
    ref64 = copy.deepcopy(ref).double()
    ref64.zero_grad(set_to_none=True)
    y6, J6, H6, _ = oracle_fields(ref64, x.double())
    ((y6 * Ry.double()).sum() + (J6 * RJ.double()).sum() + (H6 * RH.double()).sum()).backward()
    for name, a, b, c in (("y", y, yr, y6), ("J", J, Jr, J6), ("H", H, Hr, H6)):
        c = c.detach()
        e_ref = (b.detach().double() - c).abs()
        e_hip = (a.detach().cpu().double() - c).abs()
        bound = torch.maximum(3 * e_ref, TOL * c.abs().max().expand_as(c))
        assert bool((e_hip <= bound).all()), (name, e_hip.max().item(), e_ref.max().item())
    for k, g6, g32, gg in zip([k for k, _ in ref.named_parameters()], grads_of(ref64), grads_of(ref), grads_of(net)):
        e_ref, e_hip = nerr(g32, g6), nerr(gg, g6)
        assert e_hip <= max(3 * e_ref, TOL), (k, e_hip, e_ref)


@pytest.mark.parametrize("name", ["fluid_vel", "fluid_pres", "el2d"])
def test_reference_goldens(B, name):
    """The reference's own Hessians and the parameter gradients of a random functional of them
    (tests/golden/ref_ops.npz), both at 1e-5 (the polarised route holds the gradients to 1e-4)."""
    ops = dict(np.load(GOLD))
    din, dout, L, W = (int(v) for v in ops[f"{name}/shape"])
    torch.manual_seed(int(ops[f"{name}/seed"]))
    net = B.MLP(din, dout, L, W, nonlinearity="sine", hessian_jet=True).cuda()
    x3 = torch.from_numpy(ops[f"{name}/x"])[None].cuda().requires_grad_(True)
    h, st = B.hessian(net(x3), x3)
    assert st == int(ops[f"{name}/hessian_status"])
    assert h.shape == ops[f"{name}/hessian"].shape
    e = nerr(h, ops[f"{name}/hessian"])
    print(f"  hessian: {e:.2e}")
    assert e < TOL
    net.zero_grad(set_to_none=True)
    (h * torch.from_numpy(ops[f"{name}/hessian_R"]).cuda()).sum().backward()
    g = net.flat_grad_buffer().detach().cpu().numpy()[:net.param_count]
    e = nerr(g[::int(ops[f"{name}/param_stride"])], ops[f"{name}/hessian_pgrad"])
    print(f"  hessian_pgrad: {e:.2e}")
    assert e < TOL


@pytest.mark.parametrize("scale_x,scale_w0", [(4.0, 1.0), (1.0, 3.0), (8.0, 3.0)])
def test_off_domain_and_high_frequency(B, scale_x, scale_w0):
    """Points up to |x| = 8 and a first layer scaled x3, judged against fp64 autograd of the oracle: the
    HIP error stays within 5x the oracle's own fp32 error (or 1e-5) -- the polarisation test's rule."""
    torch.manual_seed(17)
    net = B.MLP(2, 1, 4, 128, nonlinearity="sine", hessian_jet=True).cuda()
    with torch.no_grad():
        net.net[0].weight.mul_(scale_w0)
    ref32 = O.OracleSiren(2, 1, 4, 128)
    ref32.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    ref64 = copy.deepcopy(ref32).double()
    x = (torch.rand(512, 2, generator=torch.Generator().manual_seed(18)) * 2 - 1) * scale_x
    xg = x.cuda().requires_grad_(True)
    h, st = B.hessian(net(xg), xg)
    x64 = x.double().requires_grad_(True)
    h64, _ = O.op_hessian(ref64(x64), x64)
    x32 = x.clone().requires_grad_(True)
    h32, _ = O.op_hessian(ref32(x32), x32)
    e_hip, e32 = nerr(h, h64), nerr(h32, h64)
    print(f"  hip {e_hip:.2e} oracle-fp32 {e32:.2e}")
    assert st == 0 and e_hip <= max(5 * e32, TOL), (e_hip, e32)


@pytest.mark.parametrize("which", ["ghess", "gy", "all"])
def test_adjoint_subsets(B, which):
    """Only the Hessian adjoint, only the value adjoint (the others NULL: no zero-fill), and y, J, H of
    one node in one loss."""
    shape = (3, 2, 2, 64)
    ref, net = pair(B, shape, seed=2)
    n = 100
    x = points(n, 3, seed=7)
    Ry, RJ, RH = weights(n, 3, 2, seed=8)
    yr, Jr, Hr, _ = oracle_fields(ref, x)
    xg = x.cuda().requires_grad_(True)
    y, J, H = B._hess.run_hess_jet(net, xg)
    if which == "ghess":
        lr_, lg = (Hr * RH).sum(), (H * RH.cuda()).sum()
    elif which == "gy":
        lr_, lg = (yr * Ry).sum(), (y * Ry.cuda()).sum()
    else:
        lr_ = (yr * Ry).sum() + ((Jr * RJ) ** 2).sum() + (Hr * RH).sum() * 1e-2
        lg = (y * Ry.cuda()).sum() + ((J * RJ.cuda()) ** 2).sum() + (H * RH.cuda()).sum() * 1e-2
    lr_.backward()
    lg.backward()
    torch.cuda.synchronize()
    check_grads(ref, net)


def test_affine_field_has_the_network_hessian(B):
    """q = f(x) + x: the identity part has zero Hessian."""
    ref, net = pair(B, (2, 2, 3, 64), seed=3)
    x = points(65, 2, seed=4)
    xr = x.clone().requires_grad_(True)
    Hr, _ = O.op_hessian(ref(xr) + xr, xr)
    xg = x.cuda().requires_grad_(True)
    before = sum(B.diff_ops.HESS_JETS.values())
    H, st = B.hessian(net(xg) + xg, xg)
    assert sum(B.diff_ops.HESS_JETS.values()) == before + 1
    assert st == 0 and H.shape == Hr.shape and nerr(H, Hr) < TOL
    R = torch.randn(Hr.shape, generator=torch.Generator().manual_seed(6))
    (Hr * R).sum().backward()
    (H * R.cuda()).sum().backward()
    torch.cuda.synchronize()
    check_grads(ref, net)


def test_routing_hessian_3d(B):
    ref, net = pair(B, (3, 2, 2, 64))
    x = points(300, 3).unsqueeze(0)
    xg = x.cuda().requires_grad_(True)
    jets, falls = sum(B.diff_ops.HESS_JETS.values()), sum(B.diff_ops.FALLBACKS.values())
    H, st = B.hessian(net(xg), xg)
    assert sum(B.diff_ops.HESS_JETS.values()) == jets + 1
    assert sum(B.diff_ops.FALLBACKS.values()) == falls
    assert st == 0 and H.shape == (1, 300, 2, 3, 3)
    xr = x.clone().requires_grad_(True)
    Hr, _ = O.op_hessian(ref(xr), xr)
    assert nerr(H, Hr) < TOL
    # the flag off: the present route (the reference-semantics fallback for d_in = 3), the same field
    net.hessian_jet = False
    xg2 = x.cuda().requires_grad_(True)
    H2, _ = B.hessian(net(xg2), xg2)
    assert sum(B.diff_ops.HESS_JETS.values()) == jets + 1
    assert sum(B.diff_ops.FALLBACKS.values()) == falls + 1
    assert nerr(H2, Hr) < TOL


def test_routing_laplace_normalized_3d(B):
    ref, net = pair(B, (3, 1, 3, 64))
    x = points(300, 3)
    xr = x.clone().requires_grad_(True)
    g = O.op_gradient(ref(xr), xr)
    dr = O.op_divergence(g / (g.norm(dim=-1, keepdim=True) + 1.0), xr)
    xg = x.cuda().requires_grad_(True)
    jets, falls = sum(B.diff_ops.HESS_JETS.values()), sum(B.diff_ops.FALLBACKS.values())
    dg = B.laplace(net(xg), xg, normalize=True, eps=1.0)
    assert sum(B.diff_ops.HESS_JETS.values()) == jets + 1 and sum(B.diff_ops.FALLBACKS.values()) == falls
    assert dg.shape == dr.shape
    e = nerr(dg, dr)
    print(f"  normalised laplace: {e:.2e}")
    assert e < TOL
    w = torch.randn(dr.shape, generator=torch.Generator().manual_seed(5))
    (w * dr).sum().backward()
    (w.cuda() * dg).sum().backward()
    torch.cuda.synchronize()
    check_grads(ref, net)


def test_mixed_loss_and_fused_adam_step(B):
    """mean(H^2) + a fused Laplacian term in one loss, backward + FusedAdam.step inside defer_reductions:
    the gradients are the oracle's and the step is the oracle's (test_fallback_keeps_the_training_step's bound)."""
    shape = (2, 1, 3, 64)
    ref, net = pair(B, shape, seed=6)
    x = points(256, 2, seed=2)
    xr = x.clone().requires_grad_(True)
    yr = ref(xr)
    loss_r = (O.op_hessian(yr, xr)[0] ** 2).mean() + (O.op_laplace(ref(xr), xr) ** 2).mean()
    loss_r.backward()

    def loss_of():
        xg = x.cuda().requires_grad_(True)
        return (B.hessian(net(xg), xg)[0] ** 2).mean() + (B.laplace(net(xg), xg) ** 2).mean()

    net.zero_grad(set_to_none=True)
    loss = loss_of()
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_r)) <= TOL * abs(float(loss_r))
    check_grads(ref, net)
    opt_r = O.OracleAdam(list(ref.parameters()), lr=1e-4)
    opt_r.step()
    opt = B.FusedAdam([{"params": list(net.parameters()), "lr": 1e-4, "module": net}])
    opt.zero_grad()
    with B._jet.defer_reductions():
        loss_of().backward()
        opt.step()
    torch.cuda.synchronize()
    for a, b in zip(ref.parameters(), net.parameters()):
        assert float((a.detach() - b.detach().cpu()).abs().max()) <= 2.5e-4  # Adam's first step ~ lr sign(g)


def test_c_abi_with_poisoned_buffers(B):
    """insr_siren_hess_fwd / _bwd at n = 17 with the saved streams and the partial rows NaN-filled
    beforehand: every float the sums read was written; finite and equal to the oracle."""
    nat = B._native
    lib = nat.lib()
    shape = (3, 2, 3, 64)
    din, dout, L, W = shape
    ref, net = pair(B, shape, seed=9)
    n = 17
    x = points(n, din, seed=10)
    Ry, RJ, RH = weights(n, din, dout, seed=11)
    yr, Jr, Hr, _ = oracle_fields(ref, x)
    ((yr * Ry).sum() + (Jr * RJ).sum() + (Hr * RH).sum()).backward()
    dev = torch.device("cuda")
    xg = x.cuda().contiguous()
    flat = net.flat_params()
    y = torch.full((n, dout), float("nan"), device=dev)
    J = torch.full((n, dout, din), float("nan"), device=dev)
    H = torch.full((n, dout, din, din), float("nan"), device=dev)
    act = torch.full((lib.insr_hess_act_bytes(n, din, L, W) // 4,), float("nan"), device=dev)
    st = nat.stream_of(dev)
    assert lib.insr_siren_hess_fwd(nat.ptr(xg), n, din, dout, L, W, nat.ptr(flat), nat.ptr(y), nat.ptr(J), nat.ptr(H),
                                   nat.ptr(act), st) == 0
    nb, stride = lib.insr_hess_partial_blocks(n, din, W), lib.insr_jet_partial_stride(din, dout, L, W)
    assert nb == 2 and lib.insr_hess_partial_bytes(n, din, dout, L, W) == nb * stride * 4
    part = torch.full((nb * stride,), float("nan"), device=dev)
    gy, gJ, gH = Ry.cuda().contiguous(), RJ.cuda().contiguous(), RH.cuda().contiguous()
    assert lib.insr_siren_hess_bwd(nat.ptr(xg), n, din, dout, L, W, nat.ptr(flat), nat.ptr(act), nat.ptr(gy),
                                   nat.ptr(gJ), nat.ptr(gH), nat.ptr(part), st) == 0
    grad = torch.full((net.param_count,), float("nan"), device=dev)
    assert lib.insr_reduce_partials_strided(nat.ptr(part), nb, net.param_count, stride, nat.ptr(grad), 0, st) == 0
    torch.cuda.synchronize()
    for name, a, b in (("y", y, yr), ("J", J, Jr), ("H", H, Hr)):
        assert bool(torch.isfinite(a).all()), name
        assert nerr(a, b) < TOL, (name, nerr(a, b))
    assert bool(torch.isfinite(grad).all())
    off = 0
    for k, p in ref.named_parameters():
        e = nerr(grad[off:off + p.numel()], p.grad.reshape(-1))
        assert e < TOL, (k, e)
        off += p.numel()


def test_two_runs_are_bit_identical(B):
    shape = (3, 3, 4, 128)
    _, net = pair(B, shape, seed=12)
    x = points(300, 3, seed=13).cuda()
    _, _, RH = weights(300, 3, 3, seed=14)
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        y, J, H = B._hess.run_hess_jet(net, xg)
        ((H * RH.cuda()).sum() + (y ** 2).sum() + J.sum()).backward()
        runs.append((y.detach().clone(), J.detach().clone(), H.detach().clone(),
                     net.flat_grad_buffer().detach().clone()))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_create_graph_through_the_node(B):
    """d/dx of sum(H . R) with create_graph=True: the node differentiates itself with torch ops
    (third-order derivatives of the network) and equals the oracle's."""
    shape = (2, 2, 3, 64)
    ref, net = pair(B, shape, seed=15)
    x = points(33, 2, seed=16)
    R = torch.randn(33, 2, 2, 2, generator=torch.Generator().manual_seed(17))
    xr = x.clone().requires_grad_(True)
    Hr, _ = O.op_hessian(ref(xr), xr)
    gr = torch.autograd.grad((Hr * R).sum(), xr, create_graph=True)[0]
    xg = x.cuda().requires_grad_(True)
    before = B._jet.REF_STATS["backward"]
    _, _, H = B._hess.run_hess_jet(net, xg)
    gg = torch.autograd.grad((H * R.cuda()).sum(), xg, create_graph=True)[0]
    assert B._jet.REF_STATS["backward"] == before + 1 and gg.requires_grad
    assert nerr(gg, gr) < TOL, nerr(gg, gr)


def test_scopes_fused_forwards_and_lowering(B):
    """Inside a fused_forwards scope hessian() raises UnsupportedPattern (its jets' values are read at
    once), flag on or off; under the loop's lowering with deferred jets it runs at once
    (lower.immediate) and returns the jet's Hessian."""
    from base import lower
    ref, net = pair(B, (3, 1, 2, 32), seed=4)
    x = points(40, 3, seed=5)
    xr = x.clone().requires_grad_(True)
    Hr, _ = O.op_hessian(ref(xr), xr)
    xg = x.cuda().requires_grad_(True)
    with B.fused_forwards():
        y = net(xg)
        with pytest.raises(B.UnsupportedPattern):
            B.hessian(y, xg)
    jets, falls = sum(B.diff_ops.HESS_JETS.values()), sum(B.diff_ops.FALLBACKS.values())
    with lower.lowering(), lower.deferred_jets():
        H, st = B.hessian(net(xg), xg)
        H = lower.materialize(H)
    assert sum(B.diff_ops.HESS_JETS.values()) == jets + 1 and sum(B.diff_ops.FALLBACKS.values()) == falls
    assert H.shape == Hr.shape and nerr(H, Hr) < TOL
