"""The saved-stream reverse sweep (policy 5: csrc/jet_fb.hpp with SAVED = true) after its VALU diet:
the fp16 split by mixed-precision FMAs (csrc/jet_x6.hpp splitq<4>) and one sin / cos per reverse
layer (the pair computed for h_{j-1}'s planes is layer j - 1's sine reverse's too) -- vs the CPU
oracle, every parameter gradient normwise max|hip - ref| <= 1e-5 max|ref| (the suite's tolerance),
at two tiles (n = 17), three (n = 33) and a ragged batch of several tiles per block (n = 4,113: the
carried pair and the two stream sets start every tile in the same roles); the 2-d gradient and the
value jets; the 5 x 128 gradient jet (an odd layer count: the sets end swapped); each backward run
twice, on two networks of the same seed, with equal bits.

The large-argument case is the suite's own (tests/test_gpu_resident_f16.py
test_large_tangents_stay_finite: first layer x 4000, 2,000 points, Laplacian and gradient adjoints,
finite and within 1e-5 of the all-bf16x6 two-kernel run): its layer-0 sine arguments reach 30 x
2,000 x |x|, far past the fast range's 8,192, so the pair that is carried into the first layer's
sine reverse is the libm one.
"""
import pytest
import torch

from oracle import siren_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5
V, G, LAP = 0, 1, 2


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


def pair(B, din, dout, L, W, seed):
    torch.manual_seed(seed)
    ref = O.OracleSiren(din, dout, L, W)
    torch.manual_seed(seed)
    net = B.MLP(din, dout, L, W, nonlinearity="sine")
    return ref, net.cuda()


def grads(net):
    return [(p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone() for p in net.parameters()]


def ref_grads(ref):
    return [(p.grad if p.grad is not None else torch.zeros_like(p)).detach() for p in ref.parameters()]


def twice(make, run):
    """run(make()) -> loss of a fresh GPU net, backward, twice; the gradients must agree bit for bit."""
    out = []
    for _ in range(2):
        net = make()
        run(net).backward()
        torch.cuda.synchronize()
        out.append(grads(net))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    return out[0]


def check(ref, got, tag):
    for (k, _), a, b in zip(ref.named_parameters(), ref_grads(ref), got):
        e = nerr(b, a)
        print(tag, k, f"{e:.3e}")
        assert e < TOL, (tag, k, e)


@pytest.mark.parametrize("n", [17, 33, 4113])
def test_laplace_jet_all_adjoints(B, n):
    """2 -> 1, 4 x 128: adjoints on the value, the gradient and the Laplacian."""
    assert B._native.lib().insr_jet_bwd_path(n, 2, 1, 4, 128, LAP | B._native.scope_bits()) == 2
    ref, _ = pair(B, 2, 1, 4, 128, seed=81)
    x = torch.rand(n, 2, generator=torch.Generator().manual_seed(n)) * 2 - 1
    xr = x.clone().requires_grad_(True)
    yr = ref(xr)
    gr, lr_ = O.op_gradient(yr, xr), O.op_laplace(yr, xr)
    g = torch.Generator().manual_seed(n + 1)
    Ry, Rg, Rl = torch.randn(yr.shape, generator=g), torch.randn(gr.shape, generator=g), torch.randn(lr_.shape, generator=g)
    ((yr * Ry).sum() + (gr * Rg).sum() + (lr_ * Rl).sum()).backward()

    def run(net):
        xg = x.cuda().requires_grad_(True)
        y = net(xg)
        lp, gp = B.laplace(y, xg, return_grad=True)
        return (y * Ry.cuda()).sum() + (gp * Rg.cuda()).sum() + (lp * Rl.cuda()).sum()

    check(ref, twice(lambda: pair(B, 2, 1, 4, 128, seed=81)[1], run), ("lap", n))


@pytest.mark.parametrize("kind", ["value", "jacobian"])
def test_value_and_gradient_jets(B, kind):
    """2 -> 2, 4 x 128 at 33 points."""
    n = 33
    mode = V if kind == "value" else G
    assert B._native.lib().insr_jet_bwd_path(n, 2, 2, 4, 128, mode | B._native.scope_bits()) == 2
    ref, _ = pair(B, 2, 2, 4, 128, seed=82)
    x = torch.rand(n, 2, generator=torch.Generator().manual_seed(3)) * 2 - 1
    xr = x.clone().requires_grad_(True)
    vr = ref(xr) if kind == "value" else O.op_jacobian(ref(xr), xr)[0]
    R = torch.randn(vr.shape, generator=torch.Generator().manual_seed(4))
    (vr * R).sum().backward()

    def run(net):
        xg = x.cuda().requires_grad_(True)
        v = net(xg) if kind == "value" else B.jacobian(net(xg), xg)[0]
        return (v * R.cuda()).sum()

    check(ref, twice(lambda: pair(B, 2, 2, 4, 128, seed=82)[1], run), (kind, n))


def test_five_layer_gradient_jet(B):
    """2 -> 2, 5 x 128 at 4,113 points: the Jacobian of f(x) + x."""
    n = 4113
    assert B._native.lib().insr_jet_bwd_path(n, 2, 2, 5, 128, G | B._native.scope_bits()) == 2
    ref, _ = pair(B, 2, 2, 5, 128, seed=83)
    x = torch.rand(n, 2, generator=torch.Generator().manual_seed(n)) * 2 - 1
    xr = x.clone().requires_grad_(True)
    Jr = O.op_jacobian(ref(xr) + xr, xr)[0]
    R = torch.randn(Jr.shape, generator=torch.Generator().manual_seed(n + 3))
    (Jr * R).sum().backward()

    def run(net):
        xg = x.cuda().requires_grad_(True)
        return (B.jacobian(net(xg) + xg, xg)[0] * R.cuda()).sum()

    check(ref, twice(lambda: pair(B, 2, 2, 5, 128, seed=83)[1], run), ("jac5", n))


def test_large_arguments_carry_the_libm_pair(B):
    """Inputs and bound of tests/test_gpu_resident_f16.py test_large_tangents_stay_finite."""
    out = []
    for pol, prec, f16 in ((5, None, 7), (2, "bf16x6", 0)):
        with B._native.knobs(policy=pol, bwd_f16=f16):
            x = torch.rand(2000, 2, generator=torch.Generator().manual_seed(7)) * 2 - 1

            def make():
                torch.manual_seed(75)
                net = B.MLP(2, 1, 4, 128, nonlinearity="sine", precision=prec).cuda()
                with torch.no_grad():
                    net.net[0].weight.mul_(4000.0)
                w0 = net.net[0].weight.detach().cpu()
                assert float((30.0 * (w0 @ x.t()).abs()).max()) > 8192.0 * 2  # well past the fast range
                return net

            def run(net):
                xg = x.cuda().requires_grad_(True)
                lp, gp = B.laplace(net(xg), xg, return_grad=True)
                R = torch.randn(lp.shape, generator=torch.Generator().manual_seed(8)).cuda()
                return (lp * R).sum() + (gp ** 2).sum()

            out.append(twice(make, run))
    for a, b in zip(*out):
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        e = nerr(a, b)
        print("large", f"{e:.3e}")
        assert e < TOL
