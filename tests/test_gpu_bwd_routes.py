"""Entry point x kernel cells of the backward routing that no other GPU test reaches,
straight through the C ABI: the two-phase entry insr_siren_jet_bwd_grad_adam (phases 1 then 2, and 3) on
each kernel that splits into sweep + sums, and insr_siren_jet_bwd_grad_multi's solo jobs on the two-kernel
and the resident bf16x6 kernels.

The fluid pressure net (2 -> 1, 4 x 128), Laplacian jets with adjoints on every stream, n = 17 and n = 65
(two and five tiles, the last one ragged); the kernel is forced by the per-call policy knob.  Every
parameter gradient against the CPU oracle at the suite's parity bound (1e-5 normwise per tensor,
tests/test_gpu_parity.py).
"""
import ctypes

import pytest
import torch

from oracle import siren_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5
SHAPE = (2, 1, 4, 128)
POLICY = {"wide": 2, "x6r": 3, "recompute": 4, "sweep": 5}  # the INSR_JET_POLICY code that forces a kernel
ANSWER = {"wide": (1, 0), "x6r": (2, 0), "recompute": (3, 1), "sweep": (2, 1)}  # (insr_jet_bwd_path, _kernel)


@pytest.fixture(scope="module")
def B():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import base
    base._native.load()
    return base


def nerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def case(B):
    """The network and, per n: points, the adjoints of (y, dy, lap) and the oracle's parameter gradients of
    sum(g_y y + g_dy dy + g_lap lap) -- computed once."""
    torch.manual_seed(71)
    ref = O.OracleSiren(*SHAPE)
    torch.manual_seed(71)
    net = B.MLP(*SHAPE, nonlinearity="sine").cuda()
    net.ensure_wsplit()
    data = {}
    for n in (17, 65):
        g = torch.Generator().manual_seed(n)
        x = torch.rand(n, 2, generator=g) * 2 - 1
        xr = x.clone().requires_grad_(True)
        y = ref(xr)
        dy, lap = O.op_gradient(y, xr), O.op_laplace(y, xr)
        adj = [torch.randn(t.shape, generator=g) for t in (y, dy, lap)]
        ref.zero_grad(set_to_none=True)
        sum((t * a).sum() for t, a in zip((y, dy, lap), adj)).backward()
        want = [(p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone() for p in ref.parameters()]
        data[n] = (x.cuda(), [a.contiguous().cuda() for a in adj], want)
    return ref, net, data


def forward(B, net, x, mode):
    """The forward jet of one call: its saved streams (None where the backward recomputes them)."""
    nat = B._native
    lib, n = nat.lib(), x.shape[0]
    act = None
    if lib.insr_jet_bwd_path(n, *SHAPE, mode) != 3:
        act = torch.empty(lib.insr_jet_act_bytes(n, 2, 4, 128, mode) // 4, device="cuda")
    y, dy, lap = (torch.empty(n, k, device="cuda") for k in (1, 2, 1))
    assert lib.insr_siren_jet_fwd(nat.ptr(x), n, *SHAPE, mode, nat.ptr(net.flat_params()), nat.ptr(y), nat.ptr(dy),
                                  nat.ptr(lap), nat.ptr(act), nat.stream_of(x.device)) == 0
    return act


def check(ref, flat_grad, want, what):
    sizes = [p.numel() for p in ref.parameters()]
    got = torch.split(flat_grad[:sum(sizes)], sizes)
    for (k, p), g, w in zip(ref.named_parameters(), got, want):
        e = nerr(g.reshape(p.shape), w)
        print(f"{what} {k}: {e:.3e}")
        assert e < TOL, (what, k, e)


@pytest.mark.parametrize("n", [17, 65])
@pytest.mark.parametrize("kernel", ["wide", "sweep", "recompute"])
def test_two_phase_entry_on_every_splitting_kernel(B, case, kernel, n):
    """insr_siren_jet_bwd_grad_adam without the Adam update: phases 1 then 2, and phases 3, vs the oracle."""
    ref, net, data = case
    nat = B._native
    lib = nat.lib()
    x, (gy, gdy, glap), want = data[n]
    st = nat.stream_of(x.device)
    with nat.knobs(policy=POLICY[kernel]):
        mode = net.call_mode(nat.MODE_LAP)
    assert (lib.insr_jet_bwd_path(n, *SHAPE, mode), lib.insr_jet_bwd_kernel(n, *SHAPE, mode)) == ANSWER[kernel]
    flat = net.flat_params()
    act = forward(B, net, x, mode)
    work = torch.empty(lib.insr_jet_bwd_work_bytes(n, *SHAPE, mode) // 4, device="cuda")

    def run(phases, grad):
        return lib.insr_siren_jet_bwd_grad_adam(nat.ptr(x), n, *SHAPE, mode, nat.ptr(flat), nat.ptr(act), nat.ptr(gy),
                                                nat.ptr(gdy), nat.ptr(glap), nat.ptr(work), nat.ptr(grad), 0, phases,
                                                None, None, None, 0.0, 0.0, 0.0, None, 0, st)

    g12, g3 = (torch.full((flat.numel(),), float("nan"), device="cuda") for _ in range(2))  # accumulate = 0 overwrites
    assert run(1, g12) == 0 and run(2, g12) == 0
    assert run(3, g3) == 0
    torch.cuda.synchronize()
    check(ref, g12, want, f"{kernel} n={n} phases 1+2")
    check(ref, g3, want, f"{kernel} n={n} phases 3")


@pytest.mark.parametrize("kernel", ["wide", "x6r"])
def test_multi_call_solo_jobs(B, case, kernel):
    """insr_siren_jet_bwd_grad_multi with both jobs on a kernel other than the fused one: each runs alone, the
    second accumulates onto the first."""
    ref, net, data = case
    nat = B._native
    lib = nat.lib()
    with nat.knobs(policy=POLICY[kernel]):
        mode = net.call_mode(nat.MODE_LAP)
    jobs, keep = [], []
    for n, (x, (gy, gdy, glap), _) in data.items():
        assert (lib.insr_jet_bwd_path(n, *SHAPE, mode), lib.insr_jet_bwd_kernel(n, *SHAPE, mode)) == ANSWER[kernel]
        act = forward(B, net, x, mode)
        jobs.append(nat.BwdJob(x.data_ptr(), act.data_ptr(), gy.data_ptr(), gdy.data_ptr(), glap.data_ptr(), n))
        keep.append(act)
    arr = (nat.BwdJob * len(jobs))(*jobs)
    ns = (ctypes.c_long * len(jobs))(*[j.n for j in jobs])
    flat = net.flat_params()
    work = torch.empty(lib.insr_jet_bwd_multi_work_bytes(ns, len(jobs), *SHAPE, mode) // 4, device="cuda")
    grad = torch.full((flat.numel(),), float("nan"), device="cuda")
    assert lib.insr_siren_jet_bwd_grad_multi(arr, len(jobs), *SHAPE, mode, nat.ptr(flat), nat.ptr(work), nat.ptr(grad),
                                             0, nat.stream_of(grad.device)) == 0
    torch.cuda.synchronize()
    want = [a + b for a, b in zip(data[17][2], data[65][2])]
    check(ref, grad, want, f"{kernel} multi")
