"""The f16x3 value backward at width 128 (jet_x6.hpp jet_bwd_x6<4, 8, 1, false, T>): point-major h image,
dW tiled 2 row tiles x 4 column tiles per wave with B fragments read one column tile ahead, W^T streamed
one K chunk ahead of the propagation.

SIREN 4 x 128 value jets, 2 -> 2 and 2 -> 1, at the default precision (the fused tile-split path,
insr_jet_bwd_path == 0).  Shapes: the smallest that reach every branch of the body --

  * T in {1, 2, 4} forced with knobs(tiles=(0, T)) at n = 1, n = 16 T - 3 (one block, ragged last tile) and
    n = 16 (2 T + 1) + 5 (three blocks, the last one short of T tiles: slots without data);
  * T = 5 exists only as the balanced launch shape (INSR_JET_TILES codes 0, 1, 2, 4: the knob cannot force
    it), so it runs at the natural size: the smallest n for which insr_jet_split_tiles answers 5 on this
    device, + 7 points (blocks of 5 and of 4 tiles: the odd set count's half-dead K chunk and the
    skipped one).

Checked: the parameter gradients against the CPU oracle at the parity bound (1e-5 normwise per tensor,
tests/test_gpu_parity.py), two runs bit for bit, adjoints scaled by 2^-20 on some tiles and 2^12 on others
(the block exponent moves), a two-job launch against job by job (2e-6, tests/test_gpu_multi_bwd.py), and
in-kernel loss seeds against the same adjoints passed as gy (bit for bit).
"""
import ctypes

import pytest
import torch

from oracle import siren_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5        # parity bound, normwise per tensor
ORDER_TOL = 2e-6  # one launch vs job by job: the same products, partial rows summed in another order
L, W = 4, 128


@pytest.fixture(scope="module")
def B():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import base
    base._native.load()
    return base


@pytest.fixture(scope="module")
def nets(B):
    """(oracle, net) per output width, built once."""
    out = {}
    for dout in (2, 1):
        torch.manual_seed(20 + dout)
        ref = O.OracleSiren(2, dout, L, W)
        torch.manual_seed(20 + dout)
        out[dout] = (ref, B.MLP(2, dout, L, W, nonlinearity="sine").cuda())
    return out


@pytest.fixture(scope="module")
def n_bal(B, nets):
    """Smallest n whose value backward takes 5-tile balanced blocks, + 7 points (None: never 5)."""
    nat = B._native
    lib = nat.lib()
    mode = nets[2][1].call_mode(nat.MODE_VALUE)
    for tiles in range(1, 4096):
        if lib.insr_jet_split_tiles(16 * tiles, 2, W, mode, 1) == 5:
            assert lib.insr_jet_split_tiles(16 * tiles + 7, 2, W, mode, 1) == 5
            return 16 * tiles + 7
    return None


def nerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def pts(n, seed):
    return torch.rand(n, 2, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def hip_grads(B, net, x, gy, T):
    nat = B._native
    with nat.knobs(tiles=(0, T)):
        cm = net.call_mode(nat.MODE_VALUE)
        assert nat.lib().insr_jet_bwd_path(x.shape[0], 2, gy.shape[1], L, W, cm) == 0
        if T:
            assert nat.lib().insr_jet_split_tiles(x.shape[0], 2, W, cm, 1) == T
        net.zero_grad(set_to_none=True)
        (net(x.cuda()) * gy.cuda()).sum().backward()
    torch.cuda.synchronize()
    return [p.grad.detach().clone() for p in net.parameters()]


def check(B, nets, dout, n, T, gy=None, seed=0):
    ref, net = nets[dout]
    x = pts(n, 100 + seed)
    if gy is None:
        gy = torch.randn(n, dout, generator=torch.Generator().manual_seed(200 + seed))
    g1 = hip_grads(B, net, x, gy, T)
    g2 = hip_grads(B, net, x, gy, T)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    ref.zero_grad(set_to_none=True)
    (ref(x) * gy).sum().backward()
    for (k, p), g in zip(ref.named_parameters(), g1):
        e = nerr(g, p.grad)
        print(f"dout={dout} n={n} T={T} {k}: {e:.3e}")
        assert torch.isfinite(g).all(), k
        assert e < TOL, (k, e)


def tile_scales(n):
    """2^-20 on the points of every third 16-point tile, 2^12 on the next one's, 1 elsewhere."""
    t = torch.arange(n) // 16
    s = torch.ones(n)
    s[t % 3 == 0] = 2.0 ** -20
    s[t % 3 == 1] = 2.0 ** 12
    return s[:, None]


@pytest.mark.parametrize("dout", [2, 1])
@pytest.mark.parametrize("which", ["one_point", "one_block_ragged", "three_blocks_short_tail"])
@pytest.mark.parametrize("T", [1, 2, 4])
def test_forced_tiles_match_oracle_and_repeat(B, nets, T, which, dout):
    n = {"one_point": 1, "one_block_ragged": 16 * T - 3, "three_blocks_short_tail": 16 * (2 * T + 1) + 5}[which]
    check(B, nets, dout, n, T, seed=T)


@pytest.mark.parametrize("dout", [2, 1])
def test_balanced_five_tile_blocks_match_oracle_and_repeat(B, nets, n_bal, dout):
    if n_bal is None:
        pytest.skip("insr_jet_split_tiles never answers 5 on this device")
    check(B, nets, dout, n_bal, 0, seed=5)


@pytest.mark.parametrize("T", [4, 5])
def test_adjoint_scales_move_the_block_exponent(B, nets, n_bal, T):
    if T == 5 and n_bal is None:
        pytest.skip("insr_jet_split_tiles never answers 5 on this device")
    n = n_bal if T == 5 else 16 * (2 * T + 1) + 5
    gy = torch.randn(n, 2, generator=torch.Generator().manual_seed(31)) * tile_scales(n)
    check(B, nets, 2, n, 0 if T == 5 else T, gy=gy, seed=7)


def test_two_job_launch_equals_job_by_job(B, nets, n_bal):
    """Interior + band in one insr_siren_jet_bwd_grad_multi launch = the two insr_siren_jet_bwd_grad calls."""
    nat = B._native
    lib = nat.lib()
    _, net = nets[2]
    cm = net.call_mode(nat.MODE_VALUE)
    net.ensure_wsplit()
    flat = net.flat_params()
    st = nat.stream_of(torch.device("cuda"))
    jobs, keep = [], []
    for k, n in enumerate((n_bal or 8199, 162)):
        x = pts(n, 50 + k).cuda()
        act = torch.empty(lib.insr_jet_act_bytes(n, 2, L, W, cm) // 4, device="cuda")
        y = torch.empty(n, 2, device="cuda")
        assert lib.insr_siren_jet_fwd(nat.ptr(x), n, 2, 2, L, W, cm, nat.ptr(flat), nat.ptr(y), None, None,
                                      nat.ptr(act), st) == 0
        gy = torch.randn(n, 2, generator=torch.Generator().manual_seed(60 + k)).cuda()
        jobs.append(nat.BwdJob(x.data_ptr(), act.data_ptr(), gy.data_ptr(), None, None, n))
        keep += [x, act, gy]
    P = flat.numel()
    g_single = torch.zeros(P, device="cuda")
    for j in jobs:
        w = torch.empty(lib.insr_jet_bwd_work_bytes(j.n, 2, 2, L, W, cm) // 4, device="cuda")
        assert lib.insr_siren_jet_bwd_grad(j.x, j.n, 2, 2, L, W, cm, nat.ptr(flat), j.act, j.gy, None, None,
                                           nat.ptr(w), nat.ptr(g_single), 1, st) == 0
        keep.append(w)
    arr = (nat.BwdJob * len(jobs))(*jobs)
    ns = (ctypes.c_long * len(jobs))(*[j.n for j in jobs])
    w = torch.empty(lib.insr_jet_bwd_multi_work_bytes(ns, len(jobs), 2, 2, L, W, cm) // 4, device="cuda")
    g_multi = torch.full((P,), float("nan"), device="cuda")  # accumulate = 0 overwrites
    assert lib.insr_siren_jet_bwd_grad_multi(arr, len(jobs), 2, 2, L, W, cm, nat.ptr(flat), nat.ptr(w),
                                             nat.ptr(g_multi), 0, st) == 0
    torch.cuda.synchronize()
    n_params = lib.insr_siren_param_count(2, 2, L, W)
    e = nerr(g_multi[:n_params], g_single[:n_params])
    print(f"two-job launch vs job by job: {e:.3e}")
    assert e < ORDER_TOL


def _seeded_jet(B, lazy, n, nb, seed=5):
    """One value reverse jet of a merged [interior; bands] batch with the fluid phases' loss group on its
    outputs, unit-seeded: lazy = the kernel forms the adjoints from the loss terms, else the group is
    launched and its gradient arrives as gy.  Returns the flat .grad and whether the jet was seeded."""
    from base import _jet
    from base.losses import lazy_losses, register_unit_seed, settle_lazy
    torch.manual_seed(seed)
    net = B.MLP(2, 2, L, W, nonlinearity="sine").cuda()
    g = torch.Generator(device="cuda").manual_seed(seed)
    xa = (torch.rand(n + 2 * nb, 2, device="cuda", generator=g) * 2 - 1).requires_grad_(True)
    t1 = torch.rand(n, 2, device="cuda", generator=g)
    unit = register_unit_seed(torch.ones((), device="cuda"))
    with lazy_losses(lazy):
        y = net(xa)
        main, bc = B.sq_losses(B.mse_term(y, t1, count=2 * n), B.wall_term(y, nb, row0=n))
    s0 = _jet.SEED_STATS["seeded"]
    with _jet.defer_reductions():
        with _jet.batched_backward():
            torch.autograd.backward([main, bc], grad_tensors=[unit, unit])
        settle_lazy()
        grad = net.flat_grad_buffer().detach().cpu().clone()
    torch.cuda.synchronize()
    return grad, _jet.SEED_STATS["seeded"] - s0


def test_seeded_jet_equals_adjoints_as_gy(B, n_bal):
    n = (n_bal or 8199) - 2 * 20
    g_on, k_on = _seeded_jet(B, True, n, 20)
    g_off, k_off = _seeded_jet(B, False, n, 20)
    assert k_on == 1 and k_off == 0
    assert torch.equal(g_on, g_off)
