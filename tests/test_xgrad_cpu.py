"""Coordinate gradients without a GPU: the per-network opt-in flag (MLP.coord_grad), the host side of
insr_siren_jet_bwd_x / insr_siren_jet_bwd_x_supported (include/insr_siren.h), and the torch route the
jet nodes take for the adjoint of x where no kernel serves a call (base/_jet.py _torch_x_adjoint),
against fp64 autograd of the oracle through the reference's own operators."""
import copy
import types

import pytest
import torch

from oracle import siren_oracle as O

TOL = 1e-5
MODES = {"value": 0, "grad": 1, "lap": 2}


def test_flag_default_deepcopy_and_config():
    import base as B
    from base.networks import get_network
    net = B.MLP(3, 1, 2, 32, nonlinearity="sine")
    assert net.coord_grad is False
    assert B.MLP(3, 1, 2, 32, nonlinearity="sine", coord_grad=True).coord_grad is True
    net.coord_grad = True
    assert copy.deepcopy(net).coord_grad is True
    cfg = types.SimpleNamespace(network="siren", num_hidden_layers=2, hidden_features=32, nonlinearity="sine")
    assert get_network(cfg, 2, 1).coord_grad is False
    cfg.insr_coord_grad = True
    assert get_network(cfg, 2, 1).coord_grad is True
    assert get_network(cfg, 2, 1).hessian_jet is False
    # a configuration the jets do not serve is the reference's plain torch network: it takes the flag and
    # needs none (autograd returns the adjoint of x)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (TorchMLP says once per configuration that it is off the hot path)
        t = B.MLP(2, 1, 2, 32, nonlinearity="relu", coord_grad=True)
    assert type(t).__name__ == "TorchMLP"


def test_saving_rule():
    """The forward saves its streams when a parameter requires grad, or -- flag on -- when x does."""
    import base as B
    from base import _jet
    net = B.MLP(2, 1, 2, 32, nonlinearity="sine")
    x = torch.zeros(4, 2)
    xg = torch.zeros(4, 2, requires_grad=True)
    assert _jet._needs_save(net, x) and _jet._needs_save(net)
    for p in net.parameters():
        p.requires_grad_(False)
    assert not _jet._needs_save(net, xg)
    net.coord_grad = True
    assert _jet._needs_save(net, xg) and not _jet._needs_save(net, x) and not _jet._needs_save(net)
    with torch.no_grad():
        assert not _jet._needs_save(net, xg)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import base
    return base._native.load(ge.LIB)


def test_supported_set(lib):
    from base import _native as nat
    sup = lib.insr_siren_jet_bwd_x_supported
    for W in (32, 64, 128, 256):
        for din in (1, 2, 3):
            for dout in (1, 2, 3):
                for mode in (0, 1, 2):
                    for L in (0, 1, 4):
                        assert sup(din, dout, L, W, mode) == 1, (din, dout, L, W, mode)
    assert sup(4, 1, 4, 128, 0) == 0     # d_in <= 3
    assert sup(2, 4, 4, 128, 1) == 0     # d_out <= 3
    assert sup(2, 1, 4, 100, 2) == 0     # width not compiled
    assert sup(2, 1, 4, 128, 3) == 0     # not a jet mode
    # precision bits do not matter to it ...
    for prec in nat.PRECISIONS.values():
        assert sup(2, 1, 4, 128, 2 | nat.jet_prec(prec)) == 1
    # ... a call whose backward is the recompute kernel saves no streams to read (insr_jet_bwd_path == 3)
    k = nat.jet_policy(4)
    assert lib.insr_jet_bwd_path(16708, 2, 1, 4, 128, 2 | k) == 3
    assert sup(2, 1, 4, 128, 2 | k) == 0
    assert sup(2, 1, 3, 128, 2 | k) == 1  # (that kernel serves 4 hidden layers only: the call saves as usual)


def test_invalid_arguments_rejected_without_launch(lib):
    one = 1  # a non-NULL "pointer" that is never dereferenced: every refusal below precedes the launch
    call = lambda n, din, dout, L, W, mode, p=None, a=None, g=None: lib.insr_siren_jet_bwd_x(  # noqa: E731
        n, din, dout, L, W, mode, p, a, None, None, None, g, None)
    assert call(0, 2, 1, 4, 128, 2) == 0                 # n = 0: nothing to do, no launch
    assert call(0, 2, 1, 4, 128, 2, one, one, one) == 0
    assert call(10, 2, 1, 4, 128, 2) == -1               # NULL params / act / gx
    assert call(10, 2, 1, 4, 128, 2, one, one, None) == -1
    assert call(10, 2, 1, 4, 128, 2, one, None, one) == -1
    assert call(10, 2, 1, 4, 128, 2, None, one, one) == -1
    assert call(10, 4, 1, 4, 128, 0, one, one, one) == -1     # d_in
    assert call(10, 2, 0, 4, 128, 0, one, one, one) == -1     # d_out
    assert call(10, 2, 4, 4, 128, 0, one, one, one) == -1
    assert call(10, 2, 1, -1, 128, 0, one, one, one) == -1    # depth
    assert call(10, 2, 1, 4, 128, 3, one, one, one) == -1     # not a jet mode
    assert call(-1, 2, 1, 4, 128, 0, one, one, one) == -1
    assert call(2 ** 31 - 8, 2, 1, 4, 128, 0, one, one, one) == -1   # 16 ceil(n / 16) would leave the int range
    assert call(10, 2, 1, 4, 100, 0, one, one, one) == -2     # INSR_EWIDTH
    assert call(10, 2, 1, 4, 512, 1, one, one, one) == -2


def _judge(ref64, x, adj, mode):
    """x.grad of sum(Ry y + RJ J + RL lap) for the fp64 network, through the reference's operators."""
    Ry, RJ, RL = (a.double() for a in adj)
    dout = Ry.shape[1]
    xr = x.double().clone().requires_grad_(True)
    y = ref64(xr)
    loss = (y * Ry).sum()
    if mode != "value":
        loss = loss + (O.op_jacobian(y, xr)[0] * RJ).sum()
    if mode == "lap":
        lap = torch.cat([O.op_laplace(y[:, o:o + 1], xr) for o in range(dout)], dim=-1)
        loss = loss + (lap * RL).sum()
    loss.backward()
    return xr.grad.detach()


@pytest.mark.parametrize("mode", ["value", "grad", "lap"])
def test_torch_route_matches_oracle(mode):
    """_torch_x_adjoint on torch_jet (CPU tensors): max |x-adjoint - fp64 judge| <= 1e-5 max |judge|; it
    counts itself in REF_STATS["x_backward"], warns once per shape, and leaves no parameter gradient."""
    import warnings
    import base as B
    from base import _jet
    din, dout, L, W = 2, 1, 2, 32
    n = 17
    torch.manual_seed(11)
    ref = O.OracleSiren(din, dout, L, W)
    torch.manual_seed(11)
    net = B.MLP(din, dout, L, W, nonlinearity="sine")  # the same init stream: the oracle's weights
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(n, din, generator=gen) * 2 - 1
    adj = (torch.rand(n, dout, generator=gen) + 0.5, torch.randn(n, dout, din, generator=gen),
           torch.randn(n, dout, generator=gen))
    want = _judge(copy.deepcopy(ref).double(), x, adj, mode)
    grads = (adj[0], adj[1] if mode != "value" else None, adj[2] if mode == "lap" else None)
    key = (mode, din, dout, L, W, "cpu-test")
    before = _jet.REF_STATS["x_backward"]
    with pytest.warns(UserWarning, match="coordinate gradient"):
        gx = _jet._torch_x_adjoint(net, lambda xd: _jet.torch_jet(net, xd, MODES[mode]), x, grads, key)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the second call of a shape is silent
        gx2 = _jet._torch_x_adjoint(net, lambda xd: _jet.torch_jet(net, xd, MODES[mode]), x, grads, key)
    assert _jet.REF_STATS["x_backward"] == before + 2
    assert gx.shape == (n, din) and not gx.requires_grad and torch.equal(gx, gx2)
    assert all(p.grad is None for p in net.parameters())
    err = float((gx.double() - want).abs().max() / want.abs().max())
    print(f"  {mode}: {err:.2e}")
    assert err <= TOL, err
