"""Second-order jets without a GPU: the torch restatement of the stream recurrences
(base/_hess.py torch_hess_jet, what the node differentiates itself with under create_graph=True and
the arithmetic csrc/jet_hess.hpp implements) against the oracle's autograd Hessians; the host queries
of the insr_siren_hess_* / insr_hess_* entry points; the per-network opt-in flag."""
import copy
import types

import pytest
import torch

from oracle import siren_oracle as O

SHAPES = [(2, 1, 2, 32), (2, 2, 3, 64), (3, 1, 2, 32), (3, 3, 4, 128)]


def nerr(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _pair(shape, seed=11):
    import base as B
    din, dout, L, W = shape
    torch.manual_seed(seed)
    ref = O.OracleSiren(din, dout, L, W)
    torch.manual_seed(seed)
    net = B.MLP(din, dout, L, W, nonlinearity="sine")  # the same init stream: the oracle's weights
    return ref, net


@pytest.mark.parametrize("shape", SHAPES)
def test_torch_restatement_matches_oracle(shape):
    """Values and every parameter gradient of sum(H . R), R random and NOT symmetric, at 1e-5 normwise
    (the project's contract; an exact-fp32 evaluation of the recurrences sits below 1e-6)."""
    from base import _hess
    din, dout, L, W = shape
    ref, net = _pair(shape)
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(33, din, generator=gen) * 2 - 1
    R = torch.randn(33, dout, din, din, generator=gen)
    xr = x.clone().requires_grad_(True)
    yr = ref(xr)
    Jr, _ = O.op_jacobian(yr, xr)
    Hr, _ = O.op_hessian(yr, xr)
    (Hr * R).sum().backward()
    y, J, H = _hess.torch_hess_jet(net, x)
    assert H.shape == (33, dout, din, din)
    assert nerr(y, yr) < 1e-5 and nerr(J, Jr) < 1e-5 and nerr(H, Hr) < 1e-5
    assert torch.equal(H, H.transpose(-1, -2))
    (H * R).sum().backward()
    for (name, p), q in zip(net.named_parameters(), ref.parameters()):
        if q.grad is None:  # the output bias: the Hessian does not depend on it
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert nerr(p.grad, q.grad) < 1e-5, name


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import base
    return base._native.load(ge.LIB)


def test_host_queries(lib):
    assert lib.insr_siren_hess_supported(3, 1, 4, 128) == 1
    assert lib.insr_siren_hess_supported(2, 3, 0, 32) == 1
    assert lib.insr_siren_hess_supported(4, 1, 4, 128) == 0   # d_in 2 / 3
    assert lib.insr_siren_hess_supported(1, 1, 4, 128) == 0   # d_in = 1 keeps the Laplacian stream
    assert lib.insr_siren_hess_supported(2, 1, 4, 100) == 0   # width not compiled
    assert lib.insr_siren_hess_supported(2, 4, 4, 128) == 0   # d_out <= 3
    # saved streams: (L + 1) layers x act_tiles(n) 16-point tiles x S streams x 16 W floats
    for n, din, L, W in [(64, 2, 4, 128), (65, 3, 4, 128), (1, 3, 2, 32), (300, 2, 0, 64)]:
        S = 1 + din + din * (din + 1) // 2
        tiles = ((n + 63) // 64) * 4
        assert lib.insr_hess_act_bytes(n, din, L, W) == (L + 1) * tiles * S * 16 * W * 4
    assert lib.insr_hess_act_bytes(64, 4, 4, 128) == -1
    assert lib.insr_hess_partial_blocks(0, 2, 128) == 0
    assert lib.insr_hess_partial_blocks(65, 3, 128) == 5      # one 16-point tile per block
    assert lib.insr_hess_partial_bytes(65, 2, 1, 4, 128) == 5 * lib.insr_jet_partial_stride(2, 1, 4, 128) * 4


def test_invalid_arguments_rejected_without_launch(lib):
    fwd = lambda n, din, dout, L, W: lib.insr_siren_hess_fwd(None, n, din, dout, L, W, None, None, None, None,  # noqa: E731
                                                             None, None)
    bwd = lambda n, din, dout, L, W: lib.insr_siren_hess_bwd(None, n, din, dout, L, W, None, None, None, None,  # noqa: E731
                                                             None, None, None)
    for call in (fwd, bwd):
        assert call(0, 2, 1, 4, 128) == 0        # n = 0: nothing to do, no launch
        assert call(10, 2, 1, 4, 128) == -1      # null required pointers
        assert call(10, 4, 1, 4, 128) == -1      # d_in
        assert call(10, 2, 0, 4, 128) == -1      # d_out
        assert call(-1, 2, 1, 4, 128) == -1
        assert call(2 ** 31 - 8, 2, 1, 4, 128) == -1   # 16 ceil(n / 16) would leave the int range
        assert call(10, 2, 1, 4, 100) == -2      # INSR_EWIDTH
        assert call(10, 3, 1, 4, 256) == -2      # not compiled: ten streams do not fit a CU's LDS


def test_flag_default_deepcopy_and_config():
    import base as B
    from base.networks import get_network
    net = B.MLP(3, 1, 2, 32, nonlinearity="sine")
    assert net.hessian_jet is False
    assert B.MLP(3, 1, 2, 32, nonlinearity="sine", hessian_jet=True).hessian_jet is True
    net.hessian_jet = True
    assert copy.deepcopy(net).hessian_jet is True
    cfg = types.SimpleNamespace(network="siren", num_hidden_layers=2, hidden_features=32, nonlinearity="sine")
    assert get_network(cfg, 2, 1).hessian_jet is False
    cfg.insr_hessian_jet = True
    assert get_network(cfg, 2, 1).hessian_jet is True
    from base import diff_ops
    assert isinstance(diff_ops.HESS_JETS, dict)
