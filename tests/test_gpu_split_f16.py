"""The fp16 two-term split of the f16x3 products (csrc/jet_x6.hpp splitq<4>: every fp16 plane, the
weights' and the streams', goes through it) against a numpy emulation, bit for bit:

    hi = float16(a)                 round to nearest even
    lo = float16(a - float32(hi))   the difference is exact in fp32, then round to nearest even

Inputs: one 128 x 128 layer of values a = 2^8 w covering +-0, values whose low term is fp16-subnormal
(with and without a rounding in the subnormal range), values just below fp16's largest 65504, exact
fp16 values (low term 0), tiny values (high term subnormal or zero) and ordinary weights.

Two routes to the same device function: the probe insr_split_f16 (caller-chosen values, no scale and
no guard -- the only route to a in [65280, 65504): the planes' range guard clamps |w| >= 255), and
the weight-plane refresh (insr_siren_wsplit through MLP.refresh_wsplit), read back in fragment order
as tests/test_gpu_wsplit.py does, with every |w| < 255.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W = 128


@pytest.fixture(scope="module")
def B():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import base
    base._native.load()
    return base


def emulate(a):
    """(hi, lo) fp16 bit patterns (uint16) of the fp32 array a."""
    a = np.asarray(a, dtype=np.float32)
    hi = a.astype(np.float16)
    lo = (a - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def layer_values(top):
    """128 x 128 fp32 values a (all finite in fp16, |a| < top <= 65504), every class of the docstring.
    a / 2^8 is exact for each (a power-of-two scale of a normal fp32 number)."""
    rng = np.random.default_rng(20)
    n = W * W
    parts = []
    parts.append(np.array([0.0, -0.0] * 64, dtype=np.float32))
    # low term fp16-subnormal (|lo| < 2^-14): high term in [2^-7, 2^-5), the fp32 tail goes below
    # 2^-24, so the low term also rounds; and 1 + k 2^-23 / 1 + 2^-20: subnormal low terms held exactly
    parts.append(rng.uniform(2.0 ** -7, 2.0 ** -5, 3000).astype(np.float32))
    parts.append((1.0 + np.arange(1, 513, dtype=np.float64) * 2.0 ** -23).astype(np.float32))
    parts.append(np.array([1.0 + 2.0 ** -20, -(1.0 + 2.0 ** -20), 2.0 ** -14 + 2.0 ** -30], dtype=np.float32))
    # just below the top of the range: the last fp32 values below it, and a spread over its last fp16 steps
    t = np.float32(top)
    last = [t]
    for _ in range(64):
        last.append(np.nextafter(last[-1], np.float32(0.0)))
    parts.append(np.array(last[1:], dtype=np.float32))
    parts.append((top - rng.uniform(0.0, 96.0, 1500)).astype(np.float32).clip(max=last[1]))
    # exact fp16 values: low term 0 (normal and subnormal fp16)
    h = rng.integers(0, 0x7BFF, 2500).astype(np.uint16).view(np.float16).astype(np.float32)
    parts.append(h[np.abs(h) < top])
    # ties of the high term's rounding (half an fp16 step above an fp16 value: round to even)
    k = rng.integers(1024, 2048, 500).astype(np.float64)
    parts.append(((k + 0.5) * 2.0 ** -6).astype(np.float32))
    # tiny: high term fp16-subnormal or zero, low term underflows
    parts.append((rng.uniform(-1.0, 1.0, 600) * 2.0 ** rng.integers(-40, -13, 600)).astype(np.float32))
    v = np.concatenate(parts)
    # ordinary weights: 2^8 x (SIREN hidden weights ~ U(-sqrt(6 / W) / 30, +)) and a wide log-uniform fill
    fill = n - v.size
    assert fill > 2000
    v = np.concatenate([v, (rng.uniform(-1, 1, 1000) * 256.0 * np.sqrt(6.0 / W) / 30.0).astype(np.float32),
                        (rng.uniform(-1.0, 1.0, fill - 1000) * 2.0 ** rng.integers(-12, 15, fill - 1000)).astype(np.float32)])
    v[1::2] *= np.float32(-1.0)  # both signs of every class
    v = v[rng.permutation(n)].astype(np.float32)
    assert v.size == n and np.all(np.abs(v) < top) and np.all(np.isfinite(v.astype(np.float16)))
    return v.reshape(W, W)


def test_probe_split_matches_emulation_bitwise(B):
    """insr_split_f16 on caller-chosen values up to just below 65504."""
    nat = B._native
    a = layer_values(65504.0)
    hi_w, lo_w = emulate(a.reshape(-1))
    x = torch.from_numpy(a.reshape(-1).copy()).cuda()
    hi = torch.empty(W * W // 2, dtype=torch.int32, device="cuda")
    lo = torch.empty_like(hi)
    nat.check(nat.lib().insr_split_f16(nat.ptr(x), nat.ptr(hi), nat.ptr(lo), W * W // 2, nat.stream_of(x.device)),
              "insr_split_f16")
    torch.cuda.synchronize()
    hi_g = hi.cpu().numpy().view(np.uint16)  # little endian: the pair's first value in the low half
    lo_g = lo.cpu().numpy().view(np.uint16)
    bad = np.nonzero((hi_g != hi_w) | (lo_g != lo_w))[0]
    assert bad.size == 0, [(float(a.reshape(-1)[i]), hex(hi_g[i]), hex(hi_w[i]), hex(lo_g[i]), hex(lo_w[i]))
                           for i in bad[:8]]


def test_weight_plane_refresh_matches_emulation_bitwise(B):
    """The fp16 weight planes of one 128 x 128 layer, both orientations, after refresh_wsplit."""
    nat = B._native
    a = layer_values(65280.0)  # 2^8 x 255: the planes' range guard
    torch.manual_seed(21)
    net = B.MLP(2, 1, 1, W, nonlinearity="sine").cuda()
    with torch.no_grad():
        net.net[2].weight.copy_(torch.from_numpy(a / np.float32(256.0)))
    assert np.array_equal(net.net[2].weight.detach().cpu().numpy() * np.float32(256.0), a)
    net.refresh_wsplit()
    torch.cuda.synchronize()
    assert nat.lib().insr_siren_wsplit_status(nat.ptr(net.flat_params()), 2, 1, 1, W,
                                              nat.stream_of(torch.device("cuda"))) == 0
    store = net.flat_params()._base
    L, NT, KC = 1, W // 16, W // 32
    # fragment (rt, kc), term q, lane (g, c), element jj  <-  row 16 rt + c, column 32 kc + 8 g + jj
    rt, kc, lane, jj = np.meshgrid(np.arange(NT), np.arange(KC), np.arange(64), np.arange(8), indexing="ij")
    rows, cols = 16 * rt + (lane & 15), 32 * kc + 8 * (lane >> 4) + jj
    for o in (0, 1):
        src = a if o == 0 else a.T
        hi_w, lo_w = emulate(src[rows, cols])
        h16 = store[net.wsplit_offset() + (3 + o) * L * W * W:][:L * W * W].view(torch.int16).cpu().numpy()
        got = h16.view(np.uint16).reshape(NT, KC, 2, 64, 8)
        assert np.array_equal(got[:, :, 0], hi_w), (o, "hi")
        assert np.array_equal(got[:, :, 1], lo_w), (o, "lo")
