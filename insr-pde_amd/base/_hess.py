"""Second-order jets: the value, the Jacobian and the full Hessian of a d_in = 2 / 3 SIREN from ONE
forward launch (insr_siren_hess_fwd, csrc/jet_hess.hpp), every parameter gradient from ONE reverse
launch (insr_siren_hess_bwd) -- what hessian() and laplace(normalize=True) of the reference
(base/diff_ops.py:6-41) get from d_out (1 + d_in) create_graph autograd passes.

Opt-in per network (MLP(..., hessian_jet=True) / net.hessian_jet = True / cfg.insr_hessian_jet); with
the flag off, or where insr_siren_hess_supported answers 0, base/diff_ops.py keeps its present routes.
The node sits beside _jet._SirenJet: its reverse jet writes the network's flat .grad through the same
partial-row hand-over (PendingSums "rows"), so grad_for_backward, grad_write_begin / end and
defer_reductions behave as for a fused-path reverse jet; it launches at once (it does not join a
batched_backward queue).  Under create_graph=True it differentiates itself with torch ops
(torch_hess_jet), as _SirenJet does.  Exact fp32 whatever the network's precision.  With MLP.coord_grad a
plain backward also returns the adjoint of x, through torch ops on torch_hess_jet (third order: no kernel).
"""
import ctypes

import torch

from . import _jet
from . import _native as nat

HESS_KEY = 3  # the jets' name in _jet.TIMING keys (not a library jet mode)
_jet.MODE_NAMES[HESS_KEY] = "hess"


def pairs(d):
    """The unordered pairs i <= j in the kernels' stream order (row-major upper triangle)."""
    return [(i, j) for i in range(d) for j in range(i, d)]


def torch_hess_jet(mlp, x2):
    """(y, dy, hess) of `mlp` at x2 (n, d_in) as plain, differentiable torch ops: dy (n, d_out, d_in),
    hess (n, d_out, d_in, d_in) -- the streams the HIP kernels carry (csrc/jet_hess.hpp: z = W h + b on
    every stream, bias on the value only; h = sin(w z), dh_i = w cos(w z) t_i, hh_ij = w cos(w z) u_ij -
    w^2 sin(w z) t_i t_j for the pairs i <= j).  Reference semantics for create_graph passes through the
    node: autograd differentiates this to any order, w.r.t. x2 and the parameters."""
    omega = 30.0
    ps = mlp.plist()
    L = mlp.num_hidden_layers
    d = x2.shape[1]
    pr = pairs(d)
    w0, b0 = ps[0], ps[1]
    z = torch.addmm(b0, x2, w0.t())
    t = [w0[:, i].unsqueeze(0) for i in range(d)]  # first layer: the tangents are W_0's columns
    u = None  # first layer: zero second-order streams
    for layer in range(1, L + 2):
        s = torch.sin(omega * z)
        c = omega * torch.cos(omega * z)
        w2s = (omega * omega) * s
        dh = [c * ti for ti in t]
        hh = [-w2s * (t[i] * t[j]) if u is None else c * u[k] - w2s * (t[i] * t[j]) for k, (i, j) in enumerate(pr)]
        wl, bl = ps[2 * layer], ps[2 * layer + 1]
        z = torch.addmm(bl, s, wl.t())
        t = [dhi @ wl.t() for dhi in dh]
        u = [h @ wl.t() for h in hh]
    dy = torch.stack(t, dim=-1)
    k = {p: n for n, p in enumerate(pr)}
    hess = torch.stack([torch.stack([u[k[(min(i, j), max(i, j))]] for j in range(d)], dim=-1) for i in range(d)],
                       dim=-2)
    return z, dy, hess


def enabled(mlp):
    """The network opted in and a kernel serves its shape."""
    if not getattr(mlp, "hessian_jet", False) or mlp.in_features not in (2, 3):
        return False
    return bool(nat.lib().insr_siren_hess_supported(mlp.in_features, mlp.out_features, mlp.num_hidden_layers,
                                                    mlp.kernel_width))


class _SirenHess(torch.autograd.Function):
    """Forward second-order jet (one kernel) + its reverse (one kernel + the partial-row sums)."""

    @staticmethod
    def forward(ctx, x2, mlp, save, *params):
        lib = nat.lib()
        n, din = x2.shape
        L, W, dout = mlp.num_hidden_layers, mlp.kernel_width, mlp.out_features
        flat = mlp.flat_params()
        dev = x2.device
        y = torch.empty(n, dout, device=dev, dtype=torch.float32)
        dy = torch.empty(n, dout, din, device=dev, dtype=torch.float32)
        hess = torch.empty(n, dout, din, din, device=dev, dtype=torch.float32)
        act = None
        if save:
            act = torch.empty(max(lib.insr_hess_act_bytes(n, din, L, W) // 4, 1), device=dev, dtype=torch.float32)
        with _jet._timed("fwd", HESS_KEY, n, W, (din, dout, L)):
            rc = lib.insr_siren_hess_fwd(nat.ptr(x2), n, din, dout, L, W, nat.ptr(flat), nat.ptr(y), nat.ptr(dy),
                                         nat.ptr(hess), nat.ptr(act), nat.stream_of(dev))
        nat.check(rc, "insr_siren_hess_fwd")
        ctx.set_materialize_grads(False)  # unused outputs -> None -> NULL adjoint (no zero-fill launch)
        ctx.mlp, ctx.save, ctx.x2, ctx.act = mlp, save, x2, act
        return y, dy, hess

    @staticmethod
    def backward(ctx, gy, gdy, gh):
        mlp = ctx.mlp
        none = (None,) * (3 + len(mlp.plist()))
        if torch.is_grad_enabled():  # create_graph=True: reference semantics, to any order
            return _reference_backward(ctx, (gy, gdy, gh))
        if gy is None and gdy is None and gh is None:
            return none
        res = none
        if getattr(mlp, "coord_grad", False) and ctx.needs_input_grad[0]:
            # the adjoint of x, on request (MLP.coord_grad): a third-order quantity, through torch ops (no
            # kernel is compiled for it)
            from . import losses
            losses.materialize_for(gy, gdy, gh)
            key = ("hess", ctx.x2.shape[1], mlp.out_features, mlp.num_hidden_layers, mlp.kernel_width)
            gx = _jet._torch_x_adjoint(mlp, lambda xd: torch_hess_jet(mlp, xd), ctx.x2, (gy, gdy, gh), key)
            res = (gx,) + none[1:]
        if not ctx.save or not any(p.requires_grad for p in mlp.plist()):
            return res
        c = lambda t: None if t is None else (t if t.is_contiguous() else t.contiguous())  # noqa: E731
        _launch_bwd(mlp, ctx.x2, ctx.act, c(gy), c(gdy), c(gh))
        return res


def _reference_backward(ctx, grads):
    """_SirenHess.backward under create_graph=True: the input / parameter gradients of
    sum(g_y y + g_dy dy + g_h hess) as a differentiable graph of torch ops (_jet._reference_backward's
    scheme on torch_hess_jet)."""
    mlp, x2 = ctx.mlp, ctx.x2
    from . import losses
    losses.materialize_for(*grads)
    params = mlp.plist()
    none = (None,) * (3 + len(params))
    want_x = ctx.needs_input_grad[0]
    pidx = [i for i in range(len(params)) if ctx.needs_input_grad[3 + i]]
    if not want_x and not pidx:
        return none
    outs = torch_hess_jet(mlp, x2)
    prs = [(o, g) for o, g in zip(outs, grads) if g is not None]
    if not prs:
        return none
    ins = ([x2] if want_x else []) + [params[i] for i in pidx]
    gs = torch.autograd.grad([o for o, _ in prs], ins, grad_outputs=[g for _, g in prs], create_graph=True,
                             allow_unused=True)
    res = [None] * len(none)
    k = 0
    if want_x:
        res[0], k = gs[0], 1
    for i in pidx:
        res[3 + i] = gs[k]
        k += 1
    _jet.REF_STATS["backward"] += 1
    return tuple(res)


def _launch_bwd(mlp, x2, act, gy, gdy, gh):
    """One reverse second-order jet: its partial-gradient rows now, their sums into the network's flat
    .grad now or (inside defer_reductions) with the Adam launch."""
    from . import losses
    n, din = x2.shape
    L, W, dout = mlp.num_hidden_layers, mlp.kernel_width, mlp.out_features
    lib = nat.lib()
    cur = torch.cuda.current_stream(x2.device)
    for t in (gy, gdy, gh):  # lazy loss groups among the adjoints: read as data here
        g = losses.lazy_group_of(t)
        if g is not None:
            g.materialize(cur)
    gflat, accumulate = mlp.grad_for_backward()
    st = ctypes.c_void_p(cur.cuda_stream)
    mlp.grad_write_begin(cur)  # order after a write of .grad made on another stream
    defer = getattr(_jet._Defer, "depth", 0) > 0
    with torch.cuda.stream(cur):
        part = torch.empty(max(lib.insr_hess_partial_bytes(n, din, dout, L, W) // 4, 1), device=x2.device,
                           dtype=torch.float32)
    with _jet._timed("bwd", HESS_KEY, n, W, (din, dout, L)):
        rc = lib.insr_siren_hess_bwd(nat.ptr(x2), n, din, dout, L, W, nat.ptr(mlp.flat_params()), nat.ptr(act),
                                     nat.ptr(gy), nat.ptr(gdy), nat.ptr(gh), nat.ptr(part), st)
    nat.check(rc, "insr_siren_hess_bwd")
    nb, stride = lib.insr_hess_partial_blocks(n, din, W), lib.insr_jet_partial_stride(din, dout, L, W)
    pr = _jet.PendingSums("rows", part, nb, stride, mlp, gflat, accumulate, cur, (HESS_KEY, n, W, (din, dout, L)))
    _jet._hand_over(mlp, pr, cur, defer and 0 < nb < 1024)  # (the Adam launch sums fewer than 1,024 rows)


def run_hess_jet(mlp, x):
    """(y, dy, hess) of `mlp` at x with x's leading dims: dy (..., d_out, d_in), hess (..., d_out, d_in, d_in)."""
    mlp.ensure_packed()
    din, dout = mlp.in_features, mlp.out_features
    if not enabled(mlp):
        raise _jet.UnsupportedPattern(f"no second-order jet for SIREN(in={din}, out={dout}, "
                                      f"width={mlp.kernel_width}) (or hessian_jet is off)")
    if _jet._Fused.pending is not None:
        raise _jet.UnsupportedPattern("a second-order jet inside a fused_forwards scope (it launches at once)")
    x2, lead = _jet._flatten_x(x, din)
    y, dy, hess = _SirenHess.apply(x2, mlp, _jet._needs_save(mlp, x2), *mlp.plist())
    if x.dim() == 2:
        return y, dy, hess
    return y.view(*lead, dout), dy.view(*lead, dout, din), hess.view(*lead, dout, din, din)


def hess_jet_of(mlp, holder, x):
    """The second-order jet of a network call, cached on its value tensor / node under a key of its own
    (jet_of's GRAD / LAP cache and the jet-mode hints are not touched)."""
    res = getattr(holder, "_insr_hess", None)
    if res is None:
        res = run_hess_jet(mlp, x)
        holder._insr_hess = res
    return res
