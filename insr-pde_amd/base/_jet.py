"""Autograd bridge between the `base` API and the HIP jet kernels.

`siren_value(mlp, x)` is MLP.forward.  Its output carries provenance
(`_insr_src = (mlp, x)`), so that

    gradient(y, x) / divergence(y, x) / jacobian(y, x) / laplace(y, x)

on that output run ONE forward Taylor jet (value + d tangents [+ Laplacian
stream]) in HIP instead of the reference's create_graph autograd passes
(base/diff_ops.py:33-82), and `loss.backward()` runs the matching HIP reverse
jet straight into the network's flat gradient buffer.

Recognised shapes of `y` (everything the reference models use):
  * y = mlp(x)                          (advection, fluid)
  * y = mlp(x) + x   /  x + mlp(x)      (elasticity/model.py:137, q = f(x) + x)
  * y = gradient(mlp(x), x)  inside divergence  (-> Laplacian stream)
Anything else is not fused: match() returns None and base/diff_ops.py takes the reference's
own route -- torch.autograd.grad(..., create_graph=True) -- through the graph.  A jet node
reached by such a create_graph pass differentiates itself with torch ops on the device
(torch_jet / _reference_backward: the reference semantics to any order, slower); the
library stays mandatory (the forwards are HIP; no CPU path exists).
"""
import ctypes
import os
import threading

import torch

from . import _native as nat

MODE_NAMES = {nat.MODE_VALUE: "value", nat.MODE_GRAD: "grad", nat.MODE_LAP: "lap"}


class UnsupportedPattern(RuntimeError):
    pass


def _flatten_x(x, din):
    if x.shape[-1] != din:
        raise ValueError(f"expected last dim {din}, got {tuple(x.shape)}")
    lead = x.shape[:-1]
    x2 = x.reshape(-1, din)
    if x2.dtype != torch.float32:
        raise TypeError("the HIP path computes in fp32; got " + str(x2.dtype))
    if not x2.is_cuda:
        raise nat.NativeUnavailable("insr-pde_amd runs on the GPU only (got a CPU tensor); "
                                    "move the network and samples to cuda")
    return x2.contiguous(), lead


def _needs_save(mlp, x2=None):
    """Does the forward of this call save its streams: a parameter requires grad, or the network returns
    coordinate gradients (MLP.coord_grad) and the call's points x2 require grad -- a frozen network saves
    too then (the x-adjoint launch reads the streams, _x_adjoint)."""
    if not torch.is_grad_enabled():
        return False
    if any(p.requires_grad for p in mlp.plist()):
        return True
    return bool(getattr(mlp, "coord_grad", False)) and x2 is not None and x2.requires_grad


# Optional per-launch HIP-event timing (bench.py's roofline leg).  When enabled,
# every jet launch is bracketed by torch.cuda.Event records on the launch stream.
TIMING = {"on": False, "events": []}


class _timed:
    def __init__(self, kind, mode, n, W, shape=None):
        # (kind, mode, points, width, (d_in, d_out, hidden layers))
        self.key = (kind, MODE_NAMES[mode], n, W, shape)

    def __enter__(self):
        if TIMING["on"]:
            # the device is kept busy past the host's submission of the timed launches (a spin kernel of
            # ~100 us queued first), so the events bracket device time only -- without it a short launch
            # (the one-launch advection iteration: ~25 us of work behind ~30 us of Python per call) is
            # timed as the host's submission gap
            torch.cuda._sleep(TIMING.get("spin", 250000))
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if TIMING["on"]:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            TIMING["events"].append((self.key, self.e0, e1))
        return False


class _SirenJet(torch.autograd.Function):
    """Forward jet (one kernel) + reverse jet (one kernel + partial reduction)."""

    @staticmethod
    def forward(ctx, x2, mode, mlp, save, *params):
        lib = nat.lib()
        n, din = x2.shape
        L, W, dout = mlp.num_hidden_layers, mlp.kernel_width, mlp.out_features
        cmode = mlp.call_mode(mode)  # + the network's precision bits and INSR_MODE_WSPLIT
        mlp.ensure_wsplit()          # the pre-split weight planes follow the parameters
        flat = mlp.flat_params()
        dev = x2.device
        y = torch.empty(n, dout, device=dev, dtype=torch.float32)
        dy = torch.empty(n, dout, din, device=dev, dtype=torch.float32) if mode != nat.MODE_VALUE else None
        lap = torch.empty(n, dout, device=dev, dtype=torch.float32) if mode == nat.MODE_LAP else None
        act = None
        # the recompute backward (path 3) reruns the forward per tile: nothing to save
        if save and lib.insr_jet_bwd_path(n, din, dout, L, W, cmode) != 3:
            nbytes = lib.insr_jet_act_bytes(n, din, L, W, cmode)
            act = torch.empty(max(nbytes // 4, 1), device=dev, dtype=torch.float32)
        if _Fused.pending is not None:  # launched with the other jets of the scope, at its exit
            _Fused.pending.append(((din, L, W, cmode, dev), (x2, flat, y, dy, lap, act, n, dout)))
        else:
            with _timed("fwd", mode, n, W, (din, dout, L)):
                rc = lib.insr_siren_jet_fwd(nat.ptr(x2), n, din, dout, L, W, cmode, nat.ptr(flat), nat.ptr(y),
                                            nat.ptr(dy), nat.ptr(lap), nat.ptr(act), nat.stream_of(dev))
            nat.check(rc, "insr_siren_jet_fwd")
        ctx.set_materialize_grads(False)  # unused outputs -> None -> NULL adjoint (no zero-fill launch)
        ctx.mode, ctx.cmode, ctx.mlp, ctx.save = mode, cmode, mlp, save  # the backward reuses the forward's mode
        ctx.x2, ctx.act = x2, act
        # the outputs' buffers (address, elements): a lazy loss group's terms read them (losses.LazyGroup)
        ctx.out_bufs = tuple((0, 0) if t is None else (t.data_ptr(), t.numel()) for t in (y, dy, lap))
        outs = [y]
        if dy is not None:
            outs.append(dy)
        if lap is not None:
            outs.append(lap)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        mlp, mode = ctx.mlp, ctx.mode
        none = (None,) * (4 + len(mlp.plist()))
        if torch.is_grad_enabled():
            # create_graph=True: the caller differentiates THROUGH this jet (a diff op on a graph the
            # jet matcher does not recognise, base/diff_ops.py fallback): reference semantics
            return _reference_backward(ctx, grads)
        gy = grads[0]
        gdy = grads[1] if mode != nat.MODE_VALUE else None
        glap = grads[2] if mode == nat.MODE_LAP else None
        if gy is None and gdy is None and glap is None:
            return none
        c = lambda t: None if t is None else (t if t.is_contiguous() else t.contiguous())  # noqa: E731
        gy, gdy, glap = c(gy), c(gdy), c(glap)
        res = none
        if getattr(mlp, "coord_grad", False) and ctx.needs_input_grad[0]:
            # the adjoint of x, on request (MLP.coord_grad): its own launch, now, on autograd's stream --
            # whether or not a parameter requires grad, and independent of the parameter job below
            res = (_x_adjoint(mlp, mode, ctx.cmode, ctx.x2, ctx.act, gy, gdy, glap),) + none[1:]
        if not ctx.save or not any(p.requires_grad for p in mlp.plist()):
            return res
        job = _BwdJob(mlp, mode, ctx.cmode, ctx.x2, ctx.act, gy, gdy, glap)
        job.outs = ctx.out_bufs
        queue = _BwdBatch.queue_for(job)
        if queue is not None:  # launched with the network's other jobs at the scope's exit
            queue.append(job)
        else:
            _launch_bwd(job)
        return res


def torch_jet(mlp, x2, mode):
    """The jet of `mlp` at x2 (n, d_in) as plain, differentiable torch ops on x2's device: (y, dy, lap)
    with dy (n, d_out, d_in) for GRAD / LAP and lap (n, d_out) for LAP, the streams the HIP kernels
    carry (z = W h + b on every stream, bias on the value only; h = sin(w z),
    dh_i = w cos(w z) t_i, ddh = w cos(w z) q - w^2 sin(w z) sum_i t_i^2).  Reference semantics for
    graphs the jet matcher does not recognise: autograd differentiates this to any order, w.r.t. x2
    and the parameters (what base/diff_ops.py:6-82 get from torch.autograd.grad(create_graph=True)
    through the reference's nn.Sequential, base/networks.py:67-71)."""
    omega = 30.0
    ps = mlp.plist()
    L = mlp.num_hidden_layers
    ntan = x2.shape[1] if mode != nat.MODE_VALUE else 0
    lapm = mode == nat.MODE_LAP
    w0, b0 = ps[0], ps[1]
    z = torch.addmm(b0, x2, w0.t())
    t = [w0[:, i].unsqueeze(0) for i in range(ntan)]  # first layer: the tangents are W_0's columns
    q = None  # first layer: zero Laplacian stream
    for layer in range(1, L + 2):
        s = torch.sin(omega * z)
        if ntan:
            c = omega * torch.cos(omega * z)
            dh = [c * ti for ti in t]
            if lapm:
                t2 = sum(ti * ti for ti in t)
                ddh = -(omega * omega) * s * t2 if q is None else c * q - (omega * omega) * s * t2
        wl, bl = ps[2 * layer], ps[2 * layer + 1]
        z = torch.addmm(bl, s, wl.t())
        if ntan:
            t = [dhi @ wl.t() for dhi in dh]
            if lapm:
                q = ddh @ wl.t()
    dy = torch.stack(t, dim=-1) if ntan else None
    return z, dy, (q if lapm else None)


def _reference_backward(ctx, grads):
    """_SirenJet.backward under create_graph=True: the input / parameter gradients of
    sum(g_y y + g_dy dy + g_lap lap), as a differentiable graph of torch ops (torch_jet on the
    forward's own x2, so derivatives of the result reach x through x2's graph)."""
    mlp, mode, x2 = ctx.mlp, ctx.mode, ctx.x2
    from . import losses
    losses.materialize_for(*grads)  # lazy loss groups: their gradients are read as data here
    params = mlp.plist()
    none = (None,) * (4 + len(params))
    want_x = ctx.needs_input_grad[0]
    pidx = [i for i in range(len(params)) if ctx.needs_input_grad[4 + i]]
    if not want_x and not pidx:
        return none
    outs = torch_jet(mlp, x2, mode)
    pairs = [(o, g) for o, g in zip(outs, grads) if o is not None and g is not None]
    if not pairs:
        return none
    ins = ([x2] if want_x else []) + [params[i] for i in pidx]
    # the adjoints enter as grad_outputs: the vector of the VJP, not differentiated in this call
    # (they may depend on x themselves, e.g. 2 y of d(y^2)/dx); the result stays differentiable in them
    gs = torch.autograd.grad([o for o, _ in pairs], ins, grad_outputs=[g for _, g in pairs], create_graph=True,
                             allow_unused=True)
    res = [None] * len(none)
    k = 0
    if want_x:
        res[0], k = gs[0], 1
    for i in pidx:
        res[4 + i] = gs[k]
        k += 1
    REF_STATS["backward"] += 1
    return tuple(res)


# reference-semantics backwards run through the jet nodes: create_graph passes ("backward"), and x-adjoints
# of a plain backward that no kernel served ("x_backward": _torch_x_adjoint)
REF_STATS = {"backward": 0, "x_backward": 0}


def _x_adjoint(mlp, mode, cmode, x2, act, gy, gdy, glap):
    """The adjoint of the coordinates x2 of one jet call for the (contiguous) adjoints gy / gdy / glap of
    its outputs: ONE launch of insr_siren_jet_bwd_x on the forward's saved streams, at once, on autograd's
    current stream (it joins no batched_backward queue and holds back no sums).  Where no kernel serves the
    call (insr_siren_jet_bwd_x_supported) or the forward saved nothing (the recompute policy): torch ops
    with the reference's semantics (_torch_x_adjoint)."""
    from . import losses
    n, din = x2.shape
    L, W, dout = mlp.num_hidden_layers, mlp.kernel_width, mlp.out_features
    lib = nat.lib()
    cur = torch.cuda.current_stream(x2.device)
    for t in (gy, gdy, glap):  # lazy loss groups among the adjoints: read as data here
        g = losses.lazy_group_of(t)
        if g is not None:
            g.materialize(cur)
    if act is None or not lib.insr_siren_jet_bwd_x_supported(din, dout, L, W, cmode):
        return _torch_x_adjoint(mlp, lambda xd: torch_jet(mlp, xd, mode), x2, (gy, gdy, glap),
                                (MODE_NAMES[mode], din, dout, L, W))
    gx = torch.empty(n, din, device=x2.device, dtype=torch.float32)
    with _timed("bwdx", mode, n, W, (din, dout, L)):
        rc = lib.insr_siren_jet_bwd_x(n, din, dout, L, W, cmode, nat.ptr(mlp.flat_params()), nat.ptr(act),
                                      nat.ptr(gy), nat.ptr(gdy), nat.ptr(glap), nat.ptr(gx),
                                      ctypes.c_void_p(cur.cuda_stream))
    nat.check(rc, "insr_siren_jet_bwd_x")
    return gx


_X_WARNED = set()


def _torch_x_adjoint(mlp, jet, x2, grads, key):
    """The x-adjoint of a jet call through torch ops: jet(xd) -- torch_jet / torch_hess_jet of the network --
    on a detached copy of x2 that requires grad, then autograd.grad with the adjoints as grad_outputs.  x
    only (the parameters keep their own route), first order (not differentiable further).  Off the hot
    path: counted in REF_STATS["x_backward"], one warning per shape."""
    if key not in _X_WARNED:
        _X_WARNED.add(key)
        import warnings
        warnings.warn(f"coordinate gradient of a {key[0]} jet of SIREN(in={key[1]}, out={key[2]}, hidden layers="
                      f"{key[3]}, width={key[4]}): no kernel serves this call (or its forward saved no streams); "
                      "running torch ops", stacklevel=2)
    with torch.enable_grad():
        xd = x2.detach().requires_grad_(True)
        outs = jet(xd)
        prs = [(o, g) for o, g in zip(outs, grads) if o is not None and g is not None]
        (gx,) = torch.autograd.grad([o for o, _ in prs], [xd], grad_outputs=[g.detach() for _, g in prs])
    REF_STATS["x_backward"] += 1
    return gx


class _BwdJob:
    """One reverse jet: the network, its jet mode and its forward's full call mode (precision and
    knob bits: the backward runs with the knobs its forward ran with, whatever scope is open
    when autograd reaches it), the forward's points / saved streams, the adjoints, and the
    stream autograd ran its backward on."""
    __slots__ = ("mlp", "mode", "cmode", "x2", "act", "gy", "gdy", "glap", "cur", "outs")

    def __init__(self, mlp, mode, cmode, x2, act, gy, gdy, glap):
        self.mlp, self.mode, self.cmode, self.x2, self.act = mlp, mode, cmode, x2, act
        self.gy, self.gdy, self.glap = gy, gdy, glap
        self.cur = torch.cuda.current_stream(x2.device)
        self.outs = ((0, 0), (0, 0), (0, 0))  # the forward's (y, dy, lap) buffers (_SirenJet.backward sets them)


DEFER_REDUCE = True  # BaseModel._update_network opens defer_reductions (False: A/B studies, tests)
_Defer = threading.local()  # .depth > 0 inside defer_reductions on this thread, .nets its networks


class defer_reductions:
    """`with defer_reductions(): backward; optimizer.step()` -- a fused-path reverse jet (one
    partial-gradient row per block) launched inside the scope does not launch its row sums: they are
    held on the network (MLP.set_pending_reduce) for base.FusedAdam.step, which sums them into .grad
    and runs the Adam (+ plateau) update in the same launch (insr_adam_step_partials).  Any other
    access to the flat gradient lands them first (MLP.flush_pending_reduce), and the scope's exit
    lands whatever no step consumed.  BaseModel._update_network opens it around backward + step when
    the optimiser is FusedAdam."""

    def __enter__(self):
        _Defer.depth = getattr(_Defer, "depth", 0) + 1
        if _Defer.depth == 1:
            _Defer.nets = []
        return self

    def __exit__(self, exc_type, *exc):
        _Defer.depth -= 1
        if _Defer.depth == 0:
            nets, _Defer.nets = _Defer.nets, None
            for mlp in nets:
                if exc_type is None:
                    mlp.flush_pending_reduce()
                else:  # an aborted iteration (e.g. a failed capture): nothing more is launched for it
                    mlp.take_pending_reduce()
        return False


class PendingSums:
    """The held-back sums of one reverse jet: kind "rows" -- a fused-path backward's partial-gradient
    rows (insr_reduce_partials_strided / insr_adam_step_partials); kind "split" -- the second half of a
    jet_fb.hpp or two-kernel backward (insr_siren_jet_bwd_grad_adam phase 2)."""
    __slots__ = ("kind", "buf", "nb", "stride", "job", "gflat", "accumulate", "cur", "key", "fin")

    def __init__(self, kind, buf, nb, stride, job, gflat, accumulate, cur, key, fin=None):
        self.kind, self.buf, self.nb, self.stride, self.job = kind, buf, nb, stride, job
        self.gflat, self.accumulate, self.cur, self.key = gflat, accumulate, cur, key
        self.fin = fin  # (InsrLossFin, its loss_part tensor): a seeded backward's loss values, finished here

    def launch(self, adam=None):
        """The sums into .grad; adam = (params, m, v, state, b1, b2, eps, loss or None, patience): with
        the Adam (+ plateau) update of every element in the same launch.  A seeded backward's loss values
        are finished by the same launch (before its plateau step reads them)."""
        lib = nat.lib()
        st = ctypes.c_void_p(self.cur.cuda_stream)
        p, m, v, state, b1, b2, eps, loss, patience = adam if adam is not None else (None,) * 7 + (None, 0)
        fin = None if self.fin is None else ctypes.addressof(self.fin[0])
        if self.kind == "rows":
            if adam is None:
                with _timed("reduce", *self.key):
                    if fin is None:
                        rc = lib.insr_reduce_partials_strided(nat.ptr(self.buf), self.nb, self.gflat.numel(),
                                                              self.stride, nat.ptr(self.gflat), self.accumulate, st)
                    else:
                        rc = lib.insr_reduce_partials_fin(nat.ptr(self.buf), self.nb, self.gflat.numel(), self.stride,
                                                          nat.ptr(self.gflat), self.accumulate, fin, st)
                nat.check(rc, "insr_reduce_partials_strided")
                return
            mlp = self.job
            shape = (ctypes.c_int * 4)(mlp.in_features, mlp.out_features, mlp.num_hidden_layers, mlp.kernel_width)
            args = (nat.ptr(self.buf), self.nb, self.stride, nat.ptr(self.gflat), self.accumulate, nat.ptr(p),
                    nat.ptr(m), nat.ptr(v), self.gflat.numel(), shape, nat.ptr(state), b1, b2, eps, nat.ptr(loss),
                    patience)
            if fin is None:
                nat.check(lib.insr_adam_step_partials(*args, st), "insr_adam_step_partials")
            else:
                nat.check(lib.insr_adam_step_partials_fin(*args, fin, st), "insr_adam_step_partials_fin")
            return
        mlp, x2, n, cmode = self.job
        din, dout, L, W = mlp.in_features, mlp.out_features, mlp.num_hidden_layers, mlp.kernel_width
        with _timed("reduce", *self.key):
            if fin is None:
                rc = lib.insr_siren_jet_bwd_grad_adam(
                    nat.ptr(x2), n, din, dout, L, W, cmode, nat.ptr(mlp.flat_params()), None, None, None, None,
                    nat.ptr(self.buf), nat.ptr(self.gflat), self.accumulate, 2, nat.ptr(m), nat.ptr(v),
                    nat.ptr(state), b1 or 0.0, b2 or 0.0, eps or 0.0, nat.ptr(loss), patience, st)
            else:
                rc = lib.insr_siren_jet_bwd_grad_adam_fin(
                    nat.ptr(x2), n, din, dout, L, W, cmode, nat.ptr(mlp.flat_params()), nat.ptr(self.buf),
                    nat.ptr(self.gflat), self.accumulate, nat.ptr(m), nat.ptr(v), nat.ptr(state), b1 or 0.0,
                    b2 or 0.0, eps or 0.0, nat.ptr(loss), patience, fin, st)
        nat.check(rc, "insr_siren_jet_bwd_grad_adam")


def launch_reduce(pr):
    """The held-back sums of one reverse jet (MLP.flush_pending_reduce)."""
    pr.launch()


def _seed_plan(job, lib):
    """(LazyGroup, InsrSeed terms, loss_part rows) when this reverse jet evaluates a lazy loss group's
    terms itself (losses.LazyGroup: one group, all of its losses seeding this job's streams, a backward
    path that takes seeds); otherwise the lazy groups among its adjoints are launched now (before the
    reverse jet reads them) and None."""
    from . import losses
    streams = {nat.SEED_VALUE: job.gy, nat.SEED_GRAD: job.gdy, nat.SEED_LAP: job.glap}
    groups = {}
    for t in streams.values():
        g = losses.lazy_group_of(t)
        if g is not None:
            groups[id(g)] = g
    if not groups:
        return None
    if len(groups) == 1:
        g = next(iter(groups.values()))
        n, din = job.x2.shape
        mlp = job.mlp
        rows = lib.insr_jet_bwd_seed_rows(n, din, mlp.out_features, mlp.num_hidden_layers, mlp.kernel_width,
                                          job.cmode)
        if rows > 0:
            terms = g.seeds_for({sid: (t, *job.outs[sid]) for sid, t in streams.items()})
            if terms:
                return g, terms, rows
    for g in groups.values():
        g.materialize(job.cur)
    return None


def _seeded_launch(job, plan, work, st):
    """The seeded first launch of a reverse jet (insr_siren_jet_bwd_seeded): its seeded adjoint streams
    pass NULL; returns the (InsrLossFin, loss_part, terms) its sums launch finishes the losses with."""
    g, terms, rows = plan
    mlp, x2 = job.mlp, job.x2
    n, din = x2.shape
    seeded = {t.stream for t in terms}
    ptr = lambda sid, t: None if sid in seeded else nat.ptr(t)  # noqa: E731
    with torch.cuda.stream(job.cur):
        lpart = torch.empty(rows * nat.SEED_MAX, device=x2.device, dtype=torch.float32)
    arr = (nat.Seed * len(terms))(*terms)
    with _timed("bwd", job.mode, n, mlp.kernel_width, (din, mlp.out_features, mlp.num_hidden_layers)):
        rc = nat.lib().insr_siren_jet_bwd_seeded(
            nat.ptr(x2), n, din, mlp.out_features, mlp.num_hidden_layers, mlp.kernel_width, job.cmode,
            nat.ptr(mlp.flat_params()), nat.ptr(job.act), ptr(nat.SEED_VALUE, job.gy), ptr(nat.SEED_GRAD, job.gdy),
            ptr(nat.SEED_LAP, job.glap), arr, len(terms), nat.ptr(lpart), nat.ptr(work), st)
    nat.check(rc, "insr_siren_jet_bwd_seeded")
    g.state = "seeded"
    g._forget()
    SEED_STATS["seeded"] += 1
    SEED_STATS[job.mode] = SEED_STATS.get(job.mode, 0) + 1
    return (g.fin(lpart, rows), lpart, arr)


SEED_STATS = {"seeded": 0}  # reverse jets that evaluated a lazy loss group's terms, in all and per jet mode


def _splits_phases(lib, path, n, din, dout, L, W, cmode):
    """Does this backward run as a sweep + separate sums (insr_siren_jet_bwd_grad_adam phases 1 / 2): a
    jet_fb.hpp kernel, or the two-kernel path of a net with hidden layers (capi.hip splits_phases)."""
    return lib.insr_jet_bwd_kernel(n, din, dout, L, W, cmode) == 1 or (path == 1 and L > 0)


def _hand_over(mlp, pr, cur, defer, launch=True):
    """A reverse jet's held-back sums: to the Adam launch (defer: inside defer_reductions), else launched
    now (launch); the write of .grad ends here either way."""
    if defer:
        mlp.set_pending_reduce(pr)
        _Defer.nets.append(mlp)
    elif launch:
        pr.launch()
    mlp.grad_write_end(cur)


def _launch_bwd(job):
    """One reverse jet into its network's flat .grad (first write of an iteration overwrites)."""
    mlp, mode, x2, act, gy, gdy, glap = job.mlp, job.mode, job.x2, job.act, job.gy, job.gdy, job.glap
    n, din = x2.shape
    L, W, dout = mlp.num_hidden_layers, mlp.kernel_width, mlp.out_features
    cmode = job.cmode
    mlp.ensure_wsplit()
    lib = nat.lib()
    plan = _seed_plan(job, lib)  # a lazy loss group's terms evaluated in this jet (None: pointers)
    gflat, accumulate = mlp.grad_for_backward()
    cur = job.cur
    st = ctypes.c_void_p(cur.cuda_stream)
    mlp.grad_write_begin(cur)  # order after a write of .grad made on another stream
    defer = getattr(_Defer, "depth", 0) > 0  # inside defer_reductions: the sums go into the Adam launch
    path = lib.insr_jet_bwd_path(n, din, dout, L, W, cmode)
    if path > 0:
        # two-kernel path (propagation + split-K dW GEMM), the resident-dW or the recompute persistent
        # kernel, with their fixed-order sums straight into .grad.  Scratch comes from the pool of the
        # stream the kernels run on (a deferred job's autograd stream may differ from the current one)
        with torch.cuda.stream(cur):
            work = torch.empty(max(lib.insr_jet_bwd_work_bytes(n, din, dout, L, W, cmode) // 4, 1),
                               device=x2.device, dtype=torch.float32)
        splits = _splits_phases(lib, path, n, din, dout, L, W, cmode)
        if plan is not None or (defer and splits):
            # the jet_fb.hpp or the two-kernel backward: its sweep now, its sums with the Adam launch
            # (defer_reductions) -- or, seeded outside that scope, right after it
            if plan is not None:
                fin = _seeded_launch(job, plan, work, st)
            else:
                fin = None
                with _timed("bwd", mode, n, W, (din, dout, L)):
                    rc = lib.insr_siren_jet_bwd_grad_adam(
                        nat.ptr(x2), n, din, dout, L, W, cmode, nat.ptr(mlp.flat_params()), nat.ptr(act), nat.ptr(gy),
                        nat.ptr(gdy), nat.ptr(glap), nat.ptr(work), nat.ptr(gflat), accumulate, 1, None, None, None,
                        0.0, 0.0, 0.0, None, 0, st)
                nat.check(rc, "insr_siren_jet_bwd_grad_adam")
            pr = PendingSums("split", work, 0, 0, (mlp, x2, n, cmode), gflat, accumulate, cur,
                             (mode, n, W, (din, dout, L)), fin)
            _hand_over(mlp, pr, cur, defer)
            return
        with _timed("bwd", mode, n, W, (din, dout, L)):
            rc = lib.insr_siren_jet_bwd_grad(nat.ptr(x2), n, din, dout, L, W, cmode, nat.ptr(mlp.flat_params()),
                                             nat.ptr(act), nat.ptr(gy), nat.ptr(gdy), nat.ptr(glap), nat.ptr(work),
                                             nat.ptr(gflat), accumulate, st)
        nat.check(rc, "insr_siren_jet_bwd_grad")
        mlp.grad_write_end(cur)
        return
    with torch.cuda.stream(cur):
        part = torch.empty(max(lib.insr_jet_partial_bytes(n, din, dout, L, W, cmode) // 4, 1), device=x2.device,
                           dtype=torch.float32)
    if plan is not None:
        fin = _seeded_launch(job, plan, part, st)
    else:
        fin = None
        with _timed("bwd", mode, n, W, (din, dout, L)):
            rc = lib.insr_siren_jet_bwd(nat.ptr(x2), n, din, dout, L, W, cmode, nat.ptr(mlp.flat_params()),
                                        nat.ptr(act), nat.ptr(gy), nat.ptr(gdy), nat.ptr(glap), nat.ptr(part), st)
        nat.check(rc, "insr_siren_jet_bwd")
    nb, stride = lib.insr_jet_partial_blocks(n, din, W, cmode), lib.insr_jet_partial_stride(din, dout, L, W)
    pr = PendingSums("rows", part, nb, stride, mlp, gflat, accumulate, cur, (mode, n, W, (din, dout, L)), fin)
    _hand_over(mlp, pr, cur, defer and 0 < nb < 1024)  # (the Adam launch sums fewer than 1,024 rows)


def _launch_bwd_multi(jobs):
    """Reverse jets of ONE network, jet mode and stream (e.g. a phase's interior batch and its
    wall bands from separate network calls, fluid/model.py:80,96-97) in one call of
    insr_siren_jet_bwd_grad_multi: the jobs the fused tile-split kernel serves share one launch
    and one fixed-order partial-row reduction."""
    mlp, mode, cur = jobs[0].mlp, jobs[0].mode, jobs[0].cur
    from . import losses
    for j in jobs:  # lazy loss groups among the adjoints: launched first (this path reads them as data)
        for t in (j.gy, j.gdy, j.glap):
            g = losses.lazy_group_of(t)
            if g is not None:
                g.materialize(cur)
    din = jobs[0].x2.shape[1]
    L, W, dout = mlp.num_hidden_layers, mlp.kernel_width, mlp.out_features
    cmode = jobs[0].cmode
    mlp.ensure_wsplit()
    lib = nat.lib()
    gflat, accumulate = mlp.grad_for_backward()
    st = ctypes.c_void_p(cur.cuda_stream)
    mlp.grad_write_begin(cur)
    defer = getattr(_Defer, "depth", 0) > 0
    if len(jobs) <= nat.MAX_BWD_JOBS and all(j.act is not None for j in jobs):
        arr = (nat.BwdJob * len(jobs))(*[
            nat.BwdJob(j.x2.data_ptr(), nat.ptr(j.act), nat.ptr(j.gy), nat.ptr(j.gdy), nat.ptr(j.glap), j.x2.shape[0])
            for j in jobs])
        # the saved-stream resident sweep serves the jobs' total (a Laplacian interior + its bands), or the
        # two-kernel backward does (round 6: the elasticity interior + its constraint calls): ONE launch (one
        # propagation + one dW launch) for all of them, the sums (phase 2) with the Adam launch --
        # insr_siren_jet_bwd_multi_sweep
        tiles = sum((j.x2.shape[0] + 15) // 16 for j in jobs)
        n_pass = 16 * tiles
        path_pass = lib.insr_jet_bwd_path(n_pass, din, dout, L, W, cmode)
        # (path 3, the recompute kernel, has no multi sweep: its jobs carry no saved streams)
        if _splits_phases(lib, path_pass, n_pass, din, dout, L, W, cmode) and path_pass != 3:
            with torch.cuda.stream(cur):
                work = torch.empty(max(lib.insr_jet_bwd_work_bytes(n_pass, din, dout, L, W, cmode) // 4, 1),
                                   device=jobs[0].x2.device, dtype=torch.float32)
            with _timed("bwd%d" % len(jobs), mode, n_pass, W, (din, dout, L)):
                rc = lib.insr_siren_jet_bwd_multi_sweep(arr, len(jobs), din, dout, L, W, cmode,
                                                        nat.ptr(mlp.flat_params()), nat.ptr(work), st)
            if rc == 0:
                pr = PendingSums("split", work, 0, 0, (mlp, jobs[0].x2, n_pass, cmode), gflat, accumulate, cur,
                                 (mode, n_pass, W, (din, dout, L)))
                _hand_over(mlp, pr, cur, defer)  # (deferred or not, the gradient is the same bits)
                return
            if rc != -1:  # (INSR_EINVAL: not this path after all -- the calls below)
                nat.check(rc, "insr_siren_jet_bwd_multi_sweep")
        # every job on the fused tile-split path: their partial rows now, the sums with the Adam launch
        # (defer_reductions), as a single job's -- insr_siren_jet_bwd_multi_rows
        ns = (ctypes.c_long * len(jobs))(*[j.x2.shape[0] for j in jobs])
        wb = lib.insr_jet_bwd_multi_work_bytes(ns, len(jobs), din, dout, L, W, cmode)
        if wb >= 0:
            with torch.cuda.stream(cur):
                work = torch.empty(max(wb // 4, 1), device=jobs[0].x2.device, dtype=torch.float32)
            with _timed("bwd%d" % len(jobs), mode, sum(ns), W, (din, dout, L)):
                nb = lib.insr_siren_jet_bwd_multi_rows(arr, len(jobs), din, dout, L, W, cmode,
                                                       nat.ptr(mlp.flat_params()), nat.ptr(work), st)
            if nb >= 0:
                stride = lib.insr_jet_partial_stride(din, dout, L, W)
                pr = PendingSums("rows", work, nb, stride, mlp, gflat, accumulate, cur,
                                 (mode, int(sum(ns)), W, (din, dout, L)))
                _hand_over(mlp, pr, cur, defer and 0 < nb < 1024, launch=nb > 0)
                return
            # (INSR_EINVAL: a job takes another path -- the full call below)
    for k in range(0, len(jobs), nat.MAX_BWD_JOBS):
        chunk = jobs[k:k + nat.MAX_BWD_JOBS]
        arr = (nat.BwdJob * len(chunk))(*[
            nat.BwdJob(j.x2.data_ptr(), nat.ptr(j.act), nat.ptr(j.gy), nat.ptr(j.gdy), nat.ptr(j.glap), j.x2.shape[0])
            for j in chunk])
        ns = (ctypes.c_long * len(chunk))(*[j.x2.shape[0] for j in chunk])
        wb = lib.insr_jet_bwd_multi_work_bytes(ns, len(chunk), din, dout, L, W, cmode)
        nat.check(wb if wb < 0 else 0, "insr_jet_bwd_multi_work_bytes")
        with torch.cuda.stream(cur):  # scratch from the pool of the stream the kernels run on
            work = torch.empty(max(wb // 4, 1), device=jobs[0].x2.device, dtype=torch.float32)
        with _timed("bwd%d" % len(chunk), mode, sum(ns), W, (din, dout, L)):
            rc = lib.insr_siren_jet_bwd_grad_multi(arr, len(chunk), din, dout, L, W, cmode,
                                                   nat.ptr(mlp.flat_params()), nat.ptr(work), nat.ptr(gflat),
                                                   accumulate, st)
        nat.check(rc, "insr_siren_jet_bwd_grad_multi")
        accumulate = 1
    mlp.grad_write_end(cur)


class _BwdBatch:
    """Open batched_backward scopes, keyed by the CUDA stream they were opened on: autograd runs a
    CUDA backward on its device worker thread (not the thread that called backward), so a
    thread-local list would miss the jobs; keyed by stream, a scope collects exactly the reverse
    jets of its own stream (the re-entrancy model is one training thread per stream) and never
    launches another thread's jobs."""
    pending = {}  # stream handle -> list of _BwdJob while a scope is open on that stream
    lock = threading.Lock()

    @staticmethod
    def key(dev=None):
        return torch.cuda.current_stream(dev).cuda_stream if torch.cuda.is_available() else 0

    @classmethod
    def queue_for(cls, job):
        with cls.lock:
            return cls.pending.get(job.cur.cuda_stream)


class batched_backward:
    """`with batched_backward(): torch.autograd.backward(...)` -- the HIP reverse jets autograd
    asks for inside the scope are launched at its exit, grouped per (network, jet mode, stream)
    in first-request order: a group of one job launches as usual, a larger group through
    insr_siren_jet_bwd_grad_multi (one launch + one reduction for all of its fused-path jobs).
    Valid because the reverse jets return no gradient to autograd (they write the networks'
    flat .grad directly, and x gets none), so nothing inside the backward pass reads their
    results; .grad holds them when the scope exits.  BaseModel._backward opens it around the
    loss backward of every iteration.  The scope collects the jobs of the stream it was opened on."""

    def __enter__(self):
        self.k = _BwdBatch.key()
        with _BwdBatch.lock:
            self.outer = self.k not in _BwdBatch.pending
            if self.outer:
                _BwdBatch.pending[self.k] = []
        return self

    def __exit__(self, exc_type, *exc):
        if not self.outer:
            return False
        with _BwdBatch.lock:
            jobs = _BwdBatch.pending.pop(self.k)
        if exc_type is None:
            _flush_backward(jobs)
        return False


class immediate_backward:
    """Suspends the batched_backward scope of the current stream: a backward run inside (a custom
    autograd node that reads .grad right after its own nested backward, diff_ops._AugLaplacian)
    launches at once."""

    def __enter__(self):
        self.k = _BwdBatch.key()
        with _BwdBatch.lock:
            self.saved = _BwdBatch.pending.pop(self.k, None)
        return self

    def __exit__(self, *exc):
        if self.saved is not None:
            with _BwdBatch.lock:
                _BwdBatch.pending[self.k] = self.saved
        return False


def _flush_backward(jobs):
    groups = {}
    for j in jobs:
        if hasattr(j, "run"):  # a finished gradient's sums to register (base/advect_iter.py): on this thread
            j.run()
            continue
        groups.setdefault((id(j.mlp), j.cmode, j.cur.cuda_stream), []).append(j)
    for js in groups.values():
        if len(js) == 1:
            _launch_bwd(js[0])
        else:
            _launch_bwd_multi(js)


class _FusedState(threading.local):
    pending = None  # per thread: list of (arch key, job) while a fused_forwards scope is open


_Fused = _FusedState()  # (forward jets run on the calling thread: thread-local)


class fused_forwards:
    """`with fused_forwards(): a = f(x); b = g(x)` -- the forward jets issued inside the
    scope are launched together at its exit: jets of one architecture and mode go into ONE
    insr_siren_jet_fwd_multi launch (horizontal fusion, up to MAX_FWD_JOBS per launch; the
    networks' output widths may differ),
    e.g. the frozen previous velocity field and the trainable one at the same collocation
    points (fluid/model.py:97-98, :143-147).  Outputs, autograd nodes and saved streams are
    those of separate calls, bit for bit.  The outputs hold no values until the scope
    exits: read them only after it (the scope accepts network calls, nothing that consumes
    their results).  Nested scopes join the outermost one."""

    def __enter__(self):
        self.outer = _Fused.pending is None
        if self.outer:
            _Fused.pending = []
        return self

    def __exit__(self, exc_type, *exc):
        if not self.outer:
            return False
        jobs, _Fused.pending = _Fused.pending, None
        if exc_type is None:
            _launch_fused(jobs)
        return False


_MIXED = os.environ.get("INSR_FUSE_MIXED", "1") != "0"


MIX_ADVECT = 3  # include/insr_siren.h INSR_MIX_ADVECT: a job mode of insr_siren_jet_fwd_mixed


def _job_array(chunk):
    return (nat.JetJob * len(chunk))(*[
        nat.JetJob(x2.data_ptr(), flat.data_ptr(), y.data_ptr(), None if dy is None else dy.data_ptr(),
                   None if lap is None else lap.data_ptr(), None if act is None else act.data_ptr(), nj, dj)
        for x2, flat, y, dy, lap, act, nj, dj, *_ in chunk])


def _launch_mixed(din, L, W, pbits, dev, alljobs):
    """One insr_siren_jet_fwd_mixed launch: alljobs = [(jet mode, job tuple)]."""
    chunk = [j for _, j in alljobs]
    modes = (ctypes.c_int * len(chunk))(*[m for m, _ in alljobs])
    sc = (ctypes.c_float * (3 * len(chunk)))(*[v for _, j in alljobs for v in (j[8] if len(j) > 8 else (0., 0., 0.))])
    n = sum(j[6] for j in chunk)
    key_dout = tuple(j[7] for j in chunk)
    with _timed("fwdmix%d" % len(chunk), max(m for m, _ in alljobs if m != MIX_ADVECT) if any(
            m != MIX_ADVECT for m, _ in alljobs) else 0, n, W, (din, key_dout, L)):
        rc = nat.lib().insr_siren_jet_fwd_mixed(_job_array(chunk), modes, sc, len(chunk), din, chunk[0][7], L, W,
                                                pbits, nat.stream_of(dev))
    nat.check(rc, "insr_siren_jet_fwd_mixed")


def advect_target(mlp, x, dt, lo=-1.0, hi=1.0, up=None):
    """(f(clamp(x - dt f(x), lo, hi)), f(x)) of a frozen field f (fluid/model.py:96-97, the
    semi-Lagrangian target of the advection) as ONE job of a mixed launch -- inside a
    fused_forwards scope together with the phase's other jets.  No autograd (a target).
    up: the (n, d) buffer f(x) is written to (default: a new one)."""
    mlp.ensure_packed()
    mlp.ensure_wsplit()
    n, din = x.shape
    if mlp.out_features != din or x.dtype != torch.float32 or not x.is_cuda:
        raise UnsupportedPattern("advect_target: a d -> d fp32 GPU field")
    x2 = x.detach() if x.is_contiguous() else x.detach().contiguous()
    dev = x2.device
    y = torch.empty(n, din, device=dev, dtype=torch.float32)
    if up is None:
        up = torch.empty(n, din, device=dev, dtype=torch.float32)
    elif up.shape != (n, din) or not up.is_contiguous():
        raise UnsupportedPattern("advect_target: up must be a contiguous (n, d) buffer")
    foot = torch.empty(n, din, device=dev, dtype=torch.float32)
    cmode = (mlp.call_mode(nat.MODE_VALUE) & ~nat.MODE_MASK) | MIX_ADVECT
    job = (x2, mlp.flat_params(), y, up, foot, None, n, din, (float(dt), float(lo), float(hi)))
    key = (din, mlp.num_hidden_layers, mlp.kernel_width, cmode, dev)
    if _Fused.pending is not None:
        _Fused.pending.append((key, job))
    else:
        _launch_mixed(din, mlp.num_hidden_layers, mlp.kernel_width, cmode & ~nat.MODE_MASK, dev, [(MIX_ADVECT, job)])
    return y, up


def _launch_fused(jobs):
    groups = {}
    for key, job in jobs:
        groups.setdefault(key, []).append(job)
    lib = nat.lib()
    # jets that differ only in their jet mode (W = 128, batches in the 2-tile value regime):
    # ONE insr_siren_jet_fwd_mixed launch, each job with its own body
    by_arch = {}
    for (din, L, W, cmode, dev), js in groups.items():
        by_arch.setdefault((din, L, W, cmode & ~nat.MODE_MASK, dev), []).append((cmode & nat.MODE_MASK, js))
    for (din, L, W, pbits, dev), parts in by_arch.items():
        alljobs = [(m, j) for m, js in parts for j in js]
        adv = any(m == MIX_ADVECT for m, _ in alljobs)
        # (the mixed kernel's Laplacian body is compiled for d_in <= 2)
        lap3 = din > 2 and any(m == nat.MODE_LAP for m, _ in alljobs)
        if adv or (_MIXED and not lap3 and len(parts) > 1 and W == 128 and len(alljobs) <= nat.MAX_FWD_JOBS
                   and all(j[6] <= 40000 for _, j in alljobs)):
            if adv and not (_MIXED and len(alljobs) <= nat.MAX_FWD_JOBS):  # targets alone, the rest as usual
                tg = [(m, j) for m, j in alljobs if m == MIX_ADVECT]
                for m, j in tg:
                    _launch_mixed(din, L, W, pbits, dev, [(m, j)])
                groups.pop((din, L, W, pbits | MIX_ADVECT, dev))
                continue
            _launch_mixed(din, L, W, pbits, dev, alljobs)
            for m, js in parts:
                groups.pop((din, L, W, pbits | m, dev))
    for (din, L, W, cmode, dev), js in groups.items():  # output widths may differ per job
        mode = cmode & nat.MODE_MASK
        for k in range(0, len(js), nat.MAX_FWD_JOBS):
            chunk = js[k:k + nat.MAX_FWD_JOBS]
            n = sum(j[6] for j in chunk)
            douts = sorted({j[7] for j in chunk})
            dout = chunk[0][7]
            key_dout = douts[0] if len(douts) == 1 else tuple(j[7] for j in chunk)  # per-job widths in the timing key
            arr = _job_array(chunk)
            with _timed("fwd%d" % len(chunk) if len(chunk) > 1 else "fwd", mode, n, W, (din, key_dout, L)):
                rc = lib.insr_siren_jet_fwd_multi(arr, len(chunk), din, dout, L, W, cmode, nat.stream_of(dev))
            nat.check(rc, "insr_siren_jet_fwd_multi")


def run_jet(mlp, x, mode):
    """Run the fused jet of `mlp` at `x`.  Returns (y, dy, lap) with leading dims of x;
    dy is (..., d_out, d_in), lap (..., d_out); missing streams are None."""
    mlp.ensure_packed()
    din = mlp.in_features
    lib = nat.lib()
    if not lib.insr_siren_supported(din, mlp.out_features, mlp.num_hidden_layers, mlp.kernel_width,
                                    mlp.call_mode(mode)):
        raise UnsupportedPattern(
            f"no HIP kernel for SIREN(in={din}, out={mlp.out_features}, width={mlp.kernel_width}) "
            f"in {MODE_NAMES[mode]} mode")
    x2, lead = _flatten_x(x, din)
    params = tuple(mlp.plist())
    outs = _SirenJet.apply(x2, mode, mlp, _needs_save(mlp, x2), *params)
    if x.dim() == 2:  # no view node: keeps y.grad_fn == our node (identity-stable, see match())
        y = outs[0]
        dy = outs[1] if mode != nat.MODE_VALUE else None
        lap = outs[2] if mode == nat.MODE_LAP else None
        return y, dy, lap
    y = outs[0].view(*lead, mlp.out_features)
    dy = outs[1].view(*lead, mlp.out_features, din) if mode != nat.MODE_VALUE else None
    lap = outs[2].view(*lead, mlp.out_features) if mode == nat.MODE_LAP else None
    return y, dy, lap


# --------------------------------------------------------------------------
# jet-mode hints: inside a training loop the phase body makes the same calls every
# iteration, so when the value of call #k of a network was later differentiated
# (gradient / divergence / jacobian / laplace), iteration i+1 runs that call's
# forward directly as the derivative jet: the value is the jet's value stream
# (bit-identical to the value-only kernel), the diff op is served from the cache,
# and one reverse jet handles every adjoint -- no wasted value-only forward and
# backward.  A wrong hint costs time, never correctness: the cache is keyed by the
# exact value tensor / node, and a miss computes the requested jet as usual.
# --------------------------------------------------------------------------
class _HintScope:
    hints = None     # {(id(mlp), ordinal): mode} of the active loop, or None
    counts = None    # {id(mlp): calls so far in this iteration}


class call_scope:
    """`with call_scope(owner):` around one iteration of a phase body; hints live on
    `owner` (the PhaseLoop), so they persist across its iterations only."""

    def __init__(self, owner):
        if not hasattr(owner, "_insr_jet_hints"):
            owner._insr_jet_hints = {}
        self.hints = owner._insr_jet_hints

    def __enter__(self):
        self.saved = (_HintScope.hints, _HintScope.counts)
        _HintScope.hints, _HintScope.counts = self.hints, {}
        return self

    def __exit__(self, *exc):
        _HintScope.hints, _HintScope.counts = self.saved
        return False


def _supported(mlp, mode):
    return bool(nat.lib().insr_siren_supported(mlp.in_features, mlp.out_features, mlp.num_hidden_layers,
                                               mlp.kernel_width, mlp.call_mode(mode)))


def _promoted(mlp, mode):
    """The jet mode of a network call inside the loop's deferred scope (base/lower.py deferred_jets): a
    call whose network already has a jet of a HIGHER mode queued (gradient over value, Laplacian over
    gradient) runs in that mode too -- the advection body's band call after its interior gradient jets
    (advection/model.py:86-87), the pressure bands' gradient calls after the interior Laplacian jet
    (fluid/model.py:111,119-120).  Its outputs are the same bits (lower streams of a higher jet), and
    the calls share one forward launch and one reverse launch."""
    jobs = _Fused.pending
    if not jobs or mode == nat.MODE_LAP:
        return mode
    from . import lower
    if not lower.deferring():
        return mode
    flat = mlp.flat_params()
    top = max(((k[3] & nat.MODE_MASK) for k, j in jobs if len(j) == 8 and j[1] is flat
               and (k[3] & nat.MODE_MASK) in (nat.MODE_GRAD, nat.MODE_LAP)), default=mode)
    if top > mode and _supported(mlp, top) and not (top == nat.MODE_LAP and mlp.in_features > 2):
        return top
    return mode


def siren_value(mlp, x):
    """MLP.forward.  Provenance lives on the tensor AND on its autograd node, because
    in `q = mlp(x) + x` the value tensor itself is a dropped temporary; only the node
    survives inside q's graph."""
    key, mode = None, nat.MODE_VALUE
    if _HintScope.hints is not None:
        ordinal = _HintScope.counts.get(id(mlp), 0)
        _HintScope.counts[id(mlp)] = ordinal + 1
        key = (id(mlp), ordinal)
        mode = _HintScope.hints.get(key, nat.MODE_VALUE)
        if mode != nat.MODE_VALUE and not (x.requires_grad and _supported(mlp, mode)):
            mode = nat.MODE_VALUE
    mode = _promoted(mlp, mode)
    res = run_jet(mlp, x, mode)
    y = res[0]
    jets = {} if mode == nat.MODE_VALUE else {mode: res}
    y._insr_src, y._insr_jets, y._insr_key = (mlp, x), jets, key
    node = y.grad_fn
    if node is not None and type(node).__name__ != "ViewBackward0":
        # (batched x (..., d): y is a view of the jet's 2-D output -- a C++ node that takes no
        # attributes; the tensor's own provenance serves diff ops on y itself)
        node._insr_src, node._insr_jets, node._insr_key = (mlp, x), jets, key
    return y


# --------------------------------------------------------------------------
# provenance matching
# --------------------------------------------------------------------------
def _grad_edge_node(t):
    if t.grad_fn is not None:
        return t.grad_fn
    if t.requires_grad:
        return torch.autograd.graph.get_gradient_edge(t).node
    return None


def match(y, x):
    """Return (mlp, holder, affine) if y is a recognised function of x, else None.

    holder carries the jet cache (the value tensor or its autograd node);
    affine=True means y = mlp(x) + x (the identity is added to the Jacobian).
    """
    src = getattr(y, "_insr_src", None)
    if src is not None:
        return (src[0], y, False) if src[1] is x else None
    fn = y.grad_fn
    if fn is None or type(fn).__name__ != "AddBackward0" or getattr(fn, "_saved_alpha", 1) != 1:
        return None
    nodes = [nf[0] for nf in fn.next_functions]
    if len(nodes) != 2:
        return None
    xnode = _grad_edge_node(x)
    if xnode is None:
        return None
    for a, b in ((0, 1), (1, 0)):
        if nodes[b] is xnode and nodes[a] is not None:
            src = getattr(nodes[a], "_insr_src", None)
            if src is not None and src[1] is x and src[0].out_features == x.shape[-1]:
                return src[0], nodes[a], True
    return None


def jet_of(mlp, holder, x, mode):
    """Derivative jets are cached on the value tensor / node; a LAP jet also serves GRAD.
    A miss inside a hint scope records the mode for this call site's next iteration."""
    cache = getattr(holder, "_insr_jets", None)
    if cache is not None:
        for m in ((nat.MODE_LAP,) if mode == nat.MODE_LAP else (nat.MODE_GRAD, nat.MODE_LAP)):
            if m in cache:
                return cache[m]
    key = getattr(holder, "_insr_key", None)
    if key is not None and _HintScope.hints is not None:
        _HintScope.hints[key] = max(_HintScope.hints.get(key, nat.MODE_VALUE), mode)
    res = run_jet(mlp, x, mode)
    if cache is not None:
        cache[mode] = res
    return res
