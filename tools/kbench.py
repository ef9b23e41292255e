"""Kernel micro-benchmark: fwd / bwd jet kernels back-to-back on one stream
(HIP events around R launches, no host gaps), for both kernel variants.

    python tools/kbench.py [--nets fluid_pres,fluid_vel] [--sizes 324,4096,16384]
    python tools/kbench.py --hessian | --xgrad | --mesh
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "insr-pde_amd")]

import torch  # noqa: E402

NETS = {"fluid_pres": (2, 1, 4, 128), "fluid_vel": (2, 2, 4, 128), "advect": (1, 1, 3, 64),
        "el2d": (2, 2, 5, 128), "el3d": (3, 3, 5, 256)}
VARIANTS = {  # label: ((fwd, bwd) forced tiles, (fwd, bwd) precision)
    "split1": ((1, 1), (0, 0)),
    "split2": ((2, 2), (0, 0)),
    "split4": ((4, 4), (0, 0)),
    "auto": ((0, 0), (0, 0)),
    "x6": ((0, 0), (1, 1)),
    "x6_1": ((1, 1), (1, 1)),
    "x6_2": ((2, 2), (1, 1)),
    "x6_4": ((4, 4), (1, 1)),
    "x6w": ((0, 0), (1, 1)),  # x6 with the two-kernel backward from width 128
    "x3": ((0, 0), (2, 2)),   # 3 bf16 products per fp32 product
    "bf": ((0, 0), (3, 3)),   # plain bf16 operands
    "h3": ((0, 0), (4, 1)),   # fp16 two-term forward (f16x3), x6 backward
}
MODES = {"value": 0, "grad": 1, "lap": 2}


def P_macs(din, dout, L, W):
    return din * W + L * W * W + W * dout


def time_it(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


HESS_SHAPES = [((2, 1, 4, 128), 16708), ((3, 3, 4, 128), 16384)]  # (d_in, d_out, L, W), points


def hessian_lines(args):
    """--hessian: the second-order jet (csrc/jet_hess.hpp) against what hessian() does without it (the
    polarised Laplacian jets for d_in = 2, the reference-semantics autograd route for d_in = 3), through
    base.hessian: the forward, and forward + backward of sum(H . R) into .grad including the sums.  The two
    routes alternate line by line, `rounds` times; a last line per shape times the two kernels alone
    (forward; backward + partial-row sums into the flat gradient)."""
    import base
    from base import _native as nat
    lib = nat.load()
    for (din, dout, L, W), n in HESS_SHAPES:
        torch.manual_seed(0)
        net = base.MLP(din, dout, L, W, nonlinearity="sine").cuda()
        flat, P = net.flat_params(), net.param_count
        x = (torch.rand(n, din, device="cuda") * 2 - 1).contiguous()
        R = torch.randn(n, dout, din, din, device="cuda")

        def api_fwd(flag):
            net.hessian_jet = flag
            xg = x.detach().requires_grad_(True)
            return base.hessian(net(xg), xg)[0]

        def api_fwd_bwd(flag):
            net.zero_grad(set_to_none=True)
            (api_fwd(flag) * R).sum().backward()

        for r in range(args.rounds):
            for flag in (True, False):
                rec = {"shape": [din, dout, L, W], "n": n, "route": "jet" if flag else "present", "round": r,
                       "fwd_us": round(time_it(lambda: api_fwd(flag), args.reps), 1),
                       "fwd_bwd_us": round(time_it(lambda: api_fwd_bwd(flag), args.reps), 1)}
                print(json.dumps(rec), flush=True)
        y = torch.empty(n, dout, device="cuda")
        dy = torch.empty(n, dout, din, device="cuda")
        h = torch.empty(n, dout, din, din, device="cuda")
        gy, gdy, gh = torch.randn_like(y), torch.randn_like(dy), torch.randn_like(h)
        act = torch.empty(lib.insr_hess_act_bytes(n, din, L, W) // 4, device="cuda")
        nb, stride = lib.insr_hess_partial_blocks(n, din, W), lib.insr_jet_partial_stride(din, dout, L, W)
        part = torch.empty(nb * stride, device="cuda")
        g = torch.zeros(P, device="cuda")
        st = nat.stream_of(x.device)

        def fwd():
            nat.check(lib.insr_siren_hess_fwd(nat.ptr(x), n, din, dout, L, W, nat.ptr(flat), nat.ptr(y), nat.ptr(dy),
                                              nat.ptr(h), nat.ptr(act), st), "hess_fwd")

        def bwdg():
            nat.check(lib.insr_siren_hess_bwd(nat.ptr(x), n, din, dout, L, W, nat.ptr(flat), nat.ptr(act),
                                              nat.ptr(gy), nat.ptr(gdy), nat.ptr(gh), nat.ptr(part), st), "hess_bwd")
            nat.check(lib.insr_reduce_partials_strided(nat.ptr(part), nb, P, stride, nat.ptr(g), 0, st), "reduce")

        tf = time_it(fwd, args.reps)
        fwd()
        print(json.dumps({"shape": [din, dout, L, W], "n": n, "route": "jet kernels", "nb": nb,
                          "fwd_us": round(tf, 2), "bwd_grad_us": round(time_it(bwdg, args.reps), 2)}), flush=True)


XGRAD_SHAPES = [((2, 1, 4, 128), "lap", 16708), ((2, 2, 4, 128), "value", 16708)]  # shape, jet mode, points


def xgrad_lines(args):
    """--xgrad: what the coordinate gradient (MLP.coord_grad, csrc/jet_xadj.hpp) adds to a backward.  Per
    shape, `rounds` times, alternating: the backward of one jet call through autograd (the adjoints handed to
    torch.autograd.backward, so no loss arithmetic is timed) with the flag off, with the flag on (+ the
    x-adjoint launch), and with the flag off followed by the torch route the nodes take where no kernel serves
    a call (_jet._torch_x_adjoint); a last line per shape times the two kernels alone: the parameter backward
    into .grad including its sums, and insr_siren_jet_bwd_x."""
    import warnings
    import base
    from base import _jet, _native as nat
    lib = nat.load()
    for (din, dout, L, W), mname, n in XGRAD_SHAPES:
        mode = MODES[mname]
        torch.manual_seed(0)
        net = base.MLP(din, dout, L, W, nonlinearity="sine", coord_grad=True).cuda()
        x = (torch.rand(n, din, device="cuda") * 2 - 1).contiguous()
        xg = x.detach().requires_grad_(True)
        outs = [o for o in _jet.run_jet(net, xg, mode) if o is not None]
        adj = [torch.randn_like(o) for o in outs]
        full = (adj + [None, None])[:3]

        def bwd(flag):
            net.coord_grad = flag
            xg.grad = None
            torch.autograd.backward(outs, adj, retain_graph=True)

        def bwd_torch():
            bwd(False)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                _jet._torch_x_adjoint(net, lambda xd: _jet.torch_jet(net, xd, mode), xg, full, (mname, din, dout, L, W))

        for r in range(args.rounds):
            rec = {"shape": [din, dout, L, W], "mode": mname, "n": n, "round": r,
                   "bwd_flag_off_us": round(time_it(lambda: bwd(False), args.reps), 1),
                   "bwd_flag_on_us": round(time_it(lambda: bwd(True), args.reps), 1),
                   "bwd_torch_route_us": round(time_it(bwd_torch, args.reps), 1)}
            print(json.dumps(rec), flush=True)
        net.ensure_wsplit()
        cmode = net.call_mode(mode)
        flat, P = net.flat_params(), net.param_count
        y = torch.empty(n, dout, device="cuda")
        dy = torch.empty(n, dout, din, device="cuda")
        lap = torch.empty(n, dout, device="cuda")
        act = torch.empty(lib.insr_jet_act_bytes(n, din, L, W, cmode) // 4, device="cuda")
        st = nat.stream_of(x.device)
        nat.check(lib.insr_siren_jet_fwd(nat.ptr(x), n, din, dout, L, W, cmode, nat.ptr(flat), nat.ptr(y), nat.ptr(dy),
                                         nat.ptr(lap), nat.ptr(act), st), "fwd")
        work = torch.empty(max(lib.insr_jet_bwd_work_bytes(n, din, dout, L, W, cmode) // 4, 1), device="cuda")
        g = torch.zeros(P, device="cuda")
        gx = torch.empty(n, din, device="cuda")
        gy, gdy, glap = full

        def bwdg():
            nat.check(lib.insr_siren_jet_bwd_grad(nat.ptr(x), n, din, dout, L, W, cmode, nat.ptr(flat), nat.ptr(act),
                                                  nat.ptr(gy), nat.ptr(gdy), nat.ptr(glap), nat.ptr(work), nat.ptr(g),
                                                  0, st), "bwd_grad")

        def bwdx():
            nat.check(lib.insr_siren_jet_bwd_x(n, din, dout, L, W, cmode, nat.ptr(flat), nat.ptr(act), nat.ptr(gy),
                                               nat.ptr(gdy), nat.ptr(glap), nat.ptr(gx), st), "bwd_x")

        print(json.dumps({"shape": [din, dout, L, W], "mode": mname, "n": n, "route": "kernels",
                          "path": lib.insr_jet_bwd_path(n, din, dout, L, W, cmode),
                          "bwd_grad_us": round(time_it(bwdg, args.reps), 2),
                          "bwd_x_us": round(time_it(bwdx, args.reps), 2)}), flush=True)


MESH_SIZES = [32768, 262144]  # the elasticity3Dbunny draw: one rank of 8, and the whole batch


def mesh_lines(args):
    """--mesh: one draw of n volume-weighted points in the bunny (tests/golden/bunny_mesh.npz), us per draw by
    HIP events after warm-up, three routes alternating line by line, `rounds` times:
      A  base.sample_boxes + MeshSampler.sample(uniforms=...)   (a sharded rank's _mesh_draw)
      B  MeshSampler.sample(generator=None)                      (one unsharded rank's _mesh_draw)
      C  MeshSampler.sample_device                               (insr_sample_mesh, one launch)
    then elasticity3Dbunny as shard (0, 8) with the graph loop (bench.py --config elasticity3Dbunny --shard-of 8),
    cfg.insr_mesh_batch off against on, ms per iteration over windows of `reps` iterations, alternating."""
    import time
    import base
    from base._loop import PhaseLoop
    from pde.config import BUNNY_FIXTURE, baseline_config
    from pde.elasticity import ElasticityModel
    from pde.mesh import MeshSampler, load_mesh
    base._native.load()
    V, E, _ = load_mesh(BUNNY_FIXTURE, 3)
    s = MeshSampler(V.double(), E, device="cuda")
    m = s.uniforms_per_point()
    torch.manual_seed(0)
    for n in MESH_SIZES:
        out = torch.empty(n, 3, device="cuda")
        routes = {"A boxes+sample(uniforms)": lambda: s.sample(n, uniforms=base.sample_boxes(
                      [(n * m // 3, (0.0,) * 3, (1.0,) * 3)], 3).view(n, m)),
                  "B sample(generator=None)": lambda: s.sample(n),
                  "C sample_device": lambda: s.sample_device(n, out=out)}
        for fn in routes.values():  # warm every shape the timed windows use
            time_it(fn, 5)
        for r in range(args.rounds):
            for name, fn in routes.items():
                print(json.dumps({"mesh": "bunny", "k": s.k, "n": n, "route": name, "round": r,
                                  "us_per_draw": round(time_it(fn, args.reps), 2)}), flush=True)
    loops = {}
    for flag in (False, True):
        cfg = baseline_config("elasticity3Dbunny", insr_graph=True, insr_graph_unroll=4, insr_sync_every=10 ** 9,
                              insr_progress=False, early_stop=False, proj_dir="/tmp/insr_bench", max_n_iters=10 ** 9,
                              insr_shard=(0, 8), insr_mesh_batch=flag)
        torch.manual_seed(1234)
        model = ElasticityModel(cfg)
        model.timestep = 1
        pl = PhaseLoop(model, ElasticityModel._solve_deformation._insr_phase, "_solve_deformation", (), {})
        pl.start()
        pl.run_iters(0, 2 + 4 * 3)  # eager, captured, then whole replayed groups
        torch.cuda.synchronize()
        loops[flag] = pl
    i0 = 14
    for r in range(args.rounds):
        for flag, pl in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pl.run_iters(i0, 4 * args.reps)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / (4 * args.reps) * 1e3
            print(json.dumps({"phase": "elasticity3Dbunny shard (0, 8)", "insr_mesh_batch": flag, "round": r,
                              "iters": 4 * args.reps, "captured": getattr(pl.m, "_insr_capture_error", None) is None,
                              "ms_per_iter": round(ms, 4)}), flush=True)
        i0 += 4 * args.reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", action="store_true", help="the mesh sampler lines (see mesh_lines)")
    ap.add_argument("--xgrad", action="store_true", help="the coordinate-gradient lines (see xgrad_lines)")
    ap.add_argument("--hessian", action="store_true", help="the Hessian lines (see hessian_lines) instead of the jets")
    ap.add_argument("--rounds", type=int, default=3, help="--hessian / --xgrad: alternations of the routes")
    ap.add_argument("--nets", default="fluid_pres,fluid_vel")
    ap.add_argument("--sizes", default="324,2048,8192,16384,65536")
    ap.add_argument("--modes", default="value,grad,lap")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--policies", default="0", help="backward-path policies (INSR_JET_POLICY mode bits) to time")
    ap.add_argument("--bwd-only", action="store_true", help="time only the backward into .grad")
    ap.add_argument("--bwd-f16", type=int, default=-1, help="INSR_JET_BWD_F16 mask (-1: library default)")
    ap.add_argument("--lib", default=None, help="alternative build of libinsr_hip.so (flag studies)")
    args = ap.parse_args()
    if args.mesh:
        return mesh_lines(args)
    if args.hessian:
        return hessian_lines(args)
    if args.xgrad:
        return xgrad_lines(args)
    import base
    from base import _native as nat
    lib = nat.load(args.lib, check_build=args.lib is None)
    f16bits = nat.jet_bwd_f16(args.bwd_f16) if args.bwd_f16 >= 0 else 0
    out = []
    for name in args.nets.split(","):
        din, dout, L, W = NETS[name]
        torch.manual_seed(0)
        net = base.MLP(din, dout, L, W, nonlinearity="sine").cuda()
        flat = net.flat_params()
        try:  # libraries with pre-split weight planes: prepare them once, pass INSR_MODE_WSPLIT
            lib.insr_siren_wsplit
            net.refresh_wsplit()
            wbit = nat.MODE_WSPLIT
        except AttributeError:
            wbit = 0
        P = net.param_count
        for mname in args.modes.split(","):
            mode0 = MODES[mname] | wbit | f16bits
            if (mode0 & 0xF) == 2 and din > 2:
                continue
            S = {0: 1, 1: 1 + din, 2: 2 + din}[mode0 & 0xF]
            for n in [int(v) for v in args.sizes.split(",")]:
                x = (torch.rand(n, din, device="cuda") * 2 - 1).contiguous()
                y = torch.empty(n, dout, device="cuda")
                dy = torch.empty(n, dout, din, device="cuda")
                lap = torch.empty(n, dout, device="cuda")
                gy, gdy, glap = torch.randn_like(y), torch.randn_like(dy), torch.randn_like(lap)
                act = torch.empty(lib.insr_jet_act_bytes(n, din, L, W, mode0) // 4, device="cuda")
                g = torch.zeros(P, device="cuda")
                st = nat.stream_of(x.device)
                for variant, pol in [(v, int(p)) for v in args.variants.split(",") for p in args.policies.split(",")]:
                    tiles, prec = VARIANTS[variant]
                    # the variant as per-call mode bits (the library keeps no configuration)
                    mode = mode0 | nat.knob_bits(policy=pol, tiles=tiles, prec=prec, wide128=variant.endswith("w"))
                    part = torch.empty(max(lib.insr_jet_partial_bytes(n, din, dout, L, W, mode) // 4, 1), device="cuda")
                    nb = lib.insr_jet_partial_blocks(n, din, W, mode)
                    tf_, tb_ = (lib.insr_jet_split_tiles(n, din, W, mode, 0),
                                lib.insr_jet_split_tiles(n, din, W, mode, 1))

                    def fwd():
                        nat.check(lib.insr_siren_jet_fwd(nat.ptr(x), n, din, dout, L, W, mode, nat.ptr(flat),
                                                         nat.ptr(y), nat.ptr(dy), nat.ptr(lap), nat.ptr(act), st),
                                  "fwd")

                    def bwd():
                        nat.check(lib.insr_siren_jet_bwd(nat.ptr(x), n, din, dout, L, W, mode, nat.ptr(flat),
                                                         nat.ptr(act), nat.ptr(gy), nat.ptr(gdy), nat.ptr(glap),
                                                         nat.ptr(part), st), "bwd")

                    work = torch.empty(max(lib.insr_jet_bwd_work_bytes(n, din, dout, L, W, mode) // 4, 1),
                                       device="cuda")
                    wide = lib.insr_jet_bwd_is_wide(n, din, W, mode)

                    def bwdg():  # backward straight into .grad (the path the autograd bridge takes)
                        nat.check(lib.insr_siren_jet_bwd_grad(nat.ptr(x), n, din, dout, L, W, mode, nat.ptr(flat),
                                                              nat.ptr(act), nat.ptr(gy), nat.ptr(gdy), nat.ptr(glap),
                                                              nat.ptr(work), nat.ptr(g), 0, st), "bwd_grad")

                    def red():
                        nat.check(lib.insr_reduce_partials_strided(nat.ptr(part), nb, P,
                                                                   lib.insr_jet_partial_stride(din, dout, L, W),
                                                                   nat.ptr(g), 0, st), "reduce")

                    tf = time_it(fwd, args.reps)
                    fwd()
                    tb = 1e9 if args.bwd_only else time_it(bwd, args.reps)
                    tr = 1e9 if args.bwd_only else time_it(red, args.reps)
                    tg = time_it(bwdg, args.reps)
                    macs = P_macs(din, dout, L, W)
                    rec = {"net": name, "mode": mname, "n": n, "variant": variant, "policy": pol,
                           "path": lib.insr_jet_bwd_path(n, din, dout, L, W, mode), "T": [tf_, tb_], "nb": nb,
                           "fwd_us": round(tf, 2),
                           "bwd_us": round(tb, 2), "reduce_us": round(tr, 2), "bwd_grad_us": round(tg, 2),
                           "wide": wide, "bwd_grad_tflops": round(n * S * 4 * macs / tg / 1e6, 2),
                           "fwd_tflops": round(n * S * 2 * macs / tf / 1e6, 2),
                           "bwd_tflops": round(n * S * 4 * macs / tb / 1e6, 2)}
                    out.append(rec)
                    print(json.dumps(rec), flush=True)



if __name__ == "__main__":
    main()
