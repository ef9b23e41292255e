"""Cost of the hyperelastic materials in the one-launch elasticity energy (the materials paragraph).

    python tools/elastic_material_bench.py launch --parent-lib PATH [--launches 200] [--rounds 5]
        insr_elastic_energy with unit-seed gradients at 262,144 rows (d = 3) and 20,400 rows (d = 2), device
        events around `launches` launches after a warm-up, the variants alternated inside one process:
          a, a2  the parent commit's library (built into a directory outside git, e.g. insr-pde_amd/lib_exp/),
                 arap + volume + kinematics -- twice, for the spread
          b      this library, the same terms
          c      this library, neohookean + kinematics
    python tools/elastic_material_bench.py step [--iters 20] [--rounds 3]
        one ElasticityModel iteration at the elasticity3Dbunny configuration (graph replay), the stock energy
        list next to ["neohookean", "kinematics", "collision", "external"].

One JSON line per measurement on stdout (profiles/hyperelastic/*.jsonl)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "insr-pde_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


class ParentElastic(ctypes.Structure):
    """struct InsrElastic as the parent commit declares it (8 terms, no Lame parameters)."""
    _P, _I, _L, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    _fields_ = [("d", _I), ("n_order", _I), ("n", _L), ("rows", _L), ("f", _P), ("J", _P), ("x", _P),
                ("f_prev", _P), ("f_pp", _P), ("dt", _F), ("ratio", _F * 8), ("ext", _F * 3),
                ("target", _F * 3), ("plane_height", _F), ("center", _F * 3), ("radius", _F),
                ("row_l", _L), ("n_l", _L), ("row_r", _L), ("n_r", _L), ("order", _I * 8),
                ("out", _P), ("terms", _P), ("gf", _P), ("gJ", _P)]


def launch_bench(args):
    from base import _native as nat
    new = nat.lib()
    old = ctypes.CDLL(args.parent_lib)
    for lib in (new, old):
        lib.insr_elastic_work_floats.restype = ctypes.c_long
        lib.insr_elastic_energy.restype = ctypes.c_int
        lib.insr_elastic_energy.argtypes = [ctypes.c_void_p] * 3
    dev = torch.device("cuda")
    stream = nat.stream_of(dev)
    for d, n in ((3, 262144), (2, 20400)):
        g = torch.Generator().manual_seed(d)
        f = (0.3 * torch.randn(n, d, generator=g)).to(dev)
        J = (0.3 * torch.randn(n, d, d, generator=g)).to(dev)
        x = (torch.rand(n, d, generator=g) * 2 - 1).to(dev)
        fp = f + 0.05 * torch.randn(n, d, generator=g).to(dev)
        fpp = fp + 0.05 * torch.randn(n, d, generator=g).to(dev)
        out, terms = torch.empty((), device=dev), torch.empty(16, device=dev)
        gf, gJ = torch.empty_like(f), torch.empty_like(J)

        def make(lib, cls, names):
            e = cls()
            e.d, e.n, e.rows = d, n, n
            e.f, e.J, e.x, e.f_prev, e.f_pp = (t.data_ptr() for t in (f, J, x, fp, fpp))
            e.dt = 0.1
            for k, name in enumerate(names):
                t = nat.EL_IDS[name]
                e.ratio[t] = {"arap": 20.0, "volume": 1e3, "kinematics": 10.0}.get(name, 1.0)
                e.order[k] = t
            e.n_order = len(names)
            e.out, e.terms, e.gf, e.gJ = out.data_ptr(), terms.data_ptr(), gf.data_ptr(), gJ.data_ptr()
            if cls is nat.Elastic:
                e.mu, e.lam = 20.0, 1e3
            work = torch.zeros(lib.insr_elastic_work_floats(), device=dev)
            return lib, e, work

        stock = ["arap", "volume", "kinematics"]
        variants = {"a": make(old, ParentElastic, stock), "b": make(new, nat.Elastic, stock),
                    "c": make(new, nat.Elastic, ["neohookean", "kinematics"]), "a2": make(old, ParentElastic, stock)}

        def run(v, k):
            lib, e, work = variants[v]
            for _ in range(k):
                rc = lib.insr_elastic_energy(ctypes.byref(e), work.data_ptr(), stream)
                if rc != 0:
                    raise RuntimeError(f"insr_elastic_energy ({v}): {rc}")

        times = {v: [] for v in variants}
        for v in variants:
            run(v, 50)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for v in variants:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                run(v, args.launches)
                t1.record()
                t1.synchronize()
                times[v].append(t0.elapsed_time(t1) * 1e3 / args.launches)
        for v, ts in times.items():
            print(json.dumps({"bench": "elastic_launch", "variant": v, "d": d, "rows": n, "launches": args.launches,
                              "us_per_launch_median": round(statistics.median(ts), 3),
                              "us_per_launch_rounds": [round(t, 3) for t in ts]}), flush=True)


def step_bench(args):
    from pde.config import baseline_config
    from pde.elasticity import ElasticityModel
    lists = {"stock": None, "neohookean": ["neohookean", "kinematics", "collision", "external"]}
    models = {}
    for name, energy in lists.items():
        kw = {} if energy is None else dict(energy=energy, insr_lame_mu=1e2, insr_lame_lambda=1e3)
        cfg = baseline_config("elasticity3Dbunny", proj_dir="/tmp/insr_bench", insr_progress=False, early_stop=False,
                              max_n_iters=args.iters, insr_graph=True, insr_sync_every=10 ** 9, **kw)
        torch.manual_seed(0)
        m = ElasticityModel(cfg)
        m.timestep = 1
        m._solve_deformation()  # warm-up: the eager iteration, the capture, replays
        torch.cuda.synchronize()
        models[name] = m
    times = {name: [] for name in models}
    for _ in range(args.rounds):
        for name, m in models.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            m._solve_deformation()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / args.iters)
    for name, ts in times.items():
        print(json.dumps({"bench": "elastic_step", "config": "elasticity3Dbunny", "energy": models[name].energy,
                          "iters": args.iters, "ms_per_step_median": round(statistics.median(ts), 4),
                          "ms_per_step_rounds": [round(t, 4) for t in ts]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["launch", "step"])
    ap.add_argument("--parent-lib")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.what == "launch":
        if not a.parent_lib:
            ap.error("launch needs --parent-lib")
        launch_bench(a)
    else:
        step_bench(a)
