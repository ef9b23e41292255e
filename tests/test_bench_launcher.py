"""bench.py --gpus N starts its own ranks (torch.distributed.run as a child process) when no
launcher did: rehearsed on the CPU with gloo (no GPU work), the rank-0 JSON line reports the
world size the process group really had."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_spawns_ranks_gloo_rehearsal():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rehearse",
                          "--steps", "5", "--warmup", "1", "--backend", "gloo"],
                         capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["process_group"]["world_size"] == 2
    assert sorted(rec["rank_devices"]) == [0, 1]
    assert rec["scaling"] == "weak"  # fluid2Dtlgn default; strong for the 8-GPU configs


def test_scaling_defaults():
    sys.path.insert(0, ROOT)
    import bench
    assert set(bench.STRONG_CONFIGS) == {"elasticity3Dbunny", "fluid2DtlgnM"}


def test_plain_run_options(monkeypatch):
    """--full and --dump-outputs are off in a plain run (the legs beside the timed steps run only with --full)."""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_writes_float32_arrays(tmp_path):
    """dump_outputs(): one float32 .npy per array of the last timed step -- every phase's loss dict and every
    trainable network's state_dict -- under names that say which."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench

    class Model:
        _trainable_networks = {"field": torch.nn.Linear(3, 2).double()}

    last = [{"main": torch.tensor(1.5), "bc": torch.tensor(0.25, dtype=torch.float64)}]
    names = bench.dump_outputs(str(tmp_path / "d"), Model(), {"phases": ("_advect",)}, last)
    assert names == ["loss.advect.bc", "loss.advect.main", "net.field.bias", "net.field.weight"]
    assert sorted(os.listdir(tmp_path / "d")) == [n + ".npy" for n in names]
    got = {n: np.load(tmp_path / "d" / (n + ".npy")) for n in names}
    assert all(v.dtype == np.float32 for v in got.values())
    assert float(got["loss.advect.main"]) == 1.5 and float(got["loss.advect.bc"]) == 0.25
    w = Model._trainable_networks["field"].weight.detach().to(torch.float32).numpy()
    assert got["net.field.weight"].shape == (2, 3) and np.array_equal(got["net.field.weight"], w)
