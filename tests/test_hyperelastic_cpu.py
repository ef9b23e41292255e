"""The hyperelastic materials' C ABI and Python surface, without a GPU: the term ids, the struct
layout, the exported symbols, and the host-side refusals of insr_elastic_energy and
insr_hyperelastic_fwd / bwd (INSR_EINVAL before any device call; the pointers are dummies that
are never dereferenced)."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insr_siren.h")
EINVAL = -1
P = [0x10000 * (i + 1) for i in range(12)]  # distinct fake device addresses


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import base
    return base._native.load(ge.LIB)


def test_term_ids():
    from base import _native as nat
    assert nat.EL_IDS["neohookean"] == 8 and nat.EL_IDS["stvk"] == 9 and nat.EL_TERMS == 10
    assert nat.EL_MATERIALS == {"neohookean": 0, "stvk": 1}
    text = open(HEADER).read()
    for name, value in (("NEOHOOKEAN", 8), ("STVK", 9), ("TERMS", 10)):
        assert f"#define INSR_EL_{name} {value}\n" in text


def test_struct_size_matches_header(tmp_path):
    """sizeof(InsrElastic) and the offsets of its new tail, from the C compiler."""
    from base import _native as nat
    fields = ("ratio", "order", "gJ", "mu", "lam")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(InsrElastic));']
    lines += [f'  printf("{f} %zu\\n", offsetof(InsrElastic, {f}));' for f in fields]
    lines.append("  return 0;\n}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.Elastic)
    for f in fields:
        assert int(got[f]) == getattr(nat.Elastic, f).offset, f
    assert nat.Elastic._fields_[-2:] == [("mu", ctypes.c_float), ("lam", ctypes.c_float)]


def test_exports_new_symbols(lib):
    for name in ("insr_hyperelastic_fwd", "insr_hyperelastic_bwd"):
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
    assert lib.insr_version() >= 400


def elastic(material, mu, lam, J=P[1]):
    from base import _native as nat
    e = nat.Elastic()
    e.d, e.n, e.rows = 3, 64, 64
    e.f, e.J, e.x, e.f_prev, e.f_pp = P[0], J, P[2], P[3], P[4]
    e.dt, e.mu, e.lam = 0.1, mu, lam
    e.ratio[nat.EL_IDS[material]] = 1.0
    e.n_order, e.order[0] = 1, nat.EL_IDS[material]
    e.out, e.terms, e.gf, e.gJ = P[5], P[6], P[7], P[8]
    return e


@pytest.mark.parametrize("material,mu,lam,J", [
    ("neohookean", 20.0, 0.0, P[1]),           # lam = 0: alpha = 1 + (mu / lam) d / (d + 1) is undefined
    ("neohookean", 20.0, -1.0, P[1]),          # lam < 0
    ("neohookean", -1.0, 1e3, P[1]),           # mu < 0
    ("neohookean", float("nan"), 1e3, P[1]),
    ("stvk", 20.0, float("inf"), P[1]),        # StVK: both finite
    ("stvk", float("nan"), 1e3, P[1]),
    ("neohookean", 20.0, 1e3, None),           # a material on with J = NULL
    ("stvk", 20.0, 1e3, None),
])
def test_elastic_energy_refuses_on_the_host(lib, material, mu, lam, J):
    e = elastic(material, mu, lam, J)
    assert lib.insr_elastic_energy(ctypes.byref(e), P[9], None) == EINVAL


@pytest.mark.parametrize("material,mu,lam", [(-1, 20.0, 1e3), (2, 20.0, 1e3), (0, 20.0, 0.0), (0, 20.0, -2.0),
                                             (0, -1.0, 1e3), (1, float("inf"), 1e3)])
def test_standalone_pair_refuses_on_the_host(lib, material, mu, lam):
    assert lib.insr_hyperelastic_fwd(P[0], 64, 3, material, mu, lam, P[1], P[2], None) == EINVAL
    assert lib.insr_hyperelastic_bwd(P[0], 64, 3, material, mu, lam, P[1], P[2], None) == EINVAL


def test_standalone_pair_refuses_bad_shapes(lib):
    assert lib.insr_hyperelastic_fwd(None, 64, 3, 0, 20.0, 1e3, P[1], P[2], None) == EINVAL
    assert lib.insr_hyperelastic_fwd(P[0], 64, 4, 0, 20.0, 1e3, P[1], P[2], None) == EINVAL
    assert lib.insr_hyperelastic_fwd(P[0], 5000, 3, 0, 20.0, 1e3, P[1], None, None) == EINVAL  # partials needed
    assert lib.insr_hyperelastic_bwd(P[0], 64, 3, 1, 20.0, 1e3, None, P[2], None) == EINVAL
    assert lib.insr_hyperelastic_bwd(P[0], 0, 3, 1, 20.0, 1e3, P[1], P[2], None) == 0  # nothing to do


@pytest.mark.parametrize("kw", [{}, {"mu": 20.0}, {"lam": 1e3}, {"mu": 20.0, "lam": 0.0}, {"mu": 20.0, "lam": -1.0},
                                {"mu": -1.0, "lam": 1e3}, {"mu": float("nan"), "lam": 1e3}])
def test_python_refuses_a_material_without_valid_parameters(kw, monkeypatch):
    """ValueError before any library call (CPU tensors: a library call would raise NativeUnavailable)."""
    import base
    from base import _native as nat
    monkeypatch.setattr(nat, "lib", lambda: pytest.fail("library call"))
    z = torch.zeros(10, 2)
    with pytest.raises(ValueError):
        base.elastic_energy(z, torch.zeros(10, 2, 2), z, z, z, n=10, dt=0.1, energy=["neohookean"], ratios={}, **kw)
    with pytest.raises(ValueError):
        base.hyperelastic_energy(torch.zeros(10, 2, 2), "neohookean", kw.get("mu"), kw.get("lam"))
    with pytest.raises(ValueError):
        base.hyperelastic_energy(torch.zeros(10, 2, 2), "mooney", 20.0, 1e3)
    with pytest.raises(ValueError):
        base.elastic_energy(z, None, z, z, z, n=10, dt=0.1, energy=["stvk"], ratios={}, mu=20.0, lam=1e3)


def test_config_carries_the_lame_parameters():
    from pde.config import baseline_config
    cfg = baseline_config("elasticity2Dstretch")
    assert cfg.insr_lame_mu is None and cfg.insr_lame_lambda is None
    cfg = baseline_config("elasticity2Dstretch", insr_lame_mu=1.0, insr_lame_lambda=10.0)
    assert (cfg.insr_lame_mu, cfg.insr_lame_lambda) == (1.0, 10.0)
