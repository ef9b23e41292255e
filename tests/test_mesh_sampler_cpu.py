"""Device mesh sampler, the part that needs no GPU: insr_mesh_points / insr_sample_mesh refuse malformed
arguments on the host before any launch (pointers here are dummies that are never dereferenced), the
uniforms-per-point query agrees with MeshSampler, the 3-tet table's cumulative measure is exact, the ctypes
mirror of InsrMesh has the C layout, and the model flag is off by default."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insr_siren.h")
EINVAL = -1
P = [0x10000 * (i + 1) for i in range(6)]  # distinct fake device addresses

TAB_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1], [0, 0, -2]], np.float64)
TAB_T = np.array([[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 2, 5]])
TRI_V = np.array([[0, 0], [1, 0], [0, 1], [-2, 0]], np.float64)
TRI_F = np.array([[0, 1, 2], [0, 2, 3]])


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import base
    return base._native.load(ge.LIB)


def mesh(cdf=P[0], corners=P[1], k=10, nc=4, dim=3):
    from base import _native as nat
    return nat.Mesh(cdf, corners, k, nc, dim)


def points(lib, m, n=64, uniforms=P[2], out=P[3], elem=P[4]):
    return lib.insr_mesh_points(None if m is None else ctypes.byref(m), uniforms, n, out, elem, None)


def sample(lib, m, n=64, out=P[3], elem=P[4], state=P[5]):
    return lib.insr_sample_mesh(None if m is None else ctypes.byref(m), n, out, elem, 1234, state, None)


GRID_MAX = 0x7FFFFFFF * 256  # points of the largest 32-bit grid of 256-thread blocks
BAD_MESHES = [None, dict(cdf=None), dict(corners=None), dict(nc=2), dict(nc=5), dict(dim=1), dict(dim=4),
              dict(nc=4, dim=2), dict(k=0), dict(k=-3)]


@pytest.mark.parametrize("call", [points, sample])
def test_host_refusals_come_before_any_launch(lib, call):
    for bad in BAD_MESHES:
        assert call(lib, None if bad is None else mesh(**bad)) == EINVAL, bad
        assert call(lib, None if bad is None else mesh(**bad), n=0) == EINVAL, bad  # also when nothing would launch
    assert call(lib, mesh(), out=None) == EINVAL
    assert call(lib, mesh(), n=-1) == EINVAL
    assert call(lib, mesh(), n=GRID_MAX + 1) == EINVAL
    for shape in (dict(nc=4, dim=3), dict(nc=3, dim=3), dict(nc=3, dim=2), dict(k=1)):
        assert call(lib, mesh(**shape), n=0) == 0, shape  # valid, nothing to draw: no launch
        assert call(lib, mesh(**shape), n=0, elem=None) == 0, shape


def test_each_entry_refuses_its_own_null_pointer(lib):
    assert points(lib, mesh(), uniforms=None) == EINVAL
    assert sample(lib, mesh(), state=None) == EINVAL


def test_uniforms_per_point_agree_with_the_python_sampler(lib):
    from pde import mesh as M
    assert lib.insr_mesh_uniforms_per_point(4) == 6 and lib.insr_mesh_uniforms_per_point(3) == 4
    for nc in (-1, 0, 2, 5):
        assert lib.insr_mesh_uniforms_per_point(nc) == EINVAL
    assert M.MeshSampler(TAB_V, TAB_T).uniforms_per_point() == lib.insr_mesh_uniforms_per_point(4)
    assert M.MeshSampler(TRI_V, TRI_F).uniforms_per_point() == lib.insr_mesh_uniforms_per_point(3)


def test_three_tet_table_has_an_exact_cdf():
    from pde import mesh as M
    s = M.MeshSampler(TAB_V, TAB_T)
    assert s.cdf.dtype.is_floating_point and s.cdf.element_size() == 8
    assert s.cdf.tolist() == [0.25, 0.5, 1.0]


def test_device_methods_need_the_gpu():
    import torch
    from base._native import NativeUnavailable
    from base.sampling import sample_mesh_into
    from pde import mesh as M
    s = M.MeshSampler(TAB_V, TAB_T)
    with pytest.raises(NativeUnavailable):
        s.sample_device(4)
    with pytest.raises(NativeUnavailable):
        s.points_device(torch.zeros(4, 6))
    with pytest.raises(NativeUnavailable):
        sample_mesh_into(torch.zeros(8, 3), 0, 4, s)
    flat = s.leading(2)  # same elements and measures, the first two coordinates
    assert flat.cdf is s.cdf and flat.corners.shape == (3, 4, 2) and flat.corners.is_contiguous()
    assert torch.equal(flat.corners, s.corners[:, :, :2]) and s.leading(3) is s


def test_mesh_struct_layout_matches_header(tmp_path):
    from base import _native as nat
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(InsrMesh));']
    for fname, _ in nat.Mesh._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(InsrMesh, {fname}));')
    lines.append("  return 0;\n}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(nat.Mesh)
    for fname, _ in nat.Mesh._fields_:
        assert int(got[fname]) == getattr(nat.Mesh, fname).offset, fname


def test_model_flag_is_off_by_default():
    from pde.config import baseline_config, make_config
    assert make_config("elasticity").insr_mesh_batch is False
    assert baseline_config("elasticity3Dbunny").insr_mesh_batch is False
