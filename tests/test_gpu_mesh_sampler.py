"""Device mesh sampler (csrc/mesh_sampler.hip: insr_mesh_points / insr_sample_mesh; pde.mesh.MeshSampler
.points_device / .sample_device; base.sampling.sample_mesh_into; ElasticityModel._mesh_batch).

Two judges.  The first is a numpy / fp64 restatement written here: Philox-4x32-10 (as test_gpu_sampler.py),
u = u0 + u1 2^-24, elem = min(searchsorted(cdf, u, right), k - 1), tets bary = e / sum e with
e = -log(max(r, 1e-30)), triangles bary = (1 - su, su (1 - r1), su r1) with su = sqrt(r0), point =
sum bary corner.  The second is MeshSampler.sample(uniforms=...), the torch path the launch replaces.
Elements must match exactly; points within max|delta| <= 1e-5 max|corner| (the project's normwise 1e-5).

Tie rows on the 3-tet table (cdf exactly (.25, .5, 1)).  The row u0 = .25 - 2^-24, u1 = 1 - 2^-24 sums to
.25 - 2^-48, just below .25: MeshSampler.sample -- the reference -- gives element 0 there; the element-1 row
"just below .5" is u0 = .5 - 2^-24, u1 = 1 - 2^-24.  Both rows are checked, each against the reference."""
import os

import numpy as np
import pytest
import torch

from pde import mesh as M

pytestmark = pytest.mark.gpu
TOL = 1e-5
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
E24 = 2.0 ** -24
BUNNY_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bunny_mesh.npz")

# unit cube [-1, 1]^3 split into 6 tets around the main diagonal (0 -> 7), as tests/test_mesh.py
CUBE_V = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64)
CUBE_T = np.array([[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]])
# three tets on one base triangle, volumes 1 : 1 : 2 -> cdf exactly (.25, .5, 1); corner 3 tells them apart
TAB_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1], [0, 0, -2]], np.float64)
TAB_T = np.array([[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 2, 5]])
TRI_V = np.array([[0, 0], [1, 0], [0, 1], [-2, 0]], np.float64)  # areas 0.5 and 1.0
TRI_F = np.array([[0, 1, 2], [0, 2, 3]])


def philox4x32_10(key, ctr):
    """numpy Philox-4x32-10; key (k0, k1), ctr (N, 4) uint32 -> (N, 4) uint32."""
    c = np.array(ctr, dtype=np.uint64)
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(M0) * c[:, 0]
        p1 = np.uint64(M1) * c[:, 2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & mask
        hi1, lo1 = p1 >> np.uint64(32), p1 & mask
        c = np.stack([hi1 ^ c[:, 1] ^ k0, lo1, hi0 ^ c[:, 3] ^ k1, lo0], axis=1)
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return c.astype(np.uint32)


def test_numpy_philox_known_answer():
    assert philox4x32_10((0, 0), [[0, 0, 0, 0]]).tolist() == [[0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]]


def stream_uniforms(seed, base, total):
    """Values 0 .. total - 1 of a launch that starts at Philox counter `base`, as fp32 uniforms."""
    groups = (total + 3) // 4
    ctr = np.zeros((groups, 4), dtype=np.uint64)
    g = np.arange(groups, dtype=np.uint64) + np.uint64(base)
    ctr[:, 0], ctr[:, 1] = g & np.uint64(0xFFFFFFFF), g >> np.uint64(32)
    bits = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), ctr).reshape(-1)[:total]
    return (bits >> 8).astype(np.float32) * np.float32(E24)


def restate(s, U):
    """(elements, fp64 points) of sampler s at the fp32 uniforms U (n, m)."""
    cdf, cor = s.cdf.cpu().numpy(), s.corners.cpu().numpy().astype(np.float64)
    U = np.asarray(U, np.float32)
    u = U[:, 0].astype(np.float64) + U[:, 1].astype(np.float64) * E24
    elem = np.minimum(np.searchsorted(cdf, u, side="right"), len(cdf) - 1)
    r = U[:, 2:].astype(np.float64)
    if cor.shape[1] == 4:
        e = -np.log(np.maximum(r, np.float64(np.float32(1e-30))))
        b = e / e.sum(1, keepdims=True)
    else:
        su = np.sqrt(r[:, :1])
        b = np.concatenate([1 - su, su * (1 - r[:, 1:]), su * r[:, 1:]], 1)
    return elem, (b[:, :, None] * cor[elem]).sum(1)


def bary_in(cor, p):
    """fp64 barycentric coordinates (n, nc) of points p (n, dim) in elements cor (n, nc, dim) (least squares
    where the element does not span the space: a triangle in 3-d)."""
    A = np.swapaxes(cor[:, 1:] - cor[:, :1], 1, 2)  # (n, dim, nc - 1)
    b = (p - cor[:, 0])[:, :, None]
    At = np.swapaxes(A, 1, 2)
    lam = np.linalg.solve(At @ A, At @ b)[:, :, 0]
    return np.concatenate([1 - lam.sum(1, keepdims=True), lam], 1)


def bound(s):
    return TOL * float(s.corners.abs().max())


@pytest.fixture(scope="module")
def B():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import base
    base._native.load()
    return base


@pytest.fixture(scope="module")
def S(B):
    """The fixtures' samplers, tables on the device."""
    Vb, Eb, _ = M.load_mesh(BUNNY_NPZ, 3)
    return {"cube": M.MeshSampler(CUBE_V, CUBE_T, device="cuda"),
            "table": M.MeshSampler(TAB_V, TAB_T, device="cuda"),
            "tri2": M.MeshSampler(TRI_V, TRI_F, device="cuda"),
            "tri3": M.MeshSampler(CUBE_V, M.boundary_faces(CUBE_T), device="cuda"),  # the cube's 12 surface triangles
            "bunny": M.MeshSampler(Vb.double(), Eb, device="cuda")}


def check_points(s, U, pts, elem):
    """Both judges at uniforms U (numpy (n, m) fp32) for the device's (pts, elem)."""
    e_ref, p_ref = restate(s, U)
    assert np.array_equal(elem.cpu().numpy(), e_ref)
    err = float(np.abs(pts.double().cpu().numpy() - p_ref).max())
    twin = s.sample(U.shape[0], uniforms=torch.as_tensor(U, device="cuda"))
    err2 = float((pts - twin).abs().max())
    print(f"n={U.shape[0]} restatement err {err:.3e} torch err {err2:.3e} bound {bound(s):.3e}")
    assert err <= bound(s) and err2 <= bound(s)


# ---- 1. insr_mesh_points ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("name", ["cube", "table", "tri2", "tri3"])
def test_points_match_both_judges(S, name, n):
    s = S[name]
    m = s.uniforms_per_point()
    U = np.random.default_rng(1000 * n + m).integers(0, 1 << 24, size=(n, m)).astype(np.float32) * np.float32(E24)
    pts, elem = s.points_device(torch.as_tensor(U, device="cuda"), elements=True)
    assert pts.shape == (n, s.corners.shape[2]) and pts.dtype == torch.float32 and elem.dtype == torch.int32
    check_points(s, U, pts, elem)
    only = s.points_device(torch.as_tensor(U, device="cuda"))  # elem = NULL is accepted
    assert torch.equal(only, pts)


def test_ties_and_edges_of_the_element_search(S):
    s = S["table"]
    assert s.cdf.cpu().tolist() == [0.25, 0.5, 1.0]
    top = 1 - E24
    near3 = [top, top, top, 0.0]  # barycentrics ~ (0, 0, 0, 1): the point sits on corner 3, z = 1, -1 or -2
    rows = [([0.25, 0.0], 1), ([0.5 - E24, top], 1), ([top, top], 2), ([0.5, 0.0], 2), ([0.0, 0.0], 0),
            ([0.25 - E24, top], 0)]  # .25 - 2^-48: the reference's element 0 (module docstring)
    U = np.array([r + near3 for r, _ in rows], np.float32)
    want = [e for _, e in rows]
    # the reference on the CPU: MeshSampler.sample(uniforms=...); corner 3 of its element gives the point's z
    z = M.MeshSampler(TAB_V, TAB_T).sample(len(rows), uniforms=torch.as_tensor(U))[:, 2]
    assert [{1: 0, -1: 1, -2: 2}[int(round(float(v)))] for v in z] == want
    pts, elem = s.points_device(torch.as_tensor(U, device="cuda"), elements=True)
    assert elem.cpu().tolist() == want
    check_points(s, U, pts, elem)


@pytest.mark.parametrize("name", ["cube", "tri2", "tri3"])
def test_barycentric_edge_uniforms_stay_inside(S, name):
    s = S[name]
    m = s.uniforms_per_point()
    top = 1 - E24
    U = np.array([[0.0] * m, [0.3, 0.0] + [1e-3, top, 1e-3, top][:m - 2], [0.9, 0.5] + [top, 1e-3, top, 0.0][:m - 2]],
                 np.float32)
    pts, elem = s.points_device(torch.as_tensor(U, device="cuda"), elements=True)
    assert bool(torch.isfinite(pts).all())
    cor = s.corners.cpu().numpy().astype(np.float64)[elem.cpu().numpy()]
    assert float(bary_in(cor, pts.double().cpu().numpy()).min()) >= -1e-5
    check_points(s, U, pts, elem)


def test_single_element_mesh(S):
    s = M.MeshSampler(TAB_V, TAB_T[:1], device="cuda")
    assert s.cdf.cpu().tolist() == [1.0]
    U = np.random.default_rng(7).integers(0, 1 << 24, size=(300, 6)).astype(np.float32) * np.float32(E24)
    pts, elem = s.points_device(torch.as_tensor(U, device="cuda"), elements=True)
    assert int(elem.abs().max()) == 0
    check_points(s, U, pts, elem)


# ---- 2. insr_sample_mesh: the stream contract ------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("cube", 1), ("cube", 3), ("cube", 1000), ("tri2", 1), ("tri2", 3),
                                    ("tri3", 257), ("bunny", 65)])
def test_stream_equals_philox_restatement_and_box_twin(B, S, name, n):
    from base.sampling import _sampler, sample_boxes
    s, seed = S[name], 0x5EED0000 + n
    m = s.uniforms_per_point()
    groups = (n * m + 3) // 4
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(seed)
    pts, elem = s.sample_device(n, elements=True)
    state, key = _sampler(dev)
    assert key == seed  # rank 0: the torch seed itself
    assert int(state[0]) == groups and int(state[1]) == 0  # advanced by ceil(n m / 4); ticket reset
    U = stream_uniforms(seed, 0, n * m).reshape(n, m)
    check_points(s, U, pts, elem)
    # a following box draw continues the stream where it would have
    after = sample_boxes([(5, [0.0] * 3, [1.0] * 3)], 3)
    assert np.array_equal(after.cpu().numpy().reshape(-1), stream_uniforms(seed, groups, 15))
    # the twin: today's sharded _mesh_draw from the same seed consumes the same numbers
    torch.manual_seed(seed)
    d = 3 if m % 3 == 0 else 2
    u = sample_boxes([(n * m // d, (0.0,) * d, (1.0,) * d)], d)
    assert int(_sampler(dev)[0][0]) == groups
    assert np.array_equal(u.cpu().numpy().reshape(-1), U.reshape(-1))
    twin = s.sample(n, uniforms=u.view(n, m))
    assert float((pts - twin).abs().max()) <= bound(s)


# ---- 3. writes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "tri2"])
def test_only_the_requested_rows_are_written(B, S, name):
    from base.sampling import sample_mesh_into
    s = S[name]
    R, row0, n = 300, 7, 257
    buf = torch.full((R, s.corners.shape[2]), float("nan"), device="cuda")
    assert sample_mesh_into(buf, row0, n, s) is buf
    nan = torch.isnan(buf).all(dim=1).cpu()
    assert bool(nan[:row0].all()) and bool(nan[row0 + n:].all())
    assert bool(torch.isfinite(buf[row0:row0 + n]).all())
    with pytest.raises(ValueError):
        sample_mesh_into(buf, R - 3, 4, s)
    with pytest.raises(ValueError):
        sample_mesh_into(torch.empty(R, 5, device="cuda"), 0, 4, s)


def test_device_methods_refuse_the_cpu():
    from base._native import NativeUnavailable
    s = M.MeshSampler(CUBE_V, CUBE_T)
    with pytest.raises(NativeUnavailable):
        s.sample_device(4)
    with pytest.raises(NativeUnavailable):
        s.points_device(torch.zeros(4, 6))


# ---- 4. determinism and capture ----------------------------------------------------------------------------------
def test_same_seed_same_bits_and_graph_replay_draws_the_eager_sequence(B, S):
    s, n, seed = S["cube"], 1000, 77
    torch.manual_seed(seed)
    eager = [s.sample_device(n).clone() for _ in range(4)]
    torch.manual_seed(seed)
    assert torch.equal(s.sample_device(n), eager[0])  # launch 1 again, eager: the state exists before the capture
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            xg = s.sample_device(n)
    torch.cuda.synchronize()
    for k in (1, 2, 3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(xg, eager[k]), k


# ---- 5. containment and element fractions ----------------------------------------------------------------------
def test_bunny_points_lie_in_their_elements(B, S):
    s, n = S["bunny"], 4096
    torch.manual_seed(3)
    pts, elem = s.sample_device(n, elements=True)
    e = elem.cpu().numpy()
    assert e.min() >= 0 and e.max() < s.k and len(np.unique(e)) > n // 2
    cor = s.corners.cpu().numpy().astype(np.float64)[e]
    lam = bary_in(cor, pts.double().cpu().numpy())
    print(f"bunny: min barycentric {lam.min():.3e}")
    assert float(lam.min()) >= -1e-5


def test_element_fractions_follow_the_volumes(B, S):
    torch.manual_seed(11)
    _, elem = S["table"].sample_device(40000, elements=True)
    frac = np.bincount(elem.cpu().numpy(), minlength=3) / 40000.0
    print("fractions", frac)
    assert np.abs(frac - np.array([0.25, 0.25, 0.5])).max() <= 0.01  # 4.6 sigma, sigma = sqrt(.25 .75 / 40000)


# ---- 6. / 7. the model -------------------------------------------------------------------------------------------
def write_medit(path, V, T):
    with open(path, "w") as f:
        f.write("MeshVersionFormatted 1\nDimension 3\nVertices\n%d\n" % len(V))
        for v in V:
            f.write("%.17g %.17g %.17g 1\n" % tuple(v))
        f.write("Tetrahedra\n%d\n" % len(T))
        for t in T:
            f.write("%d %d %d %d 1\n" % tuple(t + 1))
        f.write("End\n")


R_CUBE = 2.0 / np.sqrt(3.0)  # the normalised cube (farthest vertex at 1) scaled by 2


def cube_model(B, tmp_path, **kw):
    from pde.config import make_config
    from pde.elasticity import ElasticityModel
    p = str(tmp_path / "cube.mesh")
    write_medit(p, CUBE_V, CUBE_T)
    args = dict(dim=3, use_mesh=True, mesh_path=p, sample_resolution=8, sample_pattern=["random", "uniform"],
                num_hidden_layers=1, hidden_features=32, energy=["arap", "kinematics", "external", "volume"],
                external_force_z=-1.0, proj_dir=str(tmp_path / "proj"), insr_progress=False, early_stop=False,
                insr_mesh_batch=True)
    args.update(kw)
    torch.manual_seed(0)
    model = ElasticityModel(make_config("elasticity", **args))
    model.timestep = 1
    calls = []
    orig = model._mesh_draw
    model._mesh_draw = lambda sampler, n: calls.append(n) or orig(sampler, n)
    return model, calls


def test_model_batch_layout_and_persistence(B, tmp_path):
    from pde.elasticity import ElasticityModel
    model, calls = cube_model(B, tmp_path)
    x = model._mesh_batch(8)
    assert x.shape == (8 ** 3 + 8, 3) and x.is_leaf and x.requires_grad and x.dtype == torch.float32
    assert float(x.detach().abs().max()) <= R_CUBE + 1e-5  # inside the normalised cube
    verts = torch.as_tensor(CUBE_V * R_CUBE, dtype=torch.float32)
    assert torch.allclose(x[-8:].detach().cpu(), verts, atol=1e-6)
    assert torch.equal(x[-8:].detach(), model.mesh_V)
    ptr, seen = x.data_ptr(), [x.detach()[:512].clone()]
    body = ElasticityModel._solve_deformation._insr_phase
    model._reset_optimizer()
    for _ in range(3):
        ld = body(model)
        assert np.isfinite(float(ld["main"].detach()))
        model._update_network(ld)
        (buf, _, _), = model.__dict__["_insr_mesh_batch"].values()
        assert buf is x and buf.data_ptr() == ptr
        assert torch.equal(buf[-8:].detach(), model.mesh_V)
        assert float(buf.detach().abs().max()) <= R_CUBE + 1e-5
        assert not any(torch.equal(buf.detach()[:512], a) for a in seen)  # fresh points every iteration
        seen.append(buf.detach()[:512].clone())
    assert calls == []


def test_model_energy_equals_the_oracle_on_the_drawn_points(B, tmp_path):
    from oracle import siren_oracle as O
    from pde.elasticity import ElasticityModel
    model, calls = cube_model(B, tmp_path)
    cfg = model.cfg
    body = ElasticityModel._solve_deformation._insr_phase
    model._reset_optimizer()
    ld = body(model)
    (buf, _, _), = model.__dict__["_insr_mesh_batch"].values()
    xs = buf.detach().clone()  # the points this iteration drew and evaluated
    ecfg = dict(dt=cfg.dt, energy=list(cfg.energy), ratio_arap=cfg.ratio_arap, ratio_volume=cfg.ratio_volume,
                ratio_kinematics=cfg.ratio_kinematics, ratio_constraint=cfg.ratio_constraint,
                ratio_collide=cfg.ratio_collide, plane_height=cfg.plane_height,
                external_force=[cfg.external_force_x, cfg.external_force_y, cfg.external_force_z],
                constraint_offset_right=[0.0, 0.0, 0.0], circle_center=[0.0, 0.0, 0.0], circle_radius=1.0,
                external_force_timesteps=cfg.external_force_timesteps)
    nets = []
    for net in (model.deformation_field, model.deformation_field_prev, model.deformation_field_prev_prev):
        o = O.OracleSiren(3, 3, 1, 32)
        with torch.no_grad():
            for po, pn in zip(o.parameters(), net.parameters()):
                po.copy_(pn.detach().cpu())
        nets.append(o)
    xr = xs.cpu().requires_grad_(True)
    ref = O.elasticity_loss(nets[0], nets[1], nets[2], xr, None, None, ecfg)["main"]
    print("energy", float(ld["main"]), "oracle", float(ref))
    assert abs(float(ld["main"]) - float(ref)) <= 1e-5 * abs(float(ref)) + 1e-6
    assert calls == []


def test_model_graph_loop_captures_the_draw(B, tmp_path):
    import warnings
    model, calls = cube_model(B, tmp_path, insr_graph=True, insr_graph_unroll=4, max_n_iters=6, insr_sync_every=1000)
    before = model.deformation_field.flat_params().detach().clone()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # a capture fallback warns: fail here instead
        model._solve_deformation()
    torch.cuda.synchronize()
    assert getattr(model, "_insr_capture_error", None) is None, model._insr_capture_error
    after = model.deformation_field.flat_params().detach()
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
    (buf, _, _), = model.__dict__["_insr_mesh_batch"].values()
    assert float(buf.detach().abs().max()) <= R_CUBE + 1e-5 and torch.equal(buf[-8:].detach(), model.mesh_V)
    assert calls == []


def test_model_shard_takes_its_rows_of_every_part(B, tmp_path):
    model, calls = cube_model(B, tmp_path, insr_shard=(1, 4))
    x = model._mesh_batch(8)
    assert model._rows(512) == (128, 128) and model._rows(8) == (2, 2)
    assert x.shape == (128 + 2, 3)
    assert torch.equal(x[-2:].detach(), model.mesh_V[2:4])
    assert float(x.detach().abs().max()) <= R_CUBE + 1e-5 and float(x.detach()[:128].std()) > 0.2
    assert calls == []


def test_model_2d_triangle_scene(B, tmp_path):
    from pde.config import make_config
    from pde.elasticity import ElasticityModel
    p = str(tmp_path / "square.obj")
    with open(p, "w") as f:
        f.write("v -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nf 1 2 3\nf 1 3 4\n")
    cfg = make_config("elasticity", dim=2, use_mesh=True, mesh_path=p, sample_resolution=8,
                      sample_pattern=["random", "uniform"], num_hidden_layers=1, hidden_features=32,
                      energy=["arap", "kinematics", "external", "volume"], external_force_y=-1.0,
                      proj_dir=str(tmp_path / "proj"), insr_progress=False, early_stop=False, insr_mesh_batch=True)
    torch.manual_seed(0)
    model = ElasticityModel(cfg)
    model.timestep = 1
    model._mesh_draw = None  # never called
    x = model._mesh_batch(8)
    assert x.shape == (8 ** 2 + 4, 2)
    r = 2.0 / np.sqrt(2.0)
    assert float(x.detach().abs().max()) <= r + 1e-5 and torch.equal(x[-4:].detach(), model.mesh_V[:, :2])
    model._reset_optimizer()
    ld = ElasticityModel._solve_deformation._insr_phase(model)
    assert np.isfinite(float(ld["main"].detach()))


def test_model_flag_off_draws_as_before(B, tmp_path):
    from pde.elasticity import ElasticityModel
    model, calls = cube_model(B, tmp_path, insr_mesh_batch=False)
    assert model._mesh_batch(8) is None
    model._reset_optimizer()
    ld = ElasticityModel._solve_deformation._insr_phase(model)
    assert np.isfinite(float(ld["main"].detach())) and calls == [512]
    assert "_insr_mesh_batch" not in model.__dict__
