"""The hyperelastic materials (stable Neo-Hookean, St. Venant-Kirchhoff) of the one-launch elasticity
energy (base.elastic_energy -> insr_elastic_energy), the stand-alone op (base.hyperelastic_energy ->
insr_hyperelastic_fwd / bwd) and ElasticityModel, against an fp64 torch restatement of the
formulas in their F = G + I form with torch.autograd.grad for the stress.

Tolerances, the rule of test_gpu_elastic.py: total within 1e-5 of the largest term; every term within
1e-5 of fp64 or within 3x the error of an fp32 torch evaluation (materials: the same from-G formula;
the other terms: the reference's expression); dE/df 1e-5 and dE/dJ 1e-5 normwise (no SVD, so not the
1e-4 the singular-value terms need).

The fp32 torch evaluation of the from-G form, measured on the CPU at exactly the inputs of
test_one_launch_matches_fp64 (d in {2, 3}, n in {5, 300, 3000} at s = 0.3, and s in {0.01, 1.5} at
n = 3000; mu = 20, lam = 1e3), relative to fp64:
  neohookean  total <= 1.6e-7, stress (normwise max) <= 1.8e-7
  stvk        total <= 8.6e-8, stress (normwise max) <= 1.7e-7
so the 1e-5 bounds leave a plain fp32 evaluation more than 50x headroom for both materials."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

MU, LAM = 20.0, 1e3
MATERIALS = ["neohookean", "stvk"]


@pytest.fixture(scope="module")
def B():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import base
    return base


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def psi(G, material, mu, lam):
    """Per-point energy density as the formulas are stated: F = G + I, I_C = |F|^2, J = det F (any dtype)."""
    d = G.shape[-1]
    F = G + torch.eye(d, dtype=G.dtype)
    if material == "neohookean":
        Ic, J = (F ** 2).sum((1, 2)), torch.linalg.det(F)
        alpha = 1.0 + (mu / lam) * d / (d + 1)
        psi0 = lam / 2 * (1.0 - alpha) ** 2 - mu / 2 * math.log(d + 1)
        return mu / 2 * (Ic - d) + lam / 2 * (J - alpha) ** 2 - mu / 2 * torch.log(Ic + 1) - psi0
    E = 0.5 * (F.transpose(1, 2) @ F - torch.eye(d, dtype=G.dtype))
    return mu * (E ** 2).sum((1, 2)) + lam / 2 * torch.einsum("nii->n", E) ** 2


def psi_from_G(G, material, mu, lam):
    """The same densities evaluated from G (u = I_C - d, J - 1 from the minors, log1p), in G's dtype:
    the fp32 torch yardstick of the 3x rule."""
    d = G.shape[-1]
    tr = torch.einsum("nii->n", G)
    if material == "neohookean":
        u = (G ** 2).sum((1, 2)) + 2 * tr
        if d == 2:
            jm1 = tr + (G[:, 0, 0] * G[:, 1, 1] - G[:, 0, 1] * G[:, 1, 0])
        else:
            minors = sum(G[:, i, i] * G[:, j, j] - G[:, i, j] * G[:, j, i] for i, j in ((0, 1), (0, 2), (1, 2)))
            jm1 = tr + minors + torch.linalg.det(G)
        c = d / (d + 1)
        return mu / 2 * u + lam / 2 * (jm1 * (jm1 - 2 * (mu / lam) * c)) - mu / 2 * torch.log1p(u / (d + 1))
    E = 0.5 * (G + G.transpose(1, 2) + G.transpose(1, 2) @ G)
    return mu * (E ** 2).sum((1, 2)) + lam / 2 * torch.einsum("nii->n", E) ** 2


def reference_terms(f, J, x, fp, fpp, n, rows_l, rows_r, cfg):
    """The energy terms on tensors of any dtype (the existing ones as test_gpu_elastic.py restates them)."""
    d, dt = x.shape[1], cfg["dt"]
    q = f[:n] + x
    q_prev, q_pp = fp + x, fpp + x
    qdot, qdot_prev = (q - q_prev) / dt, (q_prev - q_pp) / dt
    S = torch.linalg.svdvals(J[:n] + torch.eye(d, dtype=J.dtype))
    t = {"neohookean": torch.sum(psi(J[:n], "neohookean", cfg["mu"], cfg["lam"])),
         "stvk": torch.sum(psi(J[:n], "stvk", cfg["mu"], cfg["lam"])),
         "arap": cfg["ra"] * torch.sum((S - 1.0) ** 2),
         "volume": cfg["rv"] * torch.sum((torch.prod(S, dim=1) - 1) ** 2),
         "kinematics": cfg["rk"] * torch.sum((qdot - qdot_prev) ** 2),
         "external": -dt * torch.sum(qdot * torch.tensor(cfg["ext"][:d], dtype=x.dtype))}
    fl, fr = f[rows_l[0]:rows_l[0] + rows_l[1]], f[rows_r[0]:rows_r[0] + rows_r[1]]
    t["constraint"] = cfg["rc"] * torch.sum(fl ** 2)
    t["constraint_right"] = cfg["rc"] * torch.sum((fr - torch.tensor(cfg["offset"][:d], dtype=x.dtype)) ** 2)
    hit = (q[:, -1] < cfg["h"]).to(x.dtype)
    t["collision"] = -dt * torch.sum(qdot[:, -1] * cfg["rcol"] * (cfg["h"] - q[:, -1]) * hit)
    return t


def make_case(d, n, n_l, n_r, seed, s=0.3):
    """test_gpu_elastic.py's make_case with the Jacobian's scale s as a parameter (G = s randn)."""
    g = torch.Generator().manual_seed(seed)
    rows = n + n_l + n_r
    f = 0.3 * torch.randn(rows, d, generator=g)
    J = s * torch.randn(rows, d, d, generator=g)
    x = torch.rand(n, d, generator=g) * 2 - 1
    fp = f[:n] + 0.05 * torch.randn(n, d, generator=g)
    fpp = fp + 0.05 * torch.randn(n, d, generator=g)
    cfg = dict(dt=0.1, ra=20.0, rv=1e3, rk=10.0, rc=1e4, rcol=1e4, ext=(0.3, -2e2, -1e2), offset=(2.0, 0.5, -0.25),
               h=-0.4, mu=MU, lam=LAM)
    return f, J, x, fp, fpp, (n, n_l), (n + n_l, n_r), cfg


def run_case(B, d, energy, n, n_l, n_r, seed, s=0.3, ratios_over=None):
    """One launch against fp64: returns nothing, asserts the module's tolerances."""
    f, J, x, fp, fpp, rows_l, rows_r, cfg = make_case(d, n, n_l, n_r, seed, s)
    f64, J64 = f.double().requires_grad_(True), J.double().requires_grad_(True)
    terms = reference_terms(f64, J64, x.double(), fp.double(), fpp.double(), n, rows_l, rows_r, cfg)
    terms32 = reference_terms(f, J, x, fp, fpp, n, rows_l, rows_r, cfg)
    for m in MATERIALS:  # the yardstick of a material: the from-G form in fp32
        terms32[m] = torch.sum(psi_from_G(J[:n], m, MU, LAM))
    total64 = 0
    for e in energy:
        total64 = total64 + terms[e]
    gf64, gJ64 = torch.autograd.grad(total64, (f64, J64), allow_unused=True)
    fg, Jg = f.cuda().requires_grad_(True), J.cuda().requires_grad_(True)
    ratios = {"arap": cfg["ra"], "volume": cfg["rv"], "kinematics": cfg["rk"], "constraint": cfg["rc"],
              "constraint_right": cfg["rc"], "collision": cfg["rcol"]}
    total, per = B.elastic_energy(fg, Jg, x.cuda(), fp.cuda(), fpp.cuda(), n=n, dt=cfg["dt"], energy=energy,
                                  ratios=ratios, ext=cfg["ext"][:d], rows_l=rows_l, rows_r=rows_r,
                                  target=cfg["offset"][:d], plane_height=cfg["h"], mu=MU, lam=LAM)
    assert per.shape == (10,)
    scale = max(abs(float(terms[e])) for e in energy)
    print(f"d={d} n={n} s={s} {energy}: total {float(total):.9g} fp64 {float(total64):.9g} "
          f"err/scale {abs(float(total) - float(total64)) / scale:.2e}")
    assert abs(float(total) - float(total64)) <= 1e-5 * scale, (float(total), float(total64))
    ids = B._native.EL_IDS
    for e in energy:
        err32 = abs(float(terms32[e]) - float(terms[e]))
        tol = max(1e-5 * max(abs(float(terms[e])), 1e-6 * scale), 3 * err32)
        print(f"  {e}: {float(per[ids[e]]):.9g} fp64 {float(terms[e]):.9g} err32 {err32:.2e}")
        assert abs(float(per[ids[e]]) - float(terms[e])) <= tol, (e, float(per[ids[e]]), float(terms[e]), err32)
    for name, t in ids.items():  # the slots of the terms that are off hold 0
        if name not in energy:
            assert float(per[t]) == 0.0, name
    seed1 = B.losses.register_unit_seed(torch.ones((), device="cuda"))
    gf, gJ = torch.autograd.grad(total, (fg, Jg), grad_outputs=seed1, retain_graph=True)
    print(f"  dE/df rel {rel(gf, gf64):.2e} dE/dJ rel {rel(gJ, gJ64):.2e}")
    # with a singular-value term in the list dE/dJ carries that term's 1e-4 (test_gpu_elastic.py), else 1e-5
    tol_J = 1e-4 if ("arap" in energy or "volume" in energy) else 1e-5
    assert rel(gf, gf64) < 1e-5
    assert rel(gJ, gJ64) < tol_J
    assert float(gJ[n:].abs().sum()) == 0.0 and gJ.shape == J.shape
    gf2, gJ2 = torch.autograd.grad(total * 3.0, (fg, Jg))  # a non-unit seed scales them
    assert rel(gf2 / 3.0, gf64) < 1e-5 and rel(gJ2 / 3.0, gJ64) < tol_J


@pytest.mark.parametrize("n,s", [(5, 0.3), (300, 0.3), (3000, 0.3), (3000, 0.01), (3000, 1.5)])
@pytest.mark.parametrize("material", MATERIALS)
@pytest.mark.parametrize("d", [2, 3])
def test_one_launch_matches_fp64(B, d, material, n, s):
    """One partial wave, two blocks through the ticket, twelve blocks; at n = 3000 also near rest (s = 0.01) and
    s = 1.5, where 40-48 % of the rows are inverted (0.2-0.3 % at s = 0.3)."""
    run_case(B, d, [material, "kinematics", "external"], n, 0, 0, 10 * n + d, s)


@pytest.mark.parametrize("d,energy", [(3, ["neohookean", "kinematics", "collision", "external"]),
                                      (2, ["arap", "stvk", "constraint", "constraint_right", "volume"])])
def test_mixed_lists(B, d, energy):
    """A material next to the existing terms: the total is the fp64 sum in list order, every term sits in its slot
    (10 of them), and with the singular-value terms the stress adds to their dE/dJ."""
    run_case(B, d, energy, 3000, 40, 40, 30000 + d)


@pytest.mark.parametrize("d", [2, 3])
def test_rest_state_is_exactly_zero(B, d):
    """G = 0: value and dE/dJ exactly 0.0 for both materials (allocator blocks dirtied with NaN first)."""
    n = 3000
    z = torch.zeros(n, d, device="cuda")
    for material in MATERIALS:
        torch.empty(8 << 20, device="cuda").fill_(float("nan"))
        G = torch.zeros(n, d, d, device="cuda", requires_grad=True)
        total, per = B.elastic_energy(z, G, z, z, z, n=n, dt=0.1, energy=[material], ratios={}, mu=MU, lam=LAM)
        seed = B.losses.register_unit_seed(torch.ones((), device="cuda"))
        gJ, = torch.autograd.grad(total, (G,), grad_outputs=seed)
        assert float(total) == 0.0 and float(per.abs().sum()) == 0.0, material
        assert float(gJ.abs().sum()) == 0.0, material
        F = torch.eye(d, device="cuda").expand(n, d, d).contiguous().requires_grad_(True)
        e = B.hyperelastic_energy(F, material, MU, LAM)
        gF, = torch.autograd.grad(e, (F,))
        assert float(e) == 0.0 and float(gF.abs().sum()) == 0.0, material


def test_material_listed_with_weight_off_gives_zero_jacobian_gradient(B):
    f, J, x, fp, fpp, _, _, _ = make_case(3, 3000, 0, 0, 78)
    fg, Jg = f.cuda().requires_grad_(True), J.cuda().requires_grad_(True)
    torch.empty(8 << 20, device="cuda").fill_(float("nan"))  # dirty the caching allocator's blocks
    total, per = B.elastic_energy(fg, Jg, x.cuda(), fp.cuda(), fpp.cuda(), n=3000, dt=0.1,
                                  energy=["neohookean", "stvk", "kinematics"],
                                  ratios={"neohookean": 0.0, "stvk": 0.0, "kinematics": 2.0}, mu=MU, lam=LAM)
    seed = B.losses.register_unit_seed(torch.ones((), device="cuda"))
    gf, gJ = torch.autograd.grad(total, (fg, Jg), grad_outputs=seed)
    assert float(gJ.abs().sum()) == 0.0 and torch.isfinite(gf).all()
    assert float(per[8]) == 0.0 and float(per[9]) == 0.0 and float(total) == float(per[2])


def test_grid_stride_path(B):
    """262,144 + 257 interior rows at d = 2: one more pass than kElMaxBlocks x kElThreads rows cover."""
    run_case(B, 2, ["neohookean", "kinematics"], 262144 + 257, 0, 0, 5)


def exact_case(d, n, seed, s=0.3):
    """G on a 2^-20 grid, so that F = G + I and F - I are exact in fp32: both ops see the same rows."""
    G = s * torch.randn(n, d, d, generator=torch.Generator().manual_seed(seed))
    G = torch.round(G.clamp(-7.0, 7.0) * 2.0 ** 20) / 2.0 ** 20
    F = G + torch.eye(d)
    assert torch.equal(F - torch.eye(d), G)
    return G, F


@pytest.mark.parametrize("n", [5, 3000])
@pytest.mark.parametrize("material", MATERIALS)
@pytest.mark.parametrize("d", [2, 3])
def test_standalone_op(B, d, material, n):
    G, F = exact_case(d, n, 100 * n + d)
    G64 = G.double().requires_grad_(True)
    e64 = psi(G64, material, MU, LAM).sum()
    g64, = torch.autograd.grad(e64, (G64,))
    Fg = F.cuda().requires_grad_(True)
    e = B.hyperelastic_energy(Fg, material, MU, LAM)
    gF, = torch.autograd.grad(e, (Fg,), retain_graph=True)
    print(f"d={d} {material} n={n}: {float(e):.9g} fp64 {float(e64):.9g} grad rel {rel(gF, g64):.2e}")
    assert abs(float(e) - float(e64)) <= 1e-5 * abs(float(e64))
    assert rel(gF, g64) < 1e-5
    gF3, = torch.autograd.grad(e * 3.0, (Fg,))
    assert rel(gF3 / 3.0, g64) < 1e-5
    # the one-launch term on the same rows: another reduction shape only
    z = torch.zeros(n, d, device="cuda")
    Gg = G.cuda().requires_grad_(True)
    total, _ = B.elastic_energy(z, Gg, z, z, z, n=n, dt=0.1, energy=[material], ratios={}, mu=MU, lam=LAM)
    seed = B.losses.register_unit_seed(torch.ones((), device="cuda"))
    gG, = torch.autograd.grad(total, (Gg,), grad_outputs=seed)
    assert abs(float(e) - float(total)) <= 1e-6 * abs(float(total))
    assert rel(gF, gG) < 1e-6
    # count < N: the rows past count add nothing and get zero gradient
    m = n - 2
    Fc = F.cuda().requires_grad_(True)
    torch.empty(8 << 20, device="cuda").fill_(float("nan"))
    ec = B.hyperelastic_energy(Fc, material, MU, LAM, count=m)
    gc, = torch.autograd.grad(ec, (Fc,))
    e64c = psi(G[:m].double(), material, MU, LAM).sum()
    assert abs(float(ec) - float(e64c)) <= 1e-5 * abs(float(e64c))
    assert float(gc[m:].abs().sum()) == 0.0 and rel(gc[:m], g64[:m]) < 1e-5


def model_cfg(dim, **kw):
    from pde.config import baseline_config
    extra = dict(dim=3, sample_resolution=8) if dim == 3 else dict(sample_resolution=20)
    return baseline_config("elasticity2Dstretch", proj_dir="/tmp/insr_test", insr_progress=False, num_hidden_layers=2,
                           hidden_features=64, energy=["neohookean", "constraint", "constraint_right"],
                           insr_lame_mu=1.0, insr_lame_lambda=10.0, **extra, **kw)


@pytest.mark.parametrize("dim", [2, 3])
def test_model_energy_and_graph(B, dim):
    """ElasticityModel with a material in cfg.energy: energy_of on a drawn batch is the fp64 formula on the
    Jacobian jet's output and the field rows, and two graph-captured iterations end bit for bit where two eager
    iterations from the same seed end (the _box_batch path)."""
    from base.diff_ops import jacobian_only
    from pde.elasticity import ElasticityModel
    cfg = model_cfg(dim)
    torch.manual_seed(0)
    m = ElasticityModel(cfg)
    m.timestep = 1
    res = cfg.sample_resolution
    xa, x, fl, fr = m._box_batch(res)
    n, nl = x.shape[0], fl.shape[0]
    assert n == 2 * res ** dim and nl == fr.shape[0] == res + res ** (dim - 1)
    e = m.energy_of(x, fl, fr, xa=xa)
    fa = m.deformation_field(xa)
    J = jacobian_only(fa, xa)
    assert J.shape == (n + 2 * nl, dim, dim)
    f64 = fa.detach().double().cpu()
    off = torch.tensor([cfg.constraint_right_offset_x, cfg.constraint_right_offset_y,
                        cfg.constraint_right_offset_z][:dim], dtype=torch.float64)
    e64 = psi(J[:n].detach().double().cpu(), "neohookean", 1.0, 10.0).sum() + \
        cfg.ratio_constraint * (f64[n:n + nl] ** 2).sum() + cfg.ratio_constraint * ((f64[n + nl:] - off) ** 2).sum()
    print(f"dim={dim}: energy_of {float(e):.9g} fp64 {float(e64):.9g}")
    assert abs(float(e) - float(e64)) <= 1e-5 * abs(float(e64))
    out = {}
    for graph in (False, True):
        torch.manual_seed(0)
        mg = ElasticityModel(model_cfg(dim, max_n_iters=2, early_stop=False, insr_graph=graph, insr_sync_every=1000))
        mg.timestep = 1
        mg._solve_deformation()
        torch.cuda.synchronize()
        if graph:
            assert getattr(mg, "_insr_capture_error", None) is None, mg._insr_capture_error
        out[graph] = mg.deformation_field.flat_params().detach().clone()
    assert bool(torch.isfinite(out[True]).all()) and torch.equal(out[True], out[False])
