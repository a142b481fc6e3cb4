"""pbf_anisotropy_compute on a GPU: against the float64 all-pairs restatement (tests/anisotropy_ref.py), the closed forms
through the library, the shapes where the kernels can go wrong, equal bytes under every gather setting and for a subset of
the outputs, that the call observes without changing anything a step does, its refusals, the benchmark flag and the C++ shim.

Bars (u = eps_N / 2 + eps_64 / 2).  Both sides start from the same bits: pStar, types and keys are read back.
neighbours: between the reference's counts at thresholds h (1 - 16 eps_N) and h (1 + 16 eps_N).
centre: one weight w = 1 - q q q, q = r / h: r carries 3.5 u (tests/test_sample_gpu.py), q one more, q^3 three times that and
  two products, the subtraction one: |delta w| <= 17 u, absolute (w <= 1).  A term w d_a of M: d_a carries u, the product u:
  <= 19 u |d_a|.  Summing k terms: (k - 1) u sum|term|.  Hence  delta M_a <= 19 u cap_a + (k + 1) u abs_a  with cap_a = sum |d_a|
  and abs_a = sum |w d_a| over the candidates, and delta S <= 17 u k + k u S.  mu = M / S, centre = (p + s mu) scale:
      bar_a = scale (s (delta M_a / S + |mu_a| (delta S / S + 2 u)) + 2 u |p_a|) + 2 u |centre_a|
  — the shape (k + c) u sum|term| / S of tests/test_sample_gpu.py.  Every quantity comes from the reference.
G: compared as a matrix (Frobenius norm), never as eigenvectors.  bar = c u k_r A_i |G_i|, A_i = tr(Q / S) / (h^2 sigma_1).
  c could not be derived from the rounding counts (the eigen-solver's share has no closed count), so it is MEASURED ON THE
  CPU: the error of a float32 numpy evaluation of the reference against its float64 one on the oracle's states of the five
  scenes, over u_32 k_r A_i |G_i|, its maximum over the particles that are not excluded, times 4 for the summation order
  (g_constant() below; measured 19.2, on `sparse`; 12.1 on the other four -> c = 76.9).  It is never fitted to the device.
  Excluded from the G bar (tests/test_anisotropy_cpu.py caps them at 2 % of the fluid): A_i > 64, or a candidate within
  16 eps_float32 h of h — nothing else.  (A neighbour count that differs from the reference's needs a candidate between the
  two thresholds above, which lies in that window.)  They are still held to: finite values; |axes axes^T - I|_F and |det - 1|
  at the solver's bar — the very bar host/test_aniso_eig is held to, four times what numpy.linalg.eigh leaves on that
  program's 10^5 matrices in the same precision (test_anisotropy_cpu.solver_bars(): about 4.3 eps in float32, 48 eps in
  float64; |det - 1| <= |A A^T - I|_F to first order, det^2 being det(A A^T)); radii[2] >= radii[0] / k_r;
  G == axes^T diag(1 / (h radii)) axes at the G bar.
With PBF_FLAG_FAST_MATH: the project's 3e-5 of the batch maximum, for centre (relative to the largest |centre|), G and the
  frame (its largest entry is 1).
Branches: tests/test_anisotropy_cpu.py shows on the oracle's states which scene fills which branch to 10 % of the fluid under
  each setting of min_neighbours; the same is asserted here on the device's states (BRANCHES)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import anisotropy_ref as AR
from anisotropy_scenes import oracle_state, scene
from test_anisotropy_cpu import solver_bars
from test_sample_cpu import STRAYS_MAX_X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 0.1
VARIANTS = [(True, False), (False, False), (False, True)]   # (fp64, PBF_FLAG_FAST_MATH)
IDS = ["fp64", "fp32", "fp32-fast"]
SCENES = ["cubes1024", "cloud", "obstacles", "sparse", "strays"]
# (scene, min_neighbours) -> the branches that hold at least 10 % of the fluid there: with 25 the anisotropic one only in
# `cloud`, with 8 the isotropic one only in `sparse`
BRANCHES = {(name, m): {"isotropic"} if m == 25 else {"anisotropic"} for name in SCENES for m in (25, 8)}
BRANCHES["cloud", 25] = BRANCHES["sparse", 8] = {"isotropic", "anisotropic"}
ERR_INVALID, ERR_STATE = -1, -4
AMP_CAP = 64.0
EDGE_REL = 16 * float(np.finfo(np.float32).eps)            # (times the h of the state)
K_R = 4.0
NAMES = ["centre", "G", "axes", "radii", "neighbours"]

_G_CONSTANT = []


def g_constant():
    """c of the G bar, measured on the CPU (module text): float32 against float64 numpy, the oracle's states, times 4"""
    if not _G_CONSTANT:
        u32, worst = float(np.finfo(np.float32).eps) / 2, 0.0
        for name in SCENES:
            st = oracle_state(name)
            kw = dict(pos_world=st["down"]["pos"], cells=AR.predict_cells_from_keys(st["keys"]), min_neighbours=8, k_r=K_R)
            a = AR.anisotropy(st["pstar"], st["down"]["type"] == 1, H, st["scale"], **kw)
            b = AR.anisotropy(st["pstar"], st["down"]["type"] == 1, H, st["scale"], dtype=np.float32, **kw)
            ok = (st["down"]["type"] == 0) & (a["amp"] <= AMP_CAP) & (a["edge"] > EDGE_REL * H)
            norm = np.sqrt((a["G"] ** 2).sum((1, 2)))
            err = np.sqrt(((b["G"].astype(np.float64) - a["G"]) ** 2).sum((1, 2)))
            worst = max(worst, float((err[ok] / (u32 * K_R * a["amp"][ok] * norm[ok])).max()))
        print("G bar: measured float32-against-float64 constant", worst, "-> c =", 4 * worst)
        _G_CONSTANT.append(4 * worst)
    return _G_CONSTANT[0]


def solver(pkg, sc, fp64, fast=False, **options):
    s = pkg.Solver(h=H, fp64=fp64, flags=pkg.FLAG_FAST_MATH if fast else 0)
    for k, v in options.items():
        s.set_option(k, v)
    return s.upload(**sc)


_STEPPED = {}


def stepped(pkg, name, fp64, fast):
    """the scene after 3 steps (K = 2) ("strays": `obstacles`, one step in a box that ends at x = 130) and its read-back
    state — made once per (scene, variant) and left unchanged"""
    key = (name, fp64, fast)
    if key not in _STEPPED:
        p = pkg.default_params(2, 1000.0)
        if name == "strays":
            p.max_bound[0] = STRAYS_MAX_X
            s = solver(pkg, scene("obstacles"), fp64, fast).steps(p, 1)
        else:
            s = solver(pkg, scene(name), fp64, fast).steps(p, 3)
        dt = np.float64 if fp64 else np.float32
        st = dict(down=s.download(), pstar=s.pstar().astype(np.float64), cells=AR.predict_cells_from_keys(s.keys()),
                  h=float(dt(H)), scale=p.scale, dtype=dt)
        _STEPPED[key] = (s, p, st, {})
    return _STEPPED[key]


def reference(st, cache, min_neighbours, k):
    """the reference at threshold h (1 + k 16 eps_N), cached per state"""
    if (min_neighbours, k) not in cache:
        delta = 16 * float(np.finfo(st["dtype"]).eps)
        cache[(min_neighbours, k)] = AR.anisotropy(st["pstar"], st["down"]["type"] == 1, st["h"], st["scale"],
                                                   pos_world=st["down"]["pos"], cells=st["cells"], k_r=K_R,
                                                   min_neighbours=min_neighbours, threshold=st["h"] * (1 + k * delta))
    return cache[(min_neighbours, k)]


def check_against(got, st, cache, min_neighbours, fp64, fast, label, cap=True):
    N = st["dtype"]
    eps = float(np.finfo(N).eps)
    u = eps / 2 + float(np.finfo(np.float64).eps) / 2
    lo, mid, hi = (reference(st, cache, min_neighbours, k) for k in (-1, 0, 1))
    fluid = st["down"]["type"] == 0
    nb = got["neighbours"].astype(np.int64)
    assert np.all(lo["neighbours"] <= nb) and np.all(nb <= hi["neighbours"])
    # obstacles: the stored position and zeros
    assert np.array_equal(got["centre"][~fluid], st["down"]["pos"][~fluid])
    for name in ("G", "axes", "radii", "neighbours"):
        assert not got[name][~fluid].any(), name
    for name in NAMES:
        assert np.isfinite(got[name]).all(), name
    # centre
    c = got["centre"].astype(np.float64)
    err = np.abs(c - mid["centre"])[fluid]
    S, k = hi["S"][fluid, None], hi["k"][fluid, None]
    dM = 19 * u * hi["cap_m"][fluid] + (k + 1) * u * hi["abs_m"][fluid]
    dS = 17 * u * k + k * u * S
    mu = np.abs(mid["centre"][fluid] / st["scale"] - st["pstar"][fluid, :3]) / 0.9
    bar = st["scale"] * (0.9 * (dM / S + mu * (dS / S + 2 * u)) + 2 * u * np.abs(st["pstar"][fluid, :3])) + 2 * u * np.abs(mid["centre"][fluid])
    if fast:
        bar = np.full_like(err, 3e-5 * np.abs(mid["centre"]).max())
    print(label, "centre: max error", err.max(), "largest bar", bar.max(), "worst error / bar", (err / bar).max())
    assert np.all(err <= bar)
    # G as a matrix
    G = AR.full3(got["G"])
    norm = np.sqrt((mid["G"] ** 2).sum((1, 2)))
    gerr = np.sqrt(((G - mid["G"]) ** 2).sum((1, 2)))
    gbar = g_constant() * u * K_R * np.where(np.isfinite(mid["amp"]), mid["amp"], 0.0) * norm
    if fast:
        gbar = np.full_like(gerr, 3e-5 * norm.max())
    excluded = fluid & ((mid["amp"] > AMP_CAP) | (mid["edge"] <= EDGE_REL * st["h"]))
    held = fluid & ~excluded
    print(label, "G: excluded", int(excluded.sum()), "of", int(fluid.sum()), "max error", gerr[held].max(), "worst error / bar",
          (gerr[held] / gbar[held]).max(), "anisotropic branch", int(mid["enough"][fluid].sum()))
    assert not cap or excluded.sum() <= 0.02 * fluid.sum()      # (the cap belongs to the scenes; a hand-made shape may hold loners)
    assert np.all(gerr[held] <= gbar[held])
    # every fluid particle, the excluded ones included: a right-handed orthonormal frame, clamped radii, G made of them
    ax, rad = got["axes"].astype(np.float64)[fluid], got["radii"].astype(np.float64)[fluid]
    orth = np.sqrt(((np.einsum("nka,nla->nkl", ax, ax) - np.eye(3)) ** 2).sum((1, 2)))
    solver_bar = 3e-5 if fast else solver_bars()["double" if N is np.float64 else "float"][1] * eps
    det = np.abs(np.linalg.det(ax) - 1)
    print(label, "axes: max |A A^T - I|", orth.max(), "max |det - 1|", det.max(), "bar", solver_bar, "in eps_N:", orth.max() / eps,
          det.max() / eps, solver_bar / eps)
    assert orth.max() <= solver_bar and det.max() <= solver_bar
    assert np.all(rad[:, 0] >= rad[:, 1]) and np.all(rad[:, 1] >= rad[:, 2]) and np.all(rad[:, 2] >= rad[:, 0] / K_R * (1 - 4 * eps))
    made = np.einsum("nka,nk,nkb->nab", ax, 1.0 / (st["h"] * rad), ax)
    own = np.sqrt(((G[fluid] - made) ** 2).sum((1, 2)))
    own_bar = np.maximum(gbar[fluid], 16 * u * np.sqrt((made ** 2).sum((1, 2))))   # (the stated formula's own roundings)
    assert np.all(own <= own_bar)
    return mid


# ---- 1. against the reference -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", SCENES)
def test_against_the_all_pairs_reference(pkg, name, fp64, fast):
    s, p, st, cache = stepped(pkg, name, fp64, fast)
    for min_neighbours in (25, 8):
        got = s.anisotropy(p, k_r=K_R, min_neighbours=min_neighbours)
        mid = check_against(got, st, cache, min_neighbours, fp64, fast, f"{name} min_neighbours={min_neighbours}")
        fluid = st["down"]["type"] == 0
        share = float(mid["enough"][fluid].mean())
        print(name, min_neighbours, "share of the fluid in the anisotropic branch:", share)
        assert share >= (0.10 if "anisotropic" in BRANCHES[name, min_neighbours] else 0.0)
        assert 1 - share >= (0.10 if "isotropic" in BRANCHES[name, min_neighbours] else 0.0)


# ---- 2. closed forms through the library ------------------------------------------------------------------------------

def at_rest(pkg, ps_solver, fp64, fast, obstacle=None, **options):
    """particles at rest at these solver-frame positions, zero force, iteration = 0: pStar is the uploaded lattice"""
    ps = np.asarray(ps_solver, np.float64)
    n = len(ps)
    sc = dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8) if obstacle is None else np.asarray(obstacle, np.uint8),
              mass=np.ones(n), pos=ps * 500.0, vel=np.zeros((n, 3)), colour=np.zeros((n, 4)))
    p = pkg.default_params(0, 1000.0)
    p.constant_force[:] = [0.0, 0.0, 0.0]
    s = solver(pkg, sc, fp64, fast, **options).step(p)
    return s, p


def interior(s, target_world):
    pos = s.download()["pos"].astype(np.float64)
    return int(np.argmin(((pos - np.asarray(target_world)) ** 2).sum(1)))


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_closed_forms_through_the_library(pkg, fp64, fast):
    tol = 1e-10 if fp64 else 2e-4
    g = 0.3 + np.arange(12) * (H / 2)
    ps = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    s, p = at_rest(pkg, ps, fp64, fast)
    got = s.anisotropy(p, k_r=K_R, min_neighbours=8)
    i = interior(s, (0.3 + 5 * H / 2,) * 3 * np.array(500.0))
    r = got["radii"][i].astype(np.float64)
    assert got["neighbours"][i] > 8 and r[0] - r[2] <= tol * r[0]
    G = AR.full3(got["G"][i:i + 1])[0]
    assert np.abs(G - np.eye(3) * G[0, 0]).max() <= tol * G[0, 0] * K_R

    g = 0.3 + np.arange(32) * (H / 4)
    ps = np.stack(np.meshgrid(g, g, [0.5], indexing="ij"), -1).reshape(-1, 3)
    s, p = at_rest(pkg, ps, fp64, fast)
    got = s.anisotropy(p, k_r=K_R, min_neighbours=8)
    i = interior(s, np.array([0.3 + 16 * H / 4, 0.3 + 16 * H / 4, 0.5]) * 500.0)
    assert got["neighbours"][i] > 8 and got["radii"][i][2] / got["radii"][i][0] == 0.25
    assert abs(abs(got["axes"][i][2][2]) - 1.0) <= tol and np.abs(got["axes"][i][2][:2]).max() <= tol ** 0.5

    ps = np.zeros((64, 3)) + [0.4, 0.3, 0.5]
    ps[:, 1] += np.arange(64) * (H / 8)
    s, p = at_rest(pkg, ps, fp64, fast)
    got = s.anisotropy(p, k_r=K_R, min_neighbours=8)
    i = interior(s, np.array([0.4, 0.3 + 32 * H / 8, 0.5]) * 500.0)
    assert got["neighbours"][i] > 8 and got["radii"][i][1] == got["radii"][i][2] and got["radii"][i][0] == 4 * got["radii"][i][1]
    assert abs(abs(got["axes"][i][0][1]) - 1.0) <= tol


# ---- 3. shapes, settings, subsets -------------------------------------------------------------------------------------

def same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_shapes_where_the_kernels_can_go_wrong(pkg, fp64, fast):
    rng = np.random.default_rng(7)
    # n = 1: alone, the isotropic record
    s, p = at_rest(pkg, [[0.5, 0.5, 0.5]], fp64, fast)
    got = s.anisotropy(p, k_n=0.5)
    assert got["neighbours"][0] == 0 and np.array_equal(got["radii"][0], [0.5] * 3) and np.array_equal(got["axes"][0], np.eye(3))
    assert np.array_equal(got["centre"][0], s.download()["pos"][0])
    # n = 65 (one wave and a lane), and a pile of 300 within h: lists beyond 160 go into the cell walk
    for n, spread in ((65, 0.3), (300, 0.045)):
        ps = 0.5 + rng.random((n, 3)) * spread
        runs = []
        for gather in (1, 0):
            s, p = at_rest(pkg, ps, fp64, fast, gather=gather)
            runs.append(s.anisotropy(p, k_r=K_R, min_neighbours=8))
        assert same(runs[0], runs[1]), n
        dt = np.float64 if fp64 else np.float32
        st = dict(down=s.download(), pstar=s.pstar().astype(np.float64), cells=AR.predict_cells_from_keys(s.keys()),
                  h=float(dt(H)), scale=p.scale, dtype=dt)
        if n == 300:
            assert runs[0]["neighbours"].max() > 160
        check_against(runs[0], st, {}, 8, fp64, fast, f"n={n}", cap=False)
    # all obstacles
    ps = 0.5 + rng.random((70, 3)) * 0.2
    s, p = at_rest(pkg, ps, fp64, fast, obstacle=np.ones(70, np.uint8))
    got = s.anisotropy(p)
    assert np.array_equal(got["centre"], s.download()["pos"]) and not any(got[k].any() for k in NAMES[1:])


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_the_same_bytes_under_every_gather_setting_and_for_subsets(pkg, fp64, fast):
    p = pkg.default_params(2, 1000.0)
    base = None
    for gather in (1, 0):
        for row_major in (1, 0):
            s = solver(pkg, scene("obstacles"), fp64, fast, gather=gather, row_major=row_major).steps(p, 3)
            got = s.anisotropy(p, k_r=K_R, min_neighbours=8)
            base = base or got
            assert same(base, got), (gather, row_major)
    for only in (["G"], ["centre", "neighbours"], ["axes", "radii"], []):
        part = s.anisotropy(p, k_r=K_R, min_neighbours=8, only=only)
        assert list(part) == only and all(np.array_equal(part[k], base[k]) for k in only)


# ---- 4. an observer ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_the_call_changes_nothing_a_step_or_another_observer_sees(pkg, fp64, fast):
    p = pkg.default_params(2, 1000.0)
    a, b = (solver(pkg, scene("obstacles"), fp64, fast).set_surface_tension(0.5, 0.2).steps(p, 2) for _ in range(2))
    for s in (a, b):
        s.diagnostics(p, density=True)
        s.whitewater_configure(capacity=1000, tau_ta=(0, 1), tau_wc=(0, 1), tau_k=(0, 1))
        s.whitewater_step(p)
    before = (a.surface_state(), a.density(), a.whitewater_potentials())
    a.anisotropy(p)
    after = (a.surface_state(), a.density(), a.whitewater_potentials())
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    a.step(p), b.step(p)
    da, db = a.download(), b.download()
    assert all(np.array_equal(da[k], db[k]) for k in da) and np.array_equal(a.pstar(), b.pstar())


# ---- 5. refusals ------------------------------------------------------------------------------------------------------

GUARD = 0xAB


def raw_call(pkg, s, p, cfg, n):
    bufs = {k: np.full(m * n * (4 if k == "neighbours" else np.dtype(s.dtype).itemsize), GUARD, np.uint8)
            for k, m in (("centre", 3), ("G", 6), ("axes", 9), ("radii", 3), ("neighbours", 1))}
    out = pkg.AnisotropyOut(*[bufs[k].ctypes.data for k in NAMES])
    rc = pkg.lib().pbf_anisotropy_compute(s.ctx, None if p is None else C.byref(p), None if cfg is None else C.byref(cfg), C.byref(out))
    return rc, all((b == GUARD).all() for b in bufs.values())


def test_refusals(pkg):
    L = pkg.lib()
    p = pkg.default_params(2, 1000.0)
    good = pkg.Anisotropy(0.9, 4.0, 20 / 3, 0.5, 25)
    s = solver(pkg, scene("cubes1024"), False)
    n = s.n
    assert raw_call(pkg, s, p, good, n) == (ERR_STATE, True)                       # before any step
    s.steps(p, 2)
    rc, untouched = raw_call(pkg, s, p, good, n)
    assert rc == 0 and not untouched
    assert raw_call(pkg, s, None, good, n) == (ERR_INVALID, True) and raw_call(pkg, s, p, None, n) == (ERR_INVALID, True)
    assert L.pbf_anisotropy_compute(s.ctx, C.byref(p), C.byref(good), None) == ERR_INVALID
    inf, nan = float("inf"), float("nan")
    for bad in ((-0.1, 4, 6, 0.5), (1.1, 4, 6, 0.5), (nan, 4, 6, 0.5), (0.9, 0.99, 6, 0.5), (0.9, nan, 6, 0.5), (0.9, inf, 6, 0.5),
                (0.9, 4, 0, 0.5), (0.9, 4, -1, 0.5), (0.9, 4, inf, 0.5), (0.9, 4, nan, 0.5), (0.9, 4, 6, 0), (0.9, 4, 6, -2),
                (0.9, 4, 6, inf), (0.9, 4, 6, nan)):
        assert raw_call(pkg, s, p, pkg.Anisotropy(*bad, 25), n) == (ERR_INVALID, True), bad
    foreign = pkg.default_params(2, 1000.0)
    foreign.max_bound[0] = 700.0
    assert raw_call(pkg, s, foreign, good, n) == (ERR_STATE, True)                 # params of another grid
    assert raw_call(pkg, s, p, good, n)[0] == 0                                    # (and the table survived the refusal)
    s.upload(**scene("cubes1024"))
    assert raw_call(pkg, s, p, good, n) == (ERR_STATE, True)                       # after pbf_upload
    t = solver(pkg, scene("cubes1024"), False).steps(p, 1)
    cut = pkg.SlabCut(0, 12, 0, 0)
    assert L.pbf_slab_configure(t.ctx, C.byref(cut), 0, 0) == 0
    assert raw_call(pkg, t, p, good, n) == (ERR_STATE, True)                       # a slab-configured ctx
    e = pkg.Solver(h=H)
    assert raw_call(pkg, e, p, good, 1) == (0, True)                               # empty state: PBF_OK, nothing written


# ---- 6. shim and CLI --------------------------------------------------------------------------------------------------

def test_shim(pkg):
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_aniso_shim")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr


def test_cli_writes_ellipsoids_beside_an_unchanged_cloud(pkg, tmp_path):
    BIN = os.path.join(ROOT, "pbf-sph_amd", "benchmark")
    common = ["--resident", "--scene", "dam-break", "--particles", "8192", "--solver-iter", "2", "--no-surface", "-n", "6", "-w", "2"]
    with_, plain = tmp_path / "with", tmp_path / "plain"
    r = subprocess.run([BIN, *common, "-o", str(with_), "--anisotropy=0.9,4,6.6667,0.5,8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([BIN, *common, "-o", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not (plain / "ellipsoids.ply").exists()
    assert (with_ / "cloud.ply").read_bytes() == (plain / "cloud.ply").read_bytes()
    ply = (with_ / "ellipsoids.ply").read_text().split("\n")
    count = int([l for l in ply if l.startswith("element vertex")][0].split()[-1])
    cloud = (with_ / "cloud.ply").read_text().split("\n")
    # the dam break has no obstacles: one ellipsoid per particle of cloud.ply, in its order, each centre (p + 0.9 mu) scale within
    # h scale of its particle's position p scale (|mu| < h; the driver's scale is 500)
    assert count == int([l for l in cloud if l.startswith("element vertex")][0].split()[-1]) and count > 4000
    rows = np.array([l.split() for l in ply[ply.index("end_header") + 1:] if l], np.float64)
    where = np.array([l.split()[:3] for l in cloud[cloud.index("end_header") + 1:] if l], np.float64)
    assert where.shape == (count, 3) and np.sqrt(((rows[:, :3] - where) ** 2).sum(1)).max() <= H * 500.0
    assert rows.shape == (count, 16) and np.isfinite(rows).all() and (rows[:, 3] >= rows[:, 5]).all() and (rows[:, 15] > 8).any()
    r = subprocess.run([BIN, *common, "--slabs", "2", "--anisotropy"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--anisotropy is a single-device feature" in r.stderr
    assert "--anisotropy" in subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
