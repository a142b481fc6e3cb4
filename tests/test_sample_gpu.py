"""pbf_sample_points / pbf_sample_lattice on a GPU: against the float64 all-points-against-all-particles restatement
(tests/sample_ref.py), independence of a point's record from the batch it travels in, the lattice against the same points
formed in numpy, consistency with PBF_BUF_DENSITY, that the call observes without changing anything a step does, its
refusals, the benchmark flag and the C++ shim.

Bars (fp64 and fp32; u = eps_N / 2 + eps_64 / 2, the device's rounding unit plus the reference's).  Both sides start from
the same bits: x_s is formed in N with numpy, pStar, masses, velocities and colours are read back.  One pair term
w = m (K (d d d)), d = h h - r r:
  b - a per axis 1 rounding, its square 1, the sum of three 2:       d2 (1 + 5u)      [relative]
  r = sqrt(d2) 1 rounding:  r (1 + 3.5u);   r r 1 rounding:          r^2 (1 + 8u), r^2 <= h^2
  h h 1 rounding, the subtraction 1 (|d| <= h^2):                    |delta d| <= 10u h^2
  d^3: 3 d^2 delta d <= 30u h^6, its two products 2u;  K formed in N from h (pow, two products, a divide) <= 12u;
  the products with K and m 2u                                       |delta w| <= 46u m W(0)  -> 48u m W(0)
(an error relative to W(0) = K h^6, not to w: near r = h the cancellation in d leaves no relative accuracy).  A term of mv /
mc is one more product: u |term|.  Summing k terms in any order adds at most (k - 1) u sum|term|.  Hence per point and output
    bar = 48u cap + (k + 1) u sum|term|,     cap = sum over the in-range candidates of m_j W(0) |f_j|,  f = 1, v_j or c_j,
k = the candidates within h (1 + 16 eps_N); both sums come from the reference.  A candidate that one side admits and the
other does not lies within 16 eps_N of h: its term is below (32 eps_N)^3 m W(0), far inside the bar.
Beside that, no error may exceed the bars the project already holds this sum to — 1e-12 (fp64) and 3e-5 (fp32) of the batch
maximum (tests/test_diagnostics_gpu.py, tests/test_surface_tension_gpu.py).  With PBF_FLAG_FAST_MATH (v_rsq, fma) the
pair term has no such derivation: the bar is the one tests/test_diagnostics_gpu.py gives rho under that flag, 3e-5 of the
batch maximum.
count: between the reference at thresholds h (1 - 16 eps_N) and h (1 + 16 eps_N) — tests/test_sample_cpu.py shows that no
point of these sets has a candidate in that window.  outside: exact, and such a record is all zeros.

The class "points within h of a particle that lies outside the grid" of the point sets is empty on these three scenes:
their particles never leave the box, so every predict-time cell is a cell of the grid (tests/test_sample_cpu.py asserts
it).  A fourth state, "strays", is there for that class: `obstacles` after ONE step in a box that ends inside the first
cube, which leaves hundreds of particles binned outside the grid and clamped onto its wall, within h of sampled points
(tests/test_sample_cpu.py: oracle_state).  It is held to the same bars."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import sample_ref as SR
from test_cli_gpu import BIN
from test_nversion_cpu import scene
from test_sample_cpu import SEEDS, STRAYS_MAX_X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 0.1
VARIANTS = [(True, False), (False, False), (False, True)]   # (fp64, PBF_FLAG_FAST_MATH)
IDS = ["fp64", "fp32", "fp32-fast"]
SCENES = ["cubes1024", "cloud", "obstacles"]
ERR_INVALID, ERR_STATE = -1, -4
SUMS = ["rho", "weight", "mv", "mc"]


def solver(pkg, sc, fp64, fast=False, **options):
    s = pkg.Solver(h=H, fp64=fp64, flags=pkg.FLAG_FAST_MATH if fast else 0)
    for k, v in options.items():
        s.set_option(k, v)
    return s.upload(**sc)


_STEPPED = {}


def stepped(pkg, name, fp64, fast):
    """the scene after 3 steps (K = 2), its read-back state, the point set and the reference at three thresholds — made
    once per (scene, variant) and left unchanged"""
    key = (name, fp64, fast)
    if key not in _STEPPED:
        p = pkg.default_params(2, 1000.0)
        if name == "strays":
            p.max_bound[0] = STRAYS_MAX_X
            s = solver(pkg, scene("obstacles"), fp64, fast).steps(p, 1)
        else:
            s = solver(pkg, scene(name), fp64, fast).steps(p, 3)
        dt = np.float64 if fp64 else np.float32
        ext, lo = s.extent()
        st = dict(down=s.download(), pstar=s.pstar(), keys=s.keys(), extent=ext, min_extent=lo, table_size=len(s.table()),
                  h=float(dt(H)), scale=p.scale, dtype=dt)
        pts, classes = SR.point_set(st["down"]["pos"], st["keys"], ext, lo, st["table_size"], H, p.scale, SEEDS[name])
        delta = 16 * float(np.finfo(dt).eps)
        ref = {k: reference(pts, st, st["h"] * (1 + k * delta)) for k in (-1, 0, 1)}
        _STEPPED[key] = (s, p, st, pts, classes, ref)
    return _STEPPED[key]


def reference(pts, st, threshold=None):
    return SR.sample(pts, st["dtype"], st["down"], st["pstar"], st["keys"], st["extent"], st["min_extent"], st["table_size"],
                     st["h"], st["scale"], threshold=threshold)


def check_against(got, ref, fp64, fast, label=""):
    """got: Solver.sample dict; ref: {-1, 0, 1} -> reference at h (1 + k 16 eps).  The bars of the module docstring."""
    u = float(np.finfo(np.float64 if fp64 else np.float32).eps) / 2 + float(np.finfo(np.float64).eps) / 2
    project = 1e-12 if fp64 else 3e-5
    mid, hi = ref[0], ref[1]
    assert np.array_equal(got["outside"], mid["outside"])
    out = mid["outside"] == 1
    k_all, k_fluid = hi["count"].sum(1), hi["count"][:, 0]
    for name in SUMS:
        if name not in got:
            continue
        g = got[name].astype(np.float64)
        err = np.abs(g - mid[name])
        k = k_all if name == "rho" else k_fluid
        k = k if g.ndim == 1 else k[:, None]
        top = np.abs(mid[name]).max()
        bar = np.full_like(err, project * top) if fast else np.minimum(48 * u * hi["cap_" + name] + (k + 1) * u * hi["abs_" + name],
                                                                       project * top)
        print(label, name, "max error", err.max(), "largest bar", bar.max(), "batch maximum", top,
              "worst error / bar", np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0))))
        assert np.all(err <= bar), (name, int(np.argmax(err - bar)))
        assert not g[out].any(), name
    assert np.all(ref[-1]["count"] <= got["count"]) and np.all(got["count"] <= hi["count"])
    assert not got["count"][out].any()


def same_records(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a) and set(a) == set(b)


# ---- 1. against the reference -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", SCENES)
def test_against_the_all_pairs_reference(pkg, name, fp64, fast):
    s, p, st, pts, classes, ref = stepped(pkg, name, fp64, fast)
    got = s.sample(p, pts, velocity=True, colour=True)
    check_against(got, ref, fp64, fast, name)
    assert got["outside"][classes["outside"]].all() and not got["outside"][classes["particles"]].any()
    assert (got["weight"] > 0).sum() >= 150 and (got["weight"][~got["outside"].astype(bool)] == 0).sum() >= 20
    # the normalised fields are the stated division, 0 where weight == 0
    w = got["weight"] > 0
    assert np.array_equal(got["velocity"][w], got["mv"][w] / got["weight"][w, None]) and not got["velocity"][~w].any()
    assert np.array_equal(got["colour"][w], got["mc"][w] / got["weight"][w, None]) and not got["colour"][~w].any()
    # fewer flags: the sums that remain are the same bits
    for vel, col in ((False, False), (True, False), (False, True)):
        part = s.sample(p, pts, velocity=vel, colour=col)
        assert ("mv" in part) == vel and ("mc" in part) == col
        assert all(np.array_equal(part[k], got[k]) for k in part)


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_particles_outside_the_grid_are_candidates_by_their_keys(pkg, fp64, fast):
    """the "strays" state: a particle binned beyond the extent, but below the table's length, is walked from the grid's
    last column and counts where its final pStar is within h; a point in such a particle's own cell is outside"""
    s, p, st, pts, classes, ref = stepped(pkg, "strays", fp64, fast)
    stray = (SR.key_cells(st["keys"]) >= st["extent"].astype(np.int64)).any(1)
    seen = (ref[0]["r"][:, stray] <= st["h"]).any(1)
    print("particles outside the grid:", int(stray.sum()), "points with one of them within h:", int(seen.sum()))
    assert stray.sum() >= 100 and seen.sum() >= 20
    got = s.sample(p, pts, velocity=True, colour=True)
    check_against(got, ref, fp64, fast, "strays")
    near = classes["near_strays"]
    assert got["outside"][near].any() and not got["outside"][near].all() and (got["count"][seen].sum(1) > 0).all()


# ---- 2. independence of the batch -------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_a_record_does_not_depend_on_its_batch(pkg, fp64, fast):
    s, p, st, pts, classes, ref = stepped(pkg, "obstacles", fp64, fast)
    base = s.sample(p, pts, velocity=True, colour=True)
    perm = np.random.default_rng(5).permutation(len(pts))
    again = s.sample(p, pts[perm], velocity=True, colour=True)
    assert same_records({k: v[perm] for k, v in base.items()}, again)
    at = 0
    for size in (1, 63, 64, 65, 255, 256, 257):
        idx = (at + np.arange(size)) % len(pts)
        at += size
        part = s.sample(p, pts[idx], velocity=True, colour=True)
        assert same_records({k: v[idx] for k, v in base.items()}, part), size
    assert s.sample(p, np.zeros((0, 3)))["rho"].shape == (0,)        # n = 0: PBF_OK, nothing launched


# ---- 3. the lattice equals the points ---------------------------------------------------------------------------------

GUARD = 0xAB


def guarded(n, dtype):
    """n elements of dtype between two 64-byte guards -> (the whole buffer as bytes, the middle as an array)"""
    size = n * np.dtype(dtype).itemsize
    raw = np.full(size + 128, GUARD, np.uint8)
    return raw, raw[64:64 + size].view(dtype)


def guards_intact(raw):
    return (raw[:64] == GUARD).all() and (raw[-64:] == GUARD).all()


def raw_lattice(pkg, s, p, origin, spacing, dims, what, want):
    """pbf_sample_lattice straight through the C ABI; `want`: names of the outputs handed over (the rest NULL)"""
    from pbf_sph_amd import capi
    n = int(np.prod(dims))
    shapes = dict(rho=(n, s.dtype), weight=(n, s.dtype), mv=(3 * n, s.dtype), mc=(4 * n, s.dtype), count=(2 * n, np.uint32),
                  outside=(n, np.uint8))
    bufs = {k: guarded(*shapes[k]) for k in want}
    out = capi.SampleOut(*[bufs[k][1].ctypes.data if k in bufs else None for k in ("rho", "weight", "mv", "mc", "count", "outside")])
    o, sp, d = np.asarray(origin, np.float64), np.asarray(spacing, np.float64), np.asarray(dims, np.uint64)
    rc = pkg.lib().pbf_sample_lattice(s.ctx, C.byref(p), o.ctypes.data, sp.ctypes.data, d.ctypes.data, what, C.byref(out))
    return rc, bufs


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("dims", [(1, 1, 1), (4, 4, 4), (5, 7, 9), (9, 4, 3), (1, 1, 130)], ids=lambda d: "x".join(map(str, d)))
def test_lattice_equals_points_bit_for_bit(pkg, dims, fp64, fast):
    s, p, st, _, _, _ = stepped(pkg, "obstacles", fp64, fast)
    N = st["dtype"]
    pos = st["down"]["pos"].astype(np.float64)
    lo_w, hi_w = pos.min(0), pos.max(0)
    cell = H * p.scale
    origin, spacing = lo_w + 7.0, (hi_w - lo_w) / np.asarray(dims)
    first = next((a for a in range(3) if dims[a] > 1), None)
    if first is not None:          # the first plane of that axis lies 2.3 cells below the grid, the last at the far end of the fluid
        origin[first] = st["min_extent"][first] * p.scale - 2.3 * cell
        spacing[first] = (hi_w[first] - origin[first]) / (dims[first] - 1)
    # the same points formed in numpy, in N: origin + N(i) * spacing, one multiply and one add
    oN, sN = origin.astype(N), spacing.astype(N)
    idx = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    pts = (oN + idx.astype(N) * sN)
    assert pts.dtype == np.dtype(N)
    for vel, col in ((True, True), (False, False), (True, False), (False, True)):
        a = s.sample(p, pts.astype(np.float64), velocity=vel, colour=col)
        b = s.sample_lattice(p, origin, spacing, dims, velocity=vel, colour=col)
        assert same_records(a, b), (vel, col)
        if first is not None:
            assert a["outside"].any() and not a["outside"].all() and (a["weight"] > 0).any()
        # through the C ABI with guards: what is handed over is written inside its bounds, what is not asked for is NULL
        what = (pkg.SAMPLE_VELOCITY if vel else 0) | (pkg.SAMPLE_COLOUR if col else 0)
        want = ["rho", "weight", "count", "outside"] + (["mv"] if vel else []) + (["mc"] if col else [])
        rc, bufs = raw_lattice(pkg, s, p, origin, spacing, dims, what, want)
        assert rc == 0 and all(guards_intact(raw) for raw, _ in bufs.values())
        assert all(np.array_equal(bufs[k][1], a[k].ravel()) for k in want)
        rc, bufs = raw_lattice(pkg, s, p, origin, spacing, dims, what, ["weight", "outside"])     # the neighbours are NULL
        assert rc == 0 and all(guards_intact(raw) for raw, _ in bufs.values())
        assert np.array_equal(bufs["weight"][1], a["weight"]) and np.array_equal(bufs["outside"][1], a["outside"])


# ---- 4. consistency with PBF_BUF_DENSITY ------------------------------------------------------------------------------

@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", ["cubes1024", "cloud"])
def test_sampling_at_a_particle_gives_its_density(pkg, name, fp64, fast):
    """unit masses: the sum at x_s = pStar_i is rho_i of the density pass, where the point's cell is the particle's
    predict-time cell.  The world point is chosen so that N(point) / scale gives pStar_i back exactly; a particle without
    such a point among the three nearest candidates is left out."""
    s, p, st, _, _, _ = stepped(pkg, name, fp64, fast)
    N = st["dtype"]
    assert (st["down"]["mass"] == 1).all()
    s.diagnostics(p, density=True)
    rho = s.density().astype(np.float64)
    ps = st["pstar"][:, :3]
    w = ps * N(p.scale)
    cands = np.stack([w, np.nextafter(w, N(np.inf)), np.nextafter(w, N(-np.inf))])
    exact = (cands / N(p.scale)) == ps[None]
    pick = np.argmax(exact, 0)
    pts = np.take_along_axis(cands, pick[None], 0)[0]
    reachable = exact.any(0).all(1)
    _, cx = SR.point_cells(pts.astype(np.float64), N, st["h"], p.scale, st["min_extent"])
    home = (cx == SR.key_cells(st["keys"])).all(1)
    ok = reachable & home
    print(name, "share of particles whose final pStar is in their predict-time cell:", home.mean(), "used:", ok.mean())
    if name == "cubes1024":
        assert home.mean() >= 0.5
    assert ok.sum() >= 0.4 * len(ps)
    got = s.sample(p, pts[ok].astype(np.float64))
    delta = 16 * float(np.finfo(N).eps)
    ref = {k: reference(pts[ok].astype(np.float64), st, st["h"] * (1 + k * delta)) for k in (-1, 0, 1)}
    check_against(got, ref, fp64, fast, name)
    u = float(np.finfo(N).eps) / 2 + float(np.finfo(np.float64).eps) / 2
    top = np.abs(ref[0]["rho"]).max()
    project = (1e-12 if fp64 else 3e-5) * top
    bar = np.full(int(ok.sum()), project) if fast else np.minimum(
        48 * u * ref[1]["cap_rho"] + (ref[1]["count"].sum(1) + 1) * u * ref[1]["abs_rho"], project)
    err = np.abs(got["rho"].astype(np.float64) - rho[ok])
    print(name, "sample vs density(): max error", err.max(), "identical bits:", int((err == 0).sum()), "of", int(ok.sum()))
    assert np.all(err <= bar)
    assert np.array_equal(got["rho"], got["weight"])


# ---- 5. observer only -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("fp64", [True, False], ids=["fp64", "fp32"])
def test_a_call_between_steps_changes_nothing(pkg, fp64, graph):
    p = pkg.default_params(2, 1000.0)
    plain, split, watched = (solver(pkg, scene("cubes1024"), fp64, graph=graph) for _ in range(3))
    plain.steps(p, 6)
    split.steps(p, 3).steps(p, 3)
    watched.steps(p, 3)
    pts = watched.download()["pos"][::5].astype(np.float64) + 3.0
    before = watched.graph_stats()
    a = watched.sample(p, pts, velocity=True, colour=True)
    lat = watched.sample_lattice(p, pts.min(0) - 200.0, (30.0, 30.0, 30.0), (6, 5, 7), velocity=True)
    assert same_records(a, watched.sample(p, pts, velocity=True, colour=True))            # two calls, identical bytes
    assert same_records(lat, watched.sample_lattice(p, pts.min(0) - 200.0, (30.0, 30.0, 30.0), (6, 5, 7), velocity=True))
    assert watched.graph_stats() == before
    watched.steps(p, 3)
    want, got = plain.download(), watched.download()
    assert all(want[k].tobytes() == got[k].tobytes() for k in want)
    assert all(want[k].tobytes() == split.download()[k].tobytes() for k in want)
    assert watched.graph_stats() == split.graph_stats()
    print("graph stats", watched.graph_stats())
    if graph:
        assert watched.graph_stats()[0] > 0, "the graph path was not exercised"


# ---- 6. refusals ------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(pkg):
    from pbf_sph_amd import capi
    L = pkg.lib()
    p = pkg.default_params(2, 1000.0)
    s = solver(pkg, scene("cubes1024"), False)
    n = 8
    pts = np.ascontiguousarray(scene("cubes1024")["pos"][:n], np.float64)
    names = ("rho", "weight", "mv", "mc", "count", "outside")
    bufs = dict(rho=guarded(n, np.float32), weight=guarded(n, np.float32), mv=guarded(3 * n, np.float32),
                mc=guarded(4 * n, np.float32), count=guarded(2 * n, np.uint32), outside=guarded(n, np.uint8))

    def out_of(*which):
        return capi.SampleOut(*[bufs[k][1].ctypes.data if k in which else None for k in names])

    full, both = out_of(*names), pkg.SAMPLE_VELOCITY | pkg.SAMPLE_COLOUR
    o3, s3 = np.array([100.0, 100.0, 100.0]), np.array([10.0, 10.0, 10.0])
    d3 = np.array([2, 2, 2], np.uint64)

    def points(code, why, ctx, params, m, pp, what, out):
        assert L.pbf_sample_points(ctx, params, m, pp, what, out) == code, why
        assert all((raw == GUARD).all() for raw, _ in bufs.values()), why

    def lattice(code, why, ctx, params, dims, what, out, origin=o3, spacing=s3):
        assert L.pbf_sample_lattice(ctx, params, origin.ctypes.data, spacing.ctypes.data, dims.ctypes.data, what, out) == code, why
        assert all((raw == GUARD).all() for raw, _ in bufs.values()), why

    P, X = C.byref(p), pts.ctypes.data
    points(ERR_STATE, "before any step", s.ctx, P, n, X, both, C.byref(full))
    lattice(ERR_STATE, "before any step", s.ctx, P, d3, both, C.byref(full))
    s.step(p)
    bad = pts.copy()
    bad[3, 1] = np.nan
    points(ERR_INVALID, "NaN point", s.ctx, P, n, bad.ctypes.data, both, C.byref(full))
    bad[3, 1] = np.inf
    points(ERR_INVALID, "infinite point", s.ctx, P, n, bad.ctypes.data, both, C.byref(full))
    lattice(ERR_INVALID, "NaN origin", s.ctx, P, d3, both, C.byref(full), origin=np.array([np.nan, 0.0, 0.0]))
    lattice(ERR_INVALID, "infinite spacing", s.ctx, P, d3, both, C.byref(full), spacing=np.array([1.0, np.inf, 1.0]))
    lattice(ERR_INVALID, "zero dim", s.ctx, P, np.array([2, 0, 2], np.uint64), both, C.byref(full))
    lattice(ERR_INVALID, "2^31 points", s.ctx, P, np.array([2048, 1024, 1024], np.uint64), both, C.byref(full))
    points(ERR_INVALID, "mv without its flag", s.ctx, P, n, X, pkg.SAMPLE_COLOUR, C.byref(full))
    points(ERR_INVALID, "mc without its flag", s.ctx, P, n, X, pkg.SAMPLE_VELOCITY, C.byref(full))
    lattice(ERR_INVALID, "mv without its flag", s.ctx, P, d3, 0, C.byref(full))
    points(ERR_INVALID, "unknown bit", s.ctx, P, n, X, 4, C.byref(out_of("rho")))
    points(ERR_INVALID, "unknown bit beside known ones", s.ctx, P, n, X, both | 1 << 31, C.byref(full))
    points(ERR_INVALID, "NULL points", s.ctx, P, n, None, both, C.byref(full))
    points(ERR_INVALID, "NULL out", s.ctx, P, n, X, both, None)
    points(ERR_INVALID, "NULL params", s.ctx, None, n, X, both, C.byref(full))
    assert L.pbf_sample_points(s.ctx, None, 0, None, 0, None) == 0                         # n = 0
    q = pkg.default_params(2, 1000.0)
    q.max_bound[0] = 1400.0
    points(ERR_STATE, "params of another grid", s.ctx, C.byref(q), n, X, both, C.byref(full))
    assert b"differ" in L.pbf_last_error(s.ctx)
    lattice(ERR_STATE, "params of another grid", s.ctx, C.byref(q), d3, both, C.byref(full))
    assert s.sample(p, pts)["rho"].shape == (n,)                                           # the refusals left the grid alone
    s.upload(**{k: (v.astype(np.float32) if v.dtype.kind == "f" else v) for k, v in scene("cubes1024").items()})
    points(ERR_STATE, "after an upload", s.ctx, P, n, X, both, C.byref(full))
    s.step(p)
    cut = capi.SlabCut(0, 12, 0, 0)
    assert L.pbf_slab_configure(s.ctx, C.byref(cut), 0, 0) == 0
    points(ERR_STATE, "slab mode", s.ctx, P, n, X, both, C.byref(full))
    lattice(ERR_STATE, "slab mode", s.ctx, P, d3, both, C.byref(full))
    assert b"slab" in L.pbf_last_error(s.ctx)


# ---- 7. CLI and shim --------------------------------------------------------------------------------------------------

def test_benchmark_probe_flag(pkg, tmp_path):
    sc, side = pkg.scene_dambreak(8192)
    probes = [sc["pos"][100].astype(np.float64) + 2.0, sc["pos"][4000].astype(np.float64) - 3.0, np.array([-900.0, 50.0, 50.0])]
    flags = ["--probe=" + ",".join(repr(float(v)) for v in q) for q in probes]
    common = ["--resident", "--scene", "dam-break", "--particles", "8192", "--solver-iter", "2", "--no-surface", "-n", "4", "-w", "2",
              "-o", str(tmp_path / "out"), "--json"]

    def run(*extra):
        r = subprocess.run([BIN, *common, *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.split("\n")
        return [json.loads(l) for l in lines if l.startswith('{"frame"')], [json.loads(l) for l in lines if l.startswith('{"impl"')][0]

    once, summary = run(*flags)
    every, summary2 = run(*flags, "--probe-every=2")
    none, plain = run()
    assert [l["frame"] for l in once] == [3] and [l["frame"] for l in every] == [1, 3] and none == []
    assert once[0] == every[1]
    # the same scene and frames through the C ABI
    s = pkg.Solver(h=H).upload(**sc)
    p = pkg.default_params(2, side)
    want = {}
    for frame in (0, 1, 0, 1, 2, 3):                     # two warm-up frames, then the timed ones
        s.step(p)
        want[frame] = s.sample(p, np.array(probes), velocity=True, colour=True)
    for line in every:
        w = want[line["frame"]]
        assert len(line["probes"]) == 3
        for i, q in enumerate(line["probes"]):
            assert q["at"] == [float(v) for v in probes[i]]
            assert np.float32(q["rho"]) == w["rho"][i] and np.float32(q["weight"]) == w["weight"][i]
            assert np.array_equal(np.float32(q["velocity"]), w["velocity"][i]) and np.array_equal(np.float32(q["colour"]), w["colour"][i])
            assert q["count"] == [int(v) for v in w["count"][i]] and q["outside"] == int(w["outside"][i])
    assert every[1]["probes"][0]["weight"] > 0 and every[1]["probes"][2]["outside"] == 1
    # the reports' time is kept out: in every run the timed interval is the frames plus the loop's own overhead.  (The CLI
    # tests hold frame times to no spread of their own; what is checked is each run's own bookkeeping.)
    for name, j in (("no probe", plain), ("once", summary), ("every 2", summary2)):
        assert j["frames"] == 4
        rest = j["seconds"] * 1000.0 - j["frames"] * j["frame_ms_mean"]
        print(name, "frame_ms_mean", j["frame_ms_mean"], "timed interval minus frames (ms)", rest)
        assert -0.01 * j["frames"] * j["frame_ms_mean"] - 0.01 <= rest <= 0.25 * j["frames"] * j["frame_ms_mean"] + 0.5
    # the frame times themselves: those of the run without the flag, to a declared factor of 3 either way (a frame of this
    # scene takes ~0.15 ms and nothing but the machine's noise separates the runs; the first report makes the call's
    # allocations and costs several frames, so one that leaked into a frame's time would show)
    for j in (summary, summary2):
        assert plain["frame_ms_mean"] / 3 <= j["frame_ms_mean"] <= 3 * plain["frame_ms_mean"], (j, plain)
    # refusals of the flag, as --diagnostics has them
    r = subprocess.run([BIN, *common, "--slabs", "2", flags[0]], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--probe is a single-device feature" in r.stderr
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert "--probe=" in r.stdout and "--probe-every" in r.stdout


def test_shim(pkg):
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_sample_shim")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
