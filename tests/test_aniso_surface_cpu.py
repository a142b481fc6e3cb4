"""pbf_surface_anisotropic without a GPU: the entry point and its structure are declared, exported and bound; the plain-C++
half of csrc/pbf_aniso_field.hpp, compiled for the host (host/test_aniso_field.cpp), stays inside the counted bound in float
and double; the checker the GPU tests use (tests/aniso_surface_ref.py) agrees with a closed form that shares no reading with
it; on the oracle's states of the GPU tests' scenes no ellipsoid reaches beyond H from its particle, the field with and
without the cell mask is the same where the solver moved nothing, and hardly any node's hit pattern rests on a rounding;
and each rule of the field, broken on purpose in the checker, breaks the bound.

The scenes of the GPU file (tests/test_aniso_surface_gpu.py) are made here: those of tests/mc_scenes.py, `sparse` of
tests/anisotropy_scenes.py, and `pair` — 300 particles in a cluster, one particle alone and two particles on the same point,
nothing moving (iteration 0), for min_neighbours = 0: the pair takes the anisotropic branch with sigma_1 == 0 and gets the
documented non-finite record, which the field must skip.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aniso_surface_ref as AS
import anisotropy_ref as AR
import anisotropy_scenes
import mc_scenes as M
import nversion_mc as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD = os.path.join(ROOT, "pbf-sph_amd", "test_aniso_field")

SCENES = M.NAMES + ("sparse", "pair")
KERNEL = dict(smoothing=0.9, k_r=4.0, k_s=20.0 / 3.0, k_n=0.5, min_neighbours=25)     # the library's defaults
ISO = 0.4
SEED = 2014     # of `pair`: a seed at which no node's hit pattern rests on a rounding at the GPU test's resolutions (a
                # scene this small has 20 to 100 nodes with hits at the coarse ones, and the cap of 1 % is then zero)


def kernel_of(name, **kw):
    return dict(KERNEL, **({"min_neighbours": 0} if name == "pair" else {}), **kw)


def make(name):
    """a scene of tests/mc_scenes.py's shape"""
    std = dict(h=0.1, scale=500.0, min_bound=(0.0,) * 3, max_bound=(1000.0,) * 3, force=(0.0, 9.8, 0.0))
    if name == "sparse":
        return dict(sc=anisotropy_scenes.scene("sparse"), iteration=2, frames=3, **std)
    if name == "pair":
        rng = np.random.default_rng(SEED)
        cluster = np.array([60.0, 60.0, 60.0]) + rng.random((300, 3)) * 150.0
        pos = np.concatenate([cluster, [[60.0, 330.0, 70.0]], [[331.0, 317.0, 313.0]] * 2])
        return dict(sc=M._scene(pos, rng.uniform(0.03, 1.0, (len(pos), 4))), h=0.1, scale=500.0, min_bound=(0.0,) * 3,
                    max_bound=(400.0,) * 3, iteration=0, force=(0.0, 0.0, 0.0), frames=1)
    return M.make(name)


_ORACLE = {}


def oracle_state(name):
    """-> (scene, state after the last step, pStar, predict-time cells) of the float64 oracle, cached"""
    if name not in _ORACLE:
        import oracle_lib as O
        s = make(name)
        o = O.Oracle(True, device_pow=True)
        o.set_particles(**M.cast(s["sc"], np.float64))
        q = M.oracle_params(s, threads=4)
        for _ in range(s["frames"] - 1):
            o.step(q)
        before = o.get_particles()
        o.step(q)
        st = o.get_particles()
        _ORACLE[name] = (s, st, o.pstar().astype(np.float64), M.predict_time_cells(before, s, st["id"]))
    return _ORACLE[name]


def records_of(st, pstar, cells, s, dtype, kernel, mutate=None):
    """the float64 reference's ellipsoids (tests/anisotropy_ref.py) of a state, as the checker's records"""
    a = AR.anisotropy(pstar, st["type"] == 1, s["h"], s["scale"], pos_world=st["pos"], cells=cells, **kernel)
    with np.errstate(divide="ignore", invalid="ignore"):
        # (anisotropy_ref guards st == 0 for its own G; the library's record there is not finite)
        G = np.where((a["radii"] > 0).all(1)[:, None], AR.sym6(a["G"]), np.inf)
    G[st["type"] == 1] = 0.0
    return AS.records(a["centre"], G, a["radii"], st["pos"], st["type"], s["h"], s["scale"], dtype, mutate=mutate), a


def synthetic_lattice(ev, lat, dtype):
    """what a perfect implementation stores for an evaluation: {phi, -g / |g|}, C / phi, then the far nodes' colours"""
    g = ev["g"]
    gl = np.sqrt((g * g).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.where((gl > 0)[:, None], -g / gl[:, None], 0.0)
    pn = np.concatenate([ev["phi"][:, None], n], 1).astype(dtype)
    c = ev["c"].astype(dtype)
    want, zero = AS.fill_far(pn, c, lat.sample, dtype)
    c[zero] = want[zero]
    return pn, c


# ---- bindings ---------------------------------------------------------------------------------------------------------

def test_entry_point_is_declared_exported_and_bound(pkg):
    from pbf_sph_amd import capi
    text = open(os.path.join(ROOT, "include", "pbf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int pbf_surface_anisotropic\(pbf_ctx \*ctx, const pbf_params \*params, const pbf_aniso_surface \*cfg,\s*"
                     r"int indexed, uint64_t \*n_vertices\s*, uint64_t \*n_triangles\);", code)
    cfg = re.search(r"typedef struct pbf_aniso_surface \{(.*?)\} pbf_aniso_surface;", code, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", cfg).strip() == "double resolution, isolevel; pbf_anisotropy kernel;"
    assert [n for n, _ in capi.AnisoSurface._fields_] == ["resolution", "isolevel", "kernel"]
    assert C.sizeof(capi.AnisoSurface) == 16 + C.sizeof(capi.Anisotropy) and capi.AnisoSurface.kernel.offset == 16
    assert hasattr(C.CDLL(pkg.LIB_PATH), "pbf_surface_anisotropic") and "pbf_surface_anisotropic" in capi.exported_symbols()
    f = pkg.lib().pbf_surface_anisotropic
    assert f.restype is C.c_int and f.argtypes[2]._type_ is capi.AnisoSurface and f.argtypes[3] is C.c_int
    assert pkg.AnisoSurface is capi.AnisoSurface and callable(pkg.Solver.surface_anisotropic)
    # the header states the field and both deviations from the paper
    for phrase in ("anisotropic-kernel surface", "CONTRACT", "DEVIATIONS", "f = max(1, radii_1 / (0.99 - disp))", "a hit iff q2 < 1",
                   "-x +x -y +y -z +z"):
        assert phrase in text, phrase


def test_a_null_context_is_refused(pkg):
    cfg = pkg.AnisoSurface(2.0, ISO, pkg.Anisotropy(0.9, 4.0, 20 / 3, 0.5, 25))
    nt, p = C.c_uint64(), pkg.default_params(2, 1000.0)
    assert pkg.lib().pbf_surface_anisotropic(None, C.byref(p), C.byref(cfg), 0, None, C.byref(nt)) == -1


# ---- the kernels' arithmetic on the host -------------------------------------------------------------------------------

def test_host_program_stays_inside_the_counted_bound():
    r = subprocess.run([FIELD], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith(("float", "double"))]
    assert len(lines) == 2
    for l in lines:
        m = re.search(r"ratio G ([\d.]+) D ([\d.]+) t ([\d.]+) g ([\d.]+) rules (\d)", l)
        assert m and all(float(x) <= 1 for x in m.groups()[:4]) and m.group(5) == "1", l
        # (the nodes at q = 1 -+ 1e-6 lie inside float's rounding of q2 on purpose; never more than those two per record)
        assert int(re.search(r"band (\d+)", l).group(1)) <= 2 * int(re.search(r"records (\d+)", l).group(1)), l


# ---- the checker against a closed form ---------------------------------------------------------------------------------

def test_checker_matches_the_one_particle_closed_form():
    """one isolated particle, isotropic branch: phi = (1 - r^2 / (H k_n)^2)^3 / k_n^3, grad phi radial, colour its own"""
    h, scale, kn = 0.1, 500.0, 0.9
    pos = np.array([[231.0, 187.0, 263.0]])
    lat = NM.Lattice(h, scale, (0.0,) * 3, (400.0,) * 3, 3.0, np.float64)
    rec = AS.records(pos, np.array([[1 / (h * kn)] * 3 + [0.0] * 3]), np.full((1, 3), kn), pos, np.zeros(1, np.uint8), h, scale,
                     np.float64)
    assert rec["f"][0] == 1 and rec["ok"][0] and abs(rec["reach"][0] - kn) < 1e-15
    col = np.array([[0.2, 0.4, 0.6, 0.8]])
    ev = AS.evaluate(rec, col, None, lat, np.float64)
    X, Y, Z = np.meshgrid(*lat.coord, indexing="ij")
    d = np.stack([X, Y, Z], -1).reshape(-1, 3) - pos
    r2 = (d * d).sum(1)
    R = h * scale * kn
    want = np.where(r2 < R * R, (1 - r2 / R ** 2) ** 3 / kn ** 3, 0.0)
    assert (ev["hits"] > 0).sum() == (r2 < R * R).sum() > 30
    assert np.abs(ev["phi"] - want).max() <= 1e-13 * want.max()
    inside = ev["hits"] > 0
    grad = (-6 * (1 - r2 / R ** 2) ** 2 / (kn ** 3 * R * R))[:, None] * d
    assert np.abs(ev["g"][inside] - grad[inside]).max() <= 1e-12 * np.abs(grad).max()
    assert np.abs(ev["c"][inside] - col).max() <= 1e-15 and not ev["c"][~inside].any()
    assert not ev["band"].any() and ev["pre"].min() >= 1.5 * (1 - 1e-12)


# ---- the GPU tests' scenes on the oracle's states ----------------------------------------------------------------------

def _lattice(s, res, dtype):
    return NM.Lattice(s["h"], s["scale"], s["min_bound"], s["max_bound"], res, dtype)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("k_s", [20.0 / 3.0, 4.0], ids=["ks6.67", "ks4"])
def test_scenes_reach_mask_and_band(name, k_s):
    s, st, pstar, cells = oracle_state(name)
    rec, _ = records_of(st, pstar, cells, s, np.float32, kernel_of(name, k_s=k_s))
    lat = _lattice(s, 2.0, np.float32)
    fluid = st["type"] != NM.OBSTACLE
    assert (cells[fluid] >= 0).all() and (cells[fluid] < lat.extent).all(), "a particle outside the grid"
    # no ellipsoid reaches beyond H from its particle (0.99 H by the record's f; float64 rounding of the sum aside)
    print(name, "largest reach", rec["reach"].max(), "f > 1 on", int((rec["f"][rec["ok"]] > 1).sum()), "of", int(rec["ok"].sum()))
    assert rec["reach"].max() <= 0.99 + 1e-6
    masked = AS.evaluate(rec, st["colour"], cells, lat, np.float32)
    free = AS.evaluate(rec, st["colour"], None, lat, np.float32)
    same = np.array_equal(masked["hits"], free["hits"])
    print(name, "nodes with hits", int((masked["hits"] > 0).sum()), "band", int(masked["band"].sum()), "mask == all pairs:", same)
    if s["iteration"] == 0:
        # nothing moved: a particle's cell is its position's, and the reach set is a subset of the 27-cell walk
        assert same
        assert np.abs(masked["phi"] - free["phi"]).max() <= 1e-12 * max(1.0, free["phi"].max())
        assert np.abs(masked["g"] - free["g"]).max() <= 1e-12 * max(1.0, np.abs(free["g"]).max())
    with_hits = int((masked["hits"] > 0).sum())
    assert with_hits > 40
    assert int((masked["band"] & (masked["hits"] > 0)).sum()) <= 0.01 * with_hits
    assert masked["pre"].min() >= 1.4, "the pre-test must never decide a hit"


def test_pair_scene_holds_the_skipped_record_and_an_isolated_particle():
    s, st, pstar, cells = oracle_state("pair")
    rec, a = records_of(st, pstar, cells, s, np.float32, kernel_of("pair"))
    assert (~rec["ok"]).sum() == 2 and (a["neighbours"][~rec["ok"]] == 1).all() and not a["radii"][~rec["ok"]].any()
    alone = a["neighbours"] == 0
    assert alone.sum() == 1 and (a["radii"][alone] == 0.5).all() and rec["f"][alone][0] == 1
    assert (rec["f"][rec["ok"]] > 1).any()


# ---- the bound bites ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mutate", AS.MUTATIONS)
def test_a_broken_rule_breaks_the_bound(mutate, dtype):
    name = "faces"                                         # (particles in face, edge and corner cells: the clamp folds)
    s, st, pstar, cells = oracle_state(name)
    lat = _lattice(s, 1.5, dtype)
    kernel = kernel_of(name, min_neighbours=8)             # (with 25 the whole scene is isotropic with f == 1)
    rec, _ = records_of(st, pstar, cells, s, dtype, kernel)
    assert (rec["f"][rec["ok"]] > 1).sum() > 100 and (rec["f"][rec["ok"]] == 1).sum() > 100
    ev = AS.evaluate(rec, st["colour"], cells, lat, dtype)
    pn, c = synthetic_lattice(ev, lat, dtype)
    good = AS.compare(pn, c, rec, st["colour"], cells, lat, dtype, ev=ev)
    print("unmutated", AS.summary(good))
    assert good["worst"] <= 1 and good["pattern_bad"] == 0 and good["nan"] == 0 and good["with_hits"] > 100
    bad_rec, _ = records_of(st, pstar, cells, s, dtype, kernel, mutate=mutate)
    bad = AS.compare(pn, c, bad_rec, st["colour"], cells, lat, dtype, mutate=mutate)
    print(mutate, AS.summary(bad))
    assert bad["worst"] > 1 or bad["pattern_bad"] > 0
