"""pbf_sample_points / pbf_sample_lattice without a GPU: the entry points and their record are declared, exported and bound;
the reference the GPU tests use (tests/sample_ref.py) agrees with closed forms that share no reading with it, and each of
its rules, broken on purpose, breaks one of them; and on the GPU tests' scenes and point sets hardly any point has a
candidate so close to r = h that the count bracket [h (1 - delta), h (1 + delta)] could hide a wrong count."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import sample_ref as SR
from test_nversion_cpu import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, SCALE = 0.1, 500.0
SCENES = ["cubes1024", "cloud", "obstacles"]
SEEDS = {"cubes1024": 11, "cloud": 12, "obstacles": 13, "strays": 21}     # the GPU test's point sets (tests/test_sample_gpu.py)
STRAYS_MAX_X = 130.0     # the "strays" state: `obstacles`, ONE step in a box that ends at x = 130 — see oracle_state()
MUTATIONS = ["drop_cell", "sampler_mass", "obstacles_as_fluid", "strict"]


# ---- bindings ---------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_bound(pkg):
    from pbf_sph_amd import capi
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pbf_hip.h")).read(), flags=re.S)
    assert re.search(r"int pbf_sample_points\(pbf_ctx \*ctx, const pbf_params \*params, size_t n, const double \*points\s*,"
                     r" uint32_t what,\s*const pbf_sample_out \*out\);", code)
    assert re.search(r"int pbf_sample_lattice\(pbf_ctx \*ctx, const pbf_params \*params, const double origin\[3\], const double "
                     r"spacing\[3\],\s*const uint64_t dims\[3\], uint32_t what, const pbf_sample_out \*out\);", code)
    assert re.search(r"PBF_SAMPLE_VELOCITY = 1u << 0, PBF_SAMPLE_COLOUR = 1u << 1", code)
    body = re.search(r"typedef struct pbf_sample_out \{(.*?)\} pbf_sample_out;", code, flags=re.S).group(1)
    assert re.findall(r"\*(\w+);", body) == [n for n, _ in capi.SampleOut._fields_]
    assert C.sizeof(capi.SampleOut) == 6 * C.sizeof(C.c_void_p)
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("pbf_sample_points", "pbf_sample_lattice"):
        assert hasattr(L, name) and name in capi.exported_symbols()
        f = getattr(pkg.lib(), name)
        assert f.restype is C.c_int and f.argtypes[-1]._type_ is capi.SampleOut and f.argtypes[-2] is C.c_uint32
    assert pkg.SAMPLE_VELOCITY == 1 and pkg.SAMPLE_COLOUR == 2 and pkg.SampleOut is capi.SampleOut
    assert callable(pkg.Solver.sample) and callable(pkg.Solver.sample_lattice)


# ---- the reference against closed forms ------------------------------------------------------------------------------

def state(pos_s, mass=None, obstacle=None, vel=None, colour=None, extent=(24, 24, 24), lo=(-0.2, -0.2, -0.2)):
    """a hand-made state in the solver frame: keys from the positions' own cells (predict-time cell = final cell)"""
    ps = np.asarray(pos_s, np.float64).reshape(-1, 3)
    n = len(ps)
    cells = np.floor((ps - np.asarray(lo)) / H).astype(np.uint32)
    keys = SR.morton(cells[:, 0], cells[:, 1], cells[:, 2])
    down = dict(mass=np.ones(n) if mass is None else np.asarray(mass, np.float64),
                type=np.zeros(n, np.uint8) if obstacle is None else np.asarray(obstacle, np.uint8),
                vel=np.zeros((n, 3)) if vel is None else np.asarray(vel, np.float64),
                colour=np.zeros((n, 4)) if colour is None else np.asarray(colour, np.float64))
    e = np.asarray(extent, np.uint32)
    return dict(down=down, pstar=ps, keys=keys, extent=e, min_extent=np.asarray(lo), table_size=int(SR.morton(*e)))


def ref(points_s, st, **kw):
    return SR.sample(np.asarray(points_s, np.float64) * SCALE, np.float64, st["down"], st["pstar"], st["keys"], st["extent"],
                     st["min_extent"], st["table_size"], H, SCALE, **kw)


def closed_one_particle(mutate=None):
    """one particle of mass m: rho(x) = m 315 / (64 pi h^9) (h^2 - r^2)^3 at several r, 0, h exactly and just beyond.  The
    particle sits at a point whose coordinates and distances are exact in binary (h itself is not: r = h is reached by
    placing the sampler AT the particle's float64 coordinate + the float64 h along one axis, checked below)."""
    m, at = 2.5, np.array([0.75, 1.0, 0.5])
    st = state([at], mass=[m])
    rs = np.array([0.0, 0.015625, 0.03125, 0.0625, 0.09375])
    pts = at + np.stack([rs, 0 * rs, 0 * rs], -1)
    got = ref(pts, st, mutate=mutate)
    want = m * 315.0 / (64.0 * np.pi * H ** 9) * (H * H - rs * rs) ** 3
    ok = np.allclose(got["rho"], want, rtol=1e-13, atol=0) and np.array_equal(got["rho"], got["weight"])
    ok = ok and (got["count"] == [1, 0]).all() and not got["outside"].any()
    # r = h exactly: 1.0 + 0.1 - 1.0 is not 0.1, so walk along -y from 0.1 to 0: r = 0.1 - 0 = h exactly
    st0 = state([[0.75, 0.0, 0.5]], mass=[m])
    edge = ref([[0.75, H, 0.5], [0.75, np.nextafter(H, 1.0), 0.5], [0.75, 0.125, 0.5]], st0, mutate=mutate)
    ok = ok and list(edge["count"][:, 0]) == [1, 0, 0] and edge["rho"][0] == 0.0 and not edge["rho"][1:].any()
    return bool(ok)


def closed_uniform_field(mutate=None):
    """a uniform velocity and colour field: mv / weight and mc / weight equal that value to a few ulp wherever weight > 0
    — also where the masses differ and the point's neighbourhood spans all 27 cells"""
    rng = np.random.default_rng(3)
    ps = 0.6 + rng.random((400, 3)) * 0.5
    v, c = np.array([0.25, -1.5, 0.75]), np.array([0.1, 0.2, 0.3, 1.0])
    st = state(ps, mass=0.5 + rng.random(400), vel=np.tile(v, (400, 1)), colour=np.tile(c, (400, 1)))
    pts = 0.55 + rng.random((80, 3)) * 0.6
    got = ref(pts, st, mutate=mutate)
    w = got["weight"] > 0
    ok = w.sum() >= 60 and np.allclose(got["mv"][w] / got["weight"][w, None], v, rtol=1e-14, atol=0)
    ok = ok and np.allclose(got["mc"][w] / got["weight"][w, None], c, rtol=1e-14, atol=0)
    # the sum over all 27 cells against plain all pairs (a pair within h is always inside the 27 cells)
    d = np.sqrt(((pts[:, None, :] - ps[None, :, :]) ** 2).sum(-1))
    allpairs = (st["down"]["mass"][None, :] * np.where(d <= H, SR.poly6_factor(H) * (H * H - d * d) ** 3, 0.0)).sum(1)
    ok = ok and np.allclose(got["rho"], allpairs, rtol=1e-13, atol=0) and (got["count"][:, 0] == (d <= H).sum(1)).all()
    return bool(ok)


def closed_obstacle_neighbourhood(mutate=None):
    """a point whose neighbourhood holds obstacles only: rho > 0, weight = 0, count = {0, k}, no velocity"""
    ps = np.array([[1.0, 1.0, 1.0], [1.03125, 1.0, 1.0], [1.5, 1.5, 1.5]])
    st = state(ps, mass=[3.0, 3.0, 1.0], obstacle=[1, 1, 0], vel=np.ones((3, 3)))
    got = ref([[1.015625, 1.0, 1.0]], st, mutate=mutate)
    want = 2 * 3.0 * SR.poly6_factor(H) * (H * H - 0.015625 ** 2) ** 3
    return bool(np.isclose(got["rho"][0], want, rtol=1e-13) and got["weight"][0] == 0.0 and list(got["count"][0]) == [0, 2]
                and not got["mv"].any())


CLOSED = [closed_one_particle, closed_uniform_field, closed_obstacle_neighbourhood]


@pytest.mark.parametrize("form", CLOSED, ids=lambda f: f.__name__)
def test_reference_agrees_with_closed_forms(form):
    assert form()


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_every_mutation_breaks_a_closed_form(mutation):
    broken = [f.__name__ for f in CLOSED if not f(mutation)]
    print(mutation, "breaks", broken)
    assert broken


def test_reference_grid_test_and_outside_records():
    st = state([[0.75, 1.0, 0.5]])
    pts = np.array([[0.75, 1.0, 0.5], [-0.25, 1.0, 0.5], [-0.35, 1.0, 0.5], [2.15, 1.0, 0.5], [2.25, 1.0, 0.5], [0.75, 1e6, 0.5]])
    got = ref(pts, st)
    # truncation towards zero: (-0.25 + 0.2) / h = -0.5 is still cell 0; -1.5 is not
    assert list(got["outside"]) == [0, 0, 1, 0, 1, 1]
    for k in ("rho", "weight", "mv", "mc", "count"):
        assert not got[k][got["outside"] == 1].any()
    # a cell whose code + 1 reaches the table size is no cell of the grid, whatever the extent says
    code = int(SR.morton(3, 3, 3))
    cell = np.array([[3, 3, 3]])
    assert SR.in_grid(cell, st["extent"], code + 1).tolist() == [False] and SR.in_grid(cell, st["extent"], code + 2).tolist() == [True]


# ---- the scenes and point sets of the GPU test ------------------------------------------------------------------------

_STATES = {}


def oracle_state(name):
    """the oracle's state after the 3 steps (K = 2) the GPU test takes, in float64.  "strays": the `obstacles` scene after ONE
    step in a box whose upper x bound lies inside the first cube — the grid is 6 cells wide in x, the particles beyond it
    are binned at predict time into cells 6 and up (no cells of the grid, yet below the table's length) and then clamped
    onto the wall: particles that lie outside the grid, some of them in the column next to its last one."""
    if name not in _STATES:
        strays = name == "strays"
        q = O.make_params(iteration=2, mode=O.JACOBI, sort=O.SORT_STABLE, max_bound=(STRAYS_MAX_X if strays else 1000, 1000, 1000))
        o = O.Oracle(True)
        o.set_particles(**scene("obstacles" if strays else name))
        for _ in range(1 if strays else 3):
            o.step(q)
        ext, lo = o.extent()
        _STATES[name] = dict(down=o.get_particles(), pstar=o.pstar().astype(np.float64), keys=o.keys().astype(np.uint32),
                             extent=ext, min_extent=lo.astype(np.float64), table_size=len(o.table()), scale=q.scale)
    return _STATES[name]


@pytest.mark.parametrize("name", SCENES)
def test_hardly_any_point_has_a_candidate_on_the_kernel_radius(name):
    """delta = 16 eps_N (the fp32 one: the wider window).  At most 0.1 % of the points may have a candidate with r in
    (h (1 - delta), h (1 + delta)]."""
    st = oracle_state(name)
    pts, classes = SR.point_set(st["down"]["pos"], st["keys"], st["extent"], st["min_extent"], st["table_size"], H,
                                st["scale"], SEEDS[name])
    assert 400 <= len(pts) <= 600
    got = SR.sample(pts, np.float64, st["down"], st["pstar"], st["keys"], st["extent"], st["min_extent"], st["table_size"], H,
                    st["scale"])
    delta = 16 * float(np.finfo(np.float32).eps)
    near = (got["r"] > H * (1 - delta)) & (got["r"] <= H * (1 + delta))
    touched = int(near.any(1).sum())
    print(name, "points with a candidate on the radius:", touched, "of", len(pts))
    assert touched <= 0.001 * len(pts)
    # and the point set is what it claims: every class present (strays apart), outside points outside, the rest inside
    assert got["outside"][classes["outside"]].all() and not got["outside"][classes["particles"]].any()
    assert not got["outside"][classes["edge_cells"]].any() and not got["outside"][classes["random"]].any()
    assert (got["count"][classes["particles"]].sum(1) >= 1).all()          # a particle's position sees at least itself
    assert (got["weight"][classes["random"]] > 0).sum() >= 5 and (got["weight"][classes["random"]] == 0).sum() >= 5
    # no particle of these scenes ever leaves the box: the class of points near a particle outside the grid is empty here
    # (the "strays" state below is there for it)
    assert classes["near_strays"].stop == classes["near_strays"].start
    if name == "obstacles":
        assert (got["count"][:, 1] > 0).sum() >= 20


def test_the_strays_state_has_particles_outside_the_grid_that_count():
    """the fourth state of the GPU test: particles whose predict-time cell is no cell of the grid, points within h of
    them, and the same near-h condition as above"""
    st = oracle_state("strays")
    cells = SR.key_cells(st["keys"])
    stray = (cells >= st["extent"].astype(np.int64)).any(1)
    assert stray.sum() >= 100 and (st["keys"].astype(np.int64) + 1 < st["table_size"]).all()
    assert (cells[stray, 0] == st["extent"][0]).sum() >= 50            # in the column next to the grid's last one
    pts, classes = SR.point_set(st["down"]["pos"], st["keys"], st["extent"], st["min_extent"], st["table_size"], H,
                                st["scale"], SEEDS["strays"])
    near_strays = classes["near_strays"]
    assert near_strays.stop - near_strays.start == stray.sum() and len(pts) <= 1400
    got = SR.sample(pts, np.float64, st["down"], st["pstar"], st["keys"], st["extent"], st["min_extent"], st["table_size"], H,
                    st["scale"])
    seen = (got["r"][:, stray] <= H).any(1)
    print("points with a particle outside the grid within h:", int(seen.sum()), "of", len(pts))
    assert seen.sum() >= 20 and got["outside"][near_strays].any() and not got["outside"][near_strays].all()
    delta = 16 * float(np.finfo(np.float32).eps)
    touched = int(((got["r"] > H * (1 - delta)) & (got["r"] <= H * (1 + delta))).any(1).sum())
    print("strays: points with a candidate on the radius:", touched, "of", len(pts))
    assert touched <= 0.001 * len(pts)
