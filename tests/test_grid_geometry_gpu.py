"""Bit-exact parity on large, non-cubic and offset grids (tests/grid_scenes.py): the device against the oracle
(device_pow = True) stage by stage and over free-running frames, for the product default and the variants whose code
changes with the grid's shape — the quantised positions' 16-bit wrap, the 64-cell x-segments of the row diffusion, the
row cube up to P = 1024 with its ROW_FALLBACK face walkers and the reference's 10-bit wrap between x-columns 0 and
1023.  tests/test_grid_geometry_cpu.py checks that each geometry really exercises its mechanism.

edge_x allocates a 2^30-cell row cube (about 8 GiB) and a 1.5e8-entry table per solver: every solver is closed before
the next one is made, and the oracle's trace of one geometry is dropped before the next geometry's is computed.
"""
import numpy as np
import pytest

import grid_scenes as G

pytestmark = pytest.mark.gpu

FIELDS = ("id", "type", "mass", "pos", "vel", "colour")
FRAMES = 4

# option sets: the product default (row-major lists + row diffusion), the Morton-order forms, the plain global walk,
# the LDS tiles, the per-cell Morton diffusion, the row diffusion's walk-from-memory path (a one-record tile), the
# separate list-build launch, and pbf_steps (finalise(t) + predict(t + 1) fused)
VARIANTS = {"default": {}, "morton": {"row_major": 0}, "global": {"gather": 0}, "tiles": {"gather": 3},
            "cell_diffuse": {"row_diffuse": 0}, "cap1": {"diffuse_cap": 1}, "split5": {"split_build": 5},
            "steps": {}}
CASES = [(name, False, v) for name in G.NAMES for v in ("default", "morton", "global", "tiles", "cell_diffuse", "cap1")]
CASES += [("long_x", False, "split5"), ("long_x", False, "steps")]
CASES += [(name, True, v) for name in ("long_x", "edge_x") for v in ("default", "morton")]
CASES.sort(key=lambda c: (G.NAMES.index(c[0]), c[1]))  # one geometry at a time: one oracle trace alive

_TRACE = {}


def snapshot(o):
    return {k: np.array(v, copy=True) for k, v in o.get_particles().items()}


def oracle_trace(oracle, name, fp64):
    """The oracle's stage-by-stage frame 0 and the states after frames 0 .. FRAMES - 1, computed once per geometry
    and precision (a single entry: edge_x's table alone is 0.6 GB as uint32)."""
    key = (name, fp64)
    if key not in _TRACE:
        _TRACE.clear()
        sc, _, q, _ = G.make_geometry(name, fp64)
        o = oracle.Oracle(fp64, device_pow=True)
        o.set_particles(**sc)
        t = {}
        o.predict(q)
        t["predict_keys"], t["predict_pstar"] = o.keys(), o.pstar()
        o.sort(q).grid_table(q)
        t["keys"] = o.keys()
        table = o.table()
        assert table.max() < 2 ** 32
        t["table"] = table.astype(np.uint32)
        del table
        t["extent"] = o.extent()
        t["sorted"], t["sorted_pstar"] = snapshot(o), o.pstar()
        o.diffuse(q)
        t["colour"] = o.get_particles()["colour"]
        t["lambda"], t["pstar"] = [], []
        for _ in range(q.iteration):
            o.lambda_(q)
            t["lambda"].append(o.lambdas())
            o.delta(q)
            t["pstar"].append(o.pstar())
        o.finalise(q)
        t["frames"] = [snapshot(o)]
        for _ in range(1, FRAMES):
            o.step(q)
            t["frames"].append(snapshot(o))
        del o
        _TRACE[key] = t
    return _TRACE[key]


def assert_state_equal(g, w, what=""):
    for k in FIELDS:
        assert np.array_equal(g[k], w[k]), (what, k, np.abs(g[k].astype(np.float64) - w[k]).max())


def solver(pkg, name, fp64, variant):
    sc, p, _, h = G.make_geometry(name, fp64, pkg)
    s = pkg.Solver(h=h, fp64=fp64)
    for k, v in VARIANTS[variant].items():
        s.set_option(k, v)
    s.upload(**sc)
    return s, p


@pytest.mark.parametrize("name,fp64,variant", CASES, ids=[f"{n}-{'f64' if d else 'f32'}-{v}" for n, d, v in CASES])
def test_geometry_bit_exact(pkg, oracle, name, fp64, variant):
    t = oracle_trace(oracle, name, fp64)
    s, p = solver(pkg, name, fp64, variant)
    try:
        if variant == "steps":  # two calls of two steps: each call fuses finalise + predict between its steps
            s.steps(p, 2)
            assert_state_equal(s.download(), t["frames"][1], "steps frame 1")
            s.steps(p, 2)
            assert_state_equal(s.download(), t["frames"][3], "steps frame 3")
            return
        s.stage("predict", p)
        assert np.array_equal(s.keys().astype(np.uint64), t["predict_keys"])
        assert np.array_equal(s.pstar()[:, :3], t["predict_pstar"])
        s.stage("sort", p)
        assert np.array_equal(s.keys().astype(np.uint64), t["keys"])
        e, m = s.extent()
        assert tuple(int(v) for v in e) == G.GEOMETRIES[name]["ext"]
        assert np.array_equal(e, t["extent"][0]) and np.array_equal(m, t["extent"][1].astype(np.float64))
        table = s.table()
        assert len(table) == len(t["table"]) == G.table_len(G.GEOMETRIES[name]["ext"])
        assert np.array_equal(table, t["table"])
        del table
        assert_state_equal(s.download(), t["sorted"], "sort")
        assert np.array_equal(s.pstar()[:, :3], t["sorted_pstar"])
        s.stage("diffuse", p)
        assert np.array_equal(s.download()["colour"], t["colour"]), "diffuse"
        for it in range(p.iteration):
            s.stage("lambda", p)
            assert np.array_equal(s.pstar()[:, 3], t["lambda"][it]), ("lambda", it)
            s.stage("delta", p)
            assert np.array_equal(s.pstar()[:, :3], t["pstar"][it]), ("delta", it)
        s.stage("finalise", p)
        assert_state_equal(s.download(), t["frames"][0], "finalise")
        for frame in range(1, FRAMES):
            s.step(p)
            assert_state_equal(s.download(), t["frames"][frame], f"frame {frame}")
    finally:
        s.close()


SURFACES = [("long_x", dict(isolevel=30.0)),
            ("long_x", dict(resolution=1.5, particle_influence=0.75, isolevel=30.0)),
            ("offset", dict()),
            ("offset", dict(resolution=1.5, particle_influence=0.75))]


@pytest.mark.parametrize("name,mc", SURFACES, ids=[f"{n}-{i}" for i, (n, _) in enumerate(SURFACES)])
def test_geometry_surface(pkg, oracle, name, mc):
    """As tests/test_mc.py::test_surface_gpu_vs_oracle on a non-cubic lattice (the per-axis clamps of the 27-cell walk)
    and a non-default one (resolution 1.5, influence 0.75: the pow branch).  Influence 0.5: field and mesh bit-exact
    against the oracle under its second substitution (device_sqrt).  The pow branch: field within libm noise — a libm
    pow has no bit contract — and the triangle counts within 0.5 %.  Either way count + emit are bit-exact against the
    oracle's emit stage fed the device lattice.  (long_x's lines are sparse: isolevel 30.)"""
    from test_mc import bits_equal
    t = oracle_trace(oracle, name, False)
    s, p = solver(pkg, name, False, "default")
    try:
        s.steps(p, FRAMES)
        assert_state_equal(s.download(), t["frames"][-1], "state")
        sc, _, q, _ = G.make_geometry(name, False)
        o = oracle.Oracle(False, device_pow=True, device_sqrt=True)
        o.set_particles(**sc)
        for _ in range(FRAMES):
            o.step(q)
        half = mc.get("particle_influence", 0.5) == 0.5
        assert half == (oracle.OracleMc(**mc).particle_influence == 0.5)
        g = s.surface(p, pkg.McParams(**mc))
        w = o.surface(q, oracle.OracleMc(**mc))
        assert np.array_equal(g["sample"], w["sample"])
        if half:
            bits_equal(g["pn"], w["pn"], "pn")
            bits_equal(g["c"], w["c"], "c")
        else:
            tol = 2e-6
            np.testing.assert_allclose(g["pn"][:, 0], w["pn"][:, 0], rtol=tol, atol=tol * 100)
            assert np.array_equal(np.isnan(g["c"]), np.isnan(w["c"]))
            np.testing.assert_allclose(np.nan_to_num(g["pn"]), np.nan_to_num(w["pn"]), rtol=1e-4, atol=1e-4)
        e = o.surface(q, oracle.OracleMc(**mc), lattice=(g["sample"], g["pn"], g["c"]))
        assert len(e["vs"]) == len(g["vs"]) >= 3 * 4000
        for k in ("vs", "ns", "cs"):
            assert np.array_equal(g[k], e[k], equal_nan=True), k
        if half:
            assert len(g["vs"]) == len(w["vs"])
            for k in ("vs", "ns", "cs"):
                assert np.array_equal(g[k], w[k], equal_nan=True), k
        else:
            assert abs(len(g["vs"]) - len(w["vs"])) <= 0.005 * len(w["vs"]) + 30
    finally:
        s.close()
