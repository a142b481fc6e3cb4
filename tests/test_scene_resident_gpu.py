"""Sources, drains and cell queries on the device-resident path (pbf_set_sources / pbf_set_drains / pbf_stage_scene /
pbf_query_cells) against the oracle's restatement of ompsph.hpp:93-118,167-186 (Oracle.emit / drain / query): the same
particles in the same order with the same bits, the same query answers.  Small scenes only."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import scene_cases as S
from test_cli_gpu import BIN, read_ply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
ERR_INVALID, ERR_STATE = -1, -4


def make(pkg, oracle, sc, fp64, reserve=4096, options=()):
    s = pkg.Solver(h=S.H, fp64=fp64)
    for k, v in options:
        s.set_option(k, v)
    if reserve:
        s.reserve(reserve)
    s.upload(**sc)
    o = oracle.Oracle(fp64, device_pow=True)
    o.set_particles(**sc)
    return s, o, pkg.default_params(4, 1000.0), oracle.make_params(iteration=4, mode=oracle.JACOBI, sort=oracle.SORT_STABLE)


@BOTH
@pytest.mark.parametrize("graph", [0, 1])
def test_off_changes_no_bit(pkg, fp64, graph):
    sc = S.cubes_with_obstacle(pkg, fp64)
    p = pkg.default_params(4, 1000.0)
    runs = []
    for touched in (False, True):
        s = pkg.Solver(h=S.H, fp64=fp64).set_option("graph", graph).upload(**sc)
        if touched:
            s.set_sources(S.main_scene(sc)[0]).set_drains(S.main_scene(sc)[1]).set_sources([]).set_drains([])
        s.steps(p, 3).steps(p, 3)
        assert s.scene_host_syncs() == 0
        if graph:
            captured, replays, on = s.graph_stats()
            assert captured >= 1 and replays >= 1 and on
        runs.append(s.download())
    assert S.same(runs[0], runs[1])


@BOTH
def test_stage_scene_equals_oracle(pkg, oracle, fp64):
    sc = S.cubes_with_obstacle(pkg, fp64)
    sources, drains, _ = S.shim_scene(sc)
    s, o, p, q = make(pkg, oracle, sc, fp64)
    s.set_sources(sources).set_drains(drains).stage("scene", p)
    want = o.emit(sources).drain(drains).get_particles()
    assert s.n == len(want["id"]) and S.same(s.download(), want)


VARIANTS = [(), (("row_major", 0),), (("gather", 0),), (("split_build", 5),), (("fuse_predict", 0),), (("graph", 1),)]


@BOTH
@pytest.mark.parametrize("options", VARIANTS, ids=["default", "row_major0", "gather0", "split_build5", "fuse_predict0", "graph1"])
def test_free_running_equals_oracle(pkg, oracle, fp64, options):
    sc = S.cubes_with_obstacle(pkg, fp64)
    sources, drains = S.main_scene(sc)
    s, o, p, q = make(pkg, oracle, sc, fp64, options=options)
    s.set_sources(sources).set_drains(drains)
    for frame in range(6):
        s.steps(p, 1)
        S.oracle_frame(oracle, o, q, sources, drains)
        want = o.get_particles()
        assert s.n == len(want["id"]), frame
        assert S.same(s.download(), want), frame
    t, _, _, _ = make(pkg, oracle, sc, fp64, options=options)
    t.set_sources(sources).set_drains(drains).steps(p, 6)
    assert S.same(t.download(), want)
    assert 1 <= t.scene_host_syncs() <= 6
    # determinism: the same run again, the same bits
    u, _, _, _ = make(pkg, oracle, sc, fp64, options=options)
    u.set_sources(sources).set_drains(drains).steps(p, 6)
    assert S.same(u.download(), t.download())


def test_equals_advance(pkg, tmp_path):
    """the frame dumps of the shim's advance() (host/test_shim.cpp --dump) against the resident run of the same scene"""
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_shim"), "--dump", str(tmp_path)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "dumped" in r.stdout, r.stdout + r.stderr
    sc = S.cubes_with_obstacle(pkg)
    sources, drains, points = S.shim_scene(sc)
    s = pkg.Solver(h=S.H).reserve(4096).upload(**sc).set_sources(sources).set_drains(drains)
    p = pkg.default_params(4, 1000.0)
    rec = np.dtype([("id", "<u8"), ("type", "u1"), ("pos", "<f4", 3), ("vel", "<f4", 3), ("colour", "<f4", 4)])
    for frame in range(2):
        s.step(p)
        answers = s.query(p, points)
        g = s.download()
        raw = open(tmp_path / f"frame{frame}_particles.bin", "rb").read()
        w = np.frombuffer(raw[8:], rec)
        assert int(np.frombuffer(raw[:8], np.uint64)[0]) == len(w) == s.n
        assert S.same(g, w, ("id", "type", "pos", "vel", "colour")), frame
        qraw = np.frombuffer(open(tmp_path / f"frame{frame}_queries.bin", "rb").read(), np.uint64)
        at = 0
        for got in answers:
            k = int(qraw[at + 1])
            assert k == len(got) and np.array_equal(qraw[at + 2:at + 2 + k], got), frame
            at += 2 + k
        assert at == len(qraw)


@BOTH
def test_drain_boundary(pkg, oracle, fp64):
    dt = np.float64 if fp64 else np.float32
    ks = np.arange(1, 9)
    centre = (500.0, 500.0, 500.0)
    pos = np.array(centre) + ks[:, None] * np.array([3.0, 4.0, 0.0])
    pos = np.concatenate([pos, [[501.0, 500.0, 500.0]]])            # + an obstacle inside every sphere
    n = len(pos)
    sc = dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n, dt), pos=pos.astype(dt),
              vel=np.zeros((n, 3), dt), colour=np.full((n, 4), 0.5, dt))
    sc["type"][-1] = 1
    p = pkg.default_params(4, 1000.0)
    for k in ks:
        for width, gone in ((5.0 * k, False), (float(np.nextafter(dt(5.0 * k), dt(np.inf))), True)):
            # two overlapping drains: a particle both reach leaves once
            drains = [(centre, width), ((500.0, 500.0, 500.0), width)]
            s = pkg.Solver(h=S.H, fp64=fp64).upload(**sc).set_drains(drains).stage("scene", p)
            o = oracle.Oracle(fp64)
            o.set_particles(**sc)
            want = o.drain(drains).get_particles()
            got = s.download()
            assert S.same(got, want), (k, width)
            assert ((k - 1) in got["id"]) != gone and (n - 1) in got["id"]
            assert len(got["id"]) == n - (k - 1) - int(gone)


def far_obstacle(sc):
    """the scene plus one obstacle alone in a cell of its own, far from every fluid particle and from the inlets"""
    out = {k: np.concatenate([v, v[:1]]) for k, v in sc.items()}
    out["id"][-1], out["type"][-1] = 424242, 1
    out["pos"][-1] = (875.0, 125.0, 875.0)
    out["vel"][-1] = 0
    return out


@BOTH
def test_queries(pkg, oracle, fp64):
    sc = far_obstacle(S.cubes_with_obstacle(pkg, fp64))
    sources, drains, points = S.shim_scene(sc)
    lonely = tuple(float(v) for v in sc["pos"][-1])
    s, o, p, q = make(pkg, oracle, sc, fp64)
    counts = np.zeros(1, np.uint32)
    pt = np.array(points[0], np.float64)
    assert s.L.pbf_query_cells(s.ctx, C.byref(p), 1, pt.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), None,
                               0) == ERR_STATE
    s.set_sources(sources).set_drains(drains)
    for frame in range(2):
        s.step(p)
        o.emit(sources).drain(drains)
        o.predict(q).sort(q).grid_table(q)
        table, w = o.table(), o.get_particles()
        keys = o.keys()
        # more points, found on the oracle's own state: outside the grid, the last table cell, an obstacle-only cell, a
        # crowded cell
        ext, lo = o.extent()
        tn = len(table)
        sizes = np.diff(np.append(table, len(w["id"])))
        crowded = int(np.argmax(sizes[:-1]))

        def centre_of(code):
            xyz = [sum(((code >> (3 * b + a)) & 1) << b for b in range(10)) for a in range(3)]
            return tuple((float(lo[a]) + (xyz[a] + 0.5) * S.H) * S.SCALE for a in range(3))
        # order: the three points of the shim test, outside, last cell, the CROWDED cell (a middle row), obstacle only
        pts = list(points) + [(-5000.0, 100.0, 100.0), centre_of(tn - 1), centre_of(crowded), lonely]
        want = [o.query(q, pt) for pt in pts]
        assert len(want[3]) == 0 and len(want[4]) == 0 and len(want[5]) >= 2
        # the obstacle's cell holds the obstacle and nothing else, and the answer is empty
        at = int(np.nonzero(w["id"] == 424242)[0][0])
        assert w["type"][at] == 1 and (keys == keys[at]).sum() == 1 and int(keys[at]) + 1 < tn
        assert len(want[6]) == 0
        got = s.query(p, pts)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), frame
        # fewer slots than ids: the full count, the first `cap` ids, nothing beyond (in the row, in the next row, behind the end)
        cap = len(want[5]) - 1
        GUARD = np.uint64(0xABCDEF)
        buf = np.full((len(pts) + 1, cap), GUARD, np.uint64)          # one guard row behind the last point's
        cnt = np.zeros(len(pts), np.uint32)
        s._chk(s.L.pbf_query_cells(s.ctx, C.byref(p), len(pts), np.array(pts, np.float64).ctypes.data_as(C.c_void_p),
                                   cnt.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), cap), "pbf_query_cells")
        assert list(cnt) == [len(x) for x in want]
        for i, x in enumerate(want):
            k = min(len(x), cap)
            assert np.array_equal(buf[i, :k], x[:k]), (frame, i)
            assert (buf[i, k:] == GUARD).all(), (frame, i)
        assert (buf[-1] == GUARD).all()
        o.diffuse(q)
        for _ in range(4):
            o.lambda_(q).delta(q)
        o.finalise(q)


@BOTH
def test_query_with_another_grid_is_refused(pkg, fp64):
    sc = S.cubes_with_obstacle(pkg, fp64)
    p = pkg.default_params(4, 1000.0)
    s = pkg.Solver(h=S.H, fp64=fp64).upload(**sc).step(p)
    pts = [tuple(float(v) for v in sc["pos"][100]), (1500.0, 1500.0, 1500.0)]
    good = s.query(p, pts)
    size, ext, table = s.L.pbf_table_size(s.ctx), s.extent(), s.table()
    for change in ("bigger", "smaller", "scale", "shifted"):
        r = p.copy()
        if change == "bigger":
            r.max_bound[0] = r.max_bound[1] = r.max_bound[2] = 2000.0
        elif change == "smaller":
            r.max_bound[0] = 600.0
        elif change == "scale":
            r.scale = 400.0
        else:
            for a in range(3):
                r.min_bound[a], r.max_bound[a] = 50.0, 1050.0
        arr, cnt = np.array(pts, np.float64), np.full(2, 77, np.uint32)
        ids = np.full((2, 8), 0xABCDEF, np.uint64)
        rc = s.L.pbf_query_cells(s.ctx, C.byref(r), 2, arr.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p),
                                 ids.ctypes.data_as(C.c_void_p), 8)
        assert rc == ERR_STATE, change
        assert (cnt == 77).all() and (ids == 0xABCDEF).all()
        assert s.L.pbf_table_size(s.ctx) == size
        e2 = s.extent()
        assert np.array_equal(e2[0], ext[0]) and np.array_equal(e2[1], ext[1])
        assert np.array_equal(s.table(), table)
    for a, b in zip(s.query(p, pts), good):            # and the context still answers for its own grid
        assert np.array_equal(a, b)


@BOTH
def test_capacity(pkg, oracle, fp64):
    sc = S.cubes_with_obstacle(pkg, fp64)
    sources = S.main_scene(sc)[0]
    p = pkg.default_params(4, 1000.0)
    s = pkg.Solver(h=S.H, fp64=fp64).upload(**sc).set_sources(sources)
    before = s.download()
    for _ in range(2):
        assert s.L.pbf_step(s.ctx, C.byref(p)) == ERR_INVALID
        assert b"pbf_reserve" in s.L.pbf_last_error(s.ctx)
        assert s.n == 2000 and S.same(s.download(), before)
    assert s.L.pbf_stage_scene(s.ctx, C.byref(p)) == ERR_INVALID
    s, o, p, q = make(pkg, oracle, sc, fp64, reserve=2000 + 28 * S.GROWTH_FRAMES)
    s.set_sources(sources)
    for frame in range(S.GROWTH_FRAMES):
        s.step(p)
        S.oracle_frame(oracle, o, q, sources, [])
        assert S.same(s.download(), o.get_particles()), frame
    assert s.n == 2000 + 28 * S.GROWTH_FRAMES > 2048
    assert s.scene_host_syncs() == 0                     # sources only: nothing to read back
    # the reserve is exhausted to the particle: the next step is refused, the state stays
    before = s.download()
    assert s.L.pbf_step(s.ctx, C.byref(p)) == ERR_INVALID
    assert s.n == 2000 + 28 * S.GROWTH_FRAMES and S.same(s.download(), before)


def test_growth_with_extras_on(pkg, oracle):
    """fp64, surface tension + XSPH + vorticity on while the count grows across 2048 = 8 x 256: every per-particle buffer of
    the extras (sized at upload) must cover the grown set.
    (a) XSPH + vorticity: the resident run equals the oracle bit for bit, frame by frame (as
        tests/test_hip_parity.py::test_xsph_vorticity_bit_exact holds them).
    (b) with surface tension as well (it runs last and changes velocities only): every frame starts the oracle from the
        resident state before it; ids, positions and colours equal the oracle's frame bit for bit, and the velocity
        difference to the oracle's (XSPH + vorticity, no surface tension) equals the all-pairs restatement's increment
        (tests/surface_tension_ref.py) to 1e-12 relative, the record {n, rho} too — the check and the tolerance of
        tests/test_surface_tension_gpu.py::test_passes_equal_all_pairs_restatement.
    (c) the same run equals the same solver fed a fresh upload of the emitted set each frame, bit for bit."""
    import nversion as NV
    import surface_tension_ref as ST
    GAMMA, BETA = 0.05, 0.5
    sc = S.cubes_with_obstacle(pkg, True)
    sources = S.main_scene(sc)[0]
    cap = 2000 + 28 * S.GROWTH_FRAMES
    # (a)
    s, o, p, q = make(pkg, oracle, sc, True, reserve=cap)
    p.xsph = p.vorticity = q.xsph = q.vorticity = 1
    s.set_sources(sources)
    for frame in range(S.GROWTH_FRAMES):
        s.step(p)
        S.oracle_frame(oracle, o, q, sources, [])
        assert S.same(s.download(), o.get_particles()), frame
    assert s.n > 2048
    # (b), (c)
    s = pkg.Solver(h=S.H, fp64=True).set_surface_tension(GAMMA, BETA).reserve(cap).upload(**sc).set_sources(sources)
    state, crossed = sc, False
    for frame in range(S.GROWTH_FRAMES):
        s.step(p)
        got = s.download()
        o = oracle.Oracle(True, device_pow=True)
        o.set_particles(**state)
        emitted = o.emit(sources).get_particles()
        o.predict(q).sort(q).grid_table(q)
        predicted = o.pstar()[:, :3].astype(np.float64)
        o.diffuse(q)
        for _ in range(4):
            o.lambda_(q).delta(q)
        o.finalise(q)                                  # (+ vorticity confinement and XSPH: q carries the switches)
        w = o.get_particles()
        assert S.same(got, w, ("id", "type", "mass", "pos", "colour")), frame
        cells = NV.predict_cells(predicted, S.H, p.scale, list(p.min_bound))
        ps = s.pstar()[:, :3].astype(np.float64)
        assert np.array_equal(ps, o.pstar()[:, :3])
        obstacle = got["type"] == 1
        dv, rho, nrm = ST.delta_v(ps, got["mass"].astype(np.float64), S.H, p.dt, GAMMA, BETA, obstacle, cells)
        st = s.surface_state()
        assert np.abs(st[:, 3] - rho).max() <= 1e-12 * rho.max(), frame
        assert np.abs(st[:, :3] - nrm).max() <= 1e-12 * np.abs(nrm).max(), frame
        err = np.abs((got["vel"] - w["vel"]) - dv).max()
        print("frame", frame, "n", s.n, "surface-tension dv error / max", err / np.abs(dv).max())
        assert np.abs(dv).max() > 0 and err <= 1e-12 * np.abs(dv).max(), frame
        assert np.array_equal(got["vel"][obstacle], w["vel"][obstacle])
        t = pkg.Solver(h=S.H, fp64=True).set_surface_tension(GAMMA, BETA).upload(**emitted)
        assert S.same(got, t.step(p).download()), frame
        crossed = crossed or (len(state["id"]) <= 2048 < s.n)
        state = got
    assert crossed and s.n > 2048


@BOTH
def test_depletion_and_refill(pkg, oracle, fp64):
    sc = S.cubes_with_obstacle(pkg, fp64)
    sc["type"][7] = 0
    sources = S.main_scene(sc)[0][:1]
    everything = [((500.0, 500.0, 500.0), 5000.0)]
    s, o, p, q = make(pkg, oracle, sc, fp64)
    s.set_sources(sources).set_drains(everything)
    for _ in range(2):
        s.step(p)
        S.oracle_frame(oracle, o, q, sources, everything)
        assert s.n == 0 == o.n and len(s.download()["id"]) == 0
    s.set_drains([])
    for frame in range(2):
        s.steps(p, 1)
        S.oracle_frame(oracle, o, q, sources, [])
        assert s.n == 16 * (frame + 1) and S.same(s.download(), o.get_particles())


def test_read_backs(pkg):
    sc = S.cubes_with_obstacle(pkg)
    sources, drains = S.main_scene(sc)
    p = pkg.default_params(4, 1000.0)
    s = pkg.Solver(h=S.H).reserve(4096).upload(**sc).set_sources(sources)
    s.steps(p, 3)
    assert s.scene_host_syncs() == 0
    s.set_drains(drains)
    for k in range(1, 4):
        s.step(p)
        assert s.scene_host_syncs() <= k
    assert s.scene_host_syncs() >= 1
    s.steps(p, 4)
    assert s.scene_host_syncs() <= 7


def test_refusals(pkg):
    from pbf_sph_amd import capi
    sc = S.cubes_with_obstacle(pkg)
    sources, drains = S.main_scene(sc)
    s = pkg.Solver(h=S.H).reserve(4096).upload(**sc).set_sources(sources).set_drains(drains)
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(pkg.PbfError):
            s.set_sources([(1, (0, 0, 0), (0, 0, 0), S.RED, bad)])
        with pytest.raises(pkg.PbfError):
            s.set_drains([((0, 0, 0), bad)])
    assert s.L.pbf_set_sources(s.ctx, 2, None) == ERR_INVALID and s.L.pbf_set_drains(s.ctx, 1, None) == ERR_INVALID
    # the settings are unchanged: the run equals one that never saw the bad calls
    t = pkg.Solver(h=S.H).reserve(4096).upload(**sc).set_sources(sources).set_drains(drains)
    p = pkg.default_params(4, 1000.0)
    assert S.same(s.steps(p, 2).download(), t.steps(p, 2).download())
    # slab mode: refused on an attached context; pbf_slab_step refuses while one is set
    L = s.L
    noop = capi.EXCHANGE_FN(lambda *a: 0)
    comm = C.c_void_p()
    assert L.pbf_comm_create_host_callback(noop, None, 1, 0, C.byref(comm)) == 0
    cuts = np.array([0, 1024], np.uint32)
    u = pkg.Solver(h=S.H).reserve(8192).upload(**sc).set_drains(drains)
    assert L.pbf_slab_attach(u.ctx, comm, cuts.ctypes.data_as(C.c_void_p), 256, 256) == 0
    assert L.pbf_slab_step(u.ctx, C.byref(p)) == ERR_STATE
    d = (capi.Drain * 1)()
    d[0].width = 1.0
    assert L.pbf_set_drains(u.ctx, 1, C.byref(d)) == ERR_STATE
    src = (capi.Source * 1)()
    assert L.pbf_set_sources(u.ctx, 1, C.byref(src)) == ERR_STATE
    assert L.pbf_set_drains(u.ctx, 0, None) == 0           # clearing is always allowed
    pt, cnt = np.zeros(3), np.zeros(1, np.uint32)
    assert L.pbf_query_cells(u.ctx, C.byref(p), 1, pt.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), None, 0) == ERR_STATE
    u.close()
    L.pbf_comm_destroy(comm)


def test_cli_resident_equals_advance(tmp_path):
    common = ["--scene", "dam-break", "--particles", "8192", "--solver-iter", "4", "-n", "6", "-w", "0", "--no-surface", "--json",
              "--source=550,150,550,0,2,0,16,777", "--source=300,300,300,1,0,0,10", "--drain=265,650,265,120"]
    out = {}
    for mode in ("resident", "advance"):
        args = [BIN, *common, "-o", str(tmp_path / mode)] + (["--resident"] if mode == "resident" else [])
        r = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        j = json.loads([l for l in r.stdout.split("\n") if l.startswith("{")][0])
        assert f"Final Particle count : {j['particles']} " in r.stdout
        out[mode] = (j["particles"], open(tmp_path / mode / "cloud.ply", "rb").read())
    assert out["resident"][0] == out["advance"][0]
    # both inlets emit every frame (16 + 12 particles): anything below that total left through the drain
    assert out["resident"][0] < 8192 + 6 * 28
    assert out["resident"][1] == out["advance"][1]
    assert len(read_ply(str(tmp_path / "resident" / "cloud.ply"))) == out["resident"][0]
    r = subprocess.run([BIN, *common, "--slabs", "2", "-o", ""], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "single-device" in r.stderr


def test_shim_resident_scene():
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_scene_shim")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
    for name in ("scene_resident_count", "scene_resident_equals_advance", "scene_resident_queries", "scene_resident_stepwise",
                 "scene_resident_cleared"):
        assert f"ok {name}" in r.stdout, r.stdout
