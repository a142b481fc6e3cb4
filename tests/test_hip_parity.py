"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle in Jacobi /
stable-sort mode on the same inputs, stage by stage and end to end.

Bars (north_star: "within a stated float tolerance"; integer work bit-exact):

  A. BIT-EXACT, fp32 and fp64, every stage and free-running over many frames, against the oracle
     with `device_pow=True`.  The default (precise) device build uses IEEE divide/sqrt, no FMA
     contraction and the oracle's candidate order, so the ONLY arithmetic substitution is
     pow(q, 4) -> (q*q)*(q*q) (CorrN = 4 is a compile-time constant, sph_constants.h:16); the
     oracle can evaluate that form too, and then every bit agrees: keys, cell table, sorted
     permutation, colours, lambda, pStar, positions, velocities.
  B. TOLERANCE against the oracle with the reference's std::pow (ompsph.hpp:240): one step from a
     settled state <= 1e-3 world units (box = 1000), from the over-dense start lattice (1.84x rest
     density: a violent first frame that amplifies last-bit differences) <= 5e-3.
     No max-norm claims over several free-running frames: near-coincident pairs make the step
     ill-conditioned; statistics only.
  C. PBF_FLAG_FAST_MATH (v_rsq + FMAs, the analogue of the reference's own -Ofast / native_divide
     builds): <= 5e-3 world units per step from a settled state.

Parity vs the *reference binary* is unpinned for the floating-point stages (oracle/pbf_oracle.h).
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("id", "type", "mass", "pos", "vel", "colour")


def by_id(d):
    o = np.argsort(d["id"], kind="stable")
    return {k: v[o] for k, v in d.items()}


def mk(pkg, oracle, scene, fp64, flags=0, device_pow=True, gather=None):
    """gather=None leaves the PRODUCT DEFAULT (filtered lists, split_build 8, cell_diffuse 1); a variant is
    only selected where a test names it."""
    s = pkg.Solver(h=0.1, fp64=fp64, flags=flags)
    if gather == "morton":
        s.set_option("row_major", 0)
    elif gather is not None:
        s.set_option("gather", gather)
    s.upload(**scene)
    o = oracle.Oracle(fp64, device_pow=device_pow)
    o.set_particles(**scene)
    return s, o


_ORACLE_RUNS = {}


def oracle_run(oracle, key, scene, fp64, q, frames, device_pow=True):
    """The oracle's states after the given frames (0-based, last one = number of steps - 1) of a free run from `scene`,
    computed once per key and shared by the tests that compare different GPU kernels against the same run (the CPU
    oracle is what a parity test spends its time in)."""
    if key not in _ORACLE_RUNS:
        o = oracle.Oracle(fp64, device_pow=device_pow)
        o.set_particles(**scene)
        got = {}
        for frame in range(max(frames) + 1):
            o.step(q)
            if frame in frames:
                got[frame] = {k: np.array(v, copy=True) for k, v in o.get_particles().items()}
        _ORACLE_RUNS[key] = got
    return _ORACLE_RUNS[key]


def params_pair(pkg, oracle, iteration=4, side=1000.0, wells=None):
    p = pkg.default_params(iteration, side)
    if wells is not None:
        p.set_wells(wells)
    q = oracle.make_params(iteration=iteration, max_bound=(side, side, side), mode=oracle.JACOBI,
                           sort=oracle.SORT_STABLE, wells=wells)
    return p, q


def get_scene(pkg, name, fp64):
    if name == "cubes8192":
        return pkg.scene_cubes(8192, fp64), 1000.0
    if name == "cubes1024":
        return pkg.scene_cubes(1024, fp64), 1000.0
    if name == "dam8192":
        return pkg.scene_dambreak(8192, fp64)
    raise KeyError(name)


def assert_state_equal(g, w, what=""):
    for k in FIELDS:
        assert np.array_equal(g[k], w[k]), (what, k, np.abs(g[k].astype(np.float64) - w[k]).max())


SCENES = ["cubes8192", "dam8192"]


@pytest.fixture(params=["default", "morton", "global", "tiles"])
def variant(request):
    """The gather kernels must all be bit-identical to the oracle: None = the product default (neighbour lists: quantised
    build with lambda riding on it + list-driven delta-p, on the ROW-MAJOR copy of the iterations' working set — option
    row_major = 1, csrc/pbf_kernels.hpp RowArrays; per-cell diffuse), "morton" = the same kernels' Morton-order forms
    (row_major = 0: what slabs with options, hipGraph replay and the other split_build values run), 0 = per-particle
    global walk, 3 = the iteration per brick out of LDS tiles (pbf_tiles.hpp)."""
    return {"default": None, "morton": "morton", "global": 0, "tiles": 3}[request.param]

# ------------------------------------------------------------------------------------------ A


@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("scene", SCENES)
def test_every_stage_bit_exact(pkg, oracle, scene, fp64, variant):
    sc, side = get_scene(pkg, scene, fp64)
    s, o = mk(pkg, oracle, sc, fp64, gather=variant)
    p, q = params_pair(pkg, oracle, side=side)
    for _ in range(2):  # leave the lattice first
        s.step(p)
        o.step(q)
    assert_state_equal(s.download(), o.get_particles(), "warm frames")
    s.stage("predict", p)
    o.predict(q)
    assert np.array_equal(s.keys().astype(np.uint64), o.keys())
    assert np.array_equal(s.pstar()[:, :3], o.pstar())
    s.stage("sort", p)
    o.sort(q).grid_table(q)
    assert np.array_equal(s.keys().astype(np.uint64), o.keys())
    assert np.all(np.diff(s.keys().astype(np.int64)) >= 0)
    assert np.array_equal(s.table().astype(np.uint64), o.table())
    e, m = s.extent()
    eo, mo = o.extent()
    assert np.array_equal(e, eo) and np.array_equal(m, mo.astype(np.float64))
    assert_state_equal(s.download(), o.get_particles(), "sort")  # stable sort => identical permutation
    assert np.array_equal(s.pstar()[:, :3], o.pstar())
    s.stage("diffuse", p)
    o.diffuse(q)
    assert np.array_equal(s.download()["colour"], o.get_particles()["colour"])
    for it in range(4):
        s.stage("lambda", p)
        o.lambda_(q)
        assert np.array_equal(s.pstar()[:, 3], o.lambdas()), it
        s.stage("delta", p)
        o.delta(q)
        assert np.array_equal(s.pstar()[:, :3], o.pstar()), it
    s.stage("finalise", p)
    o.finalise(q)
    assert_state_equal(s.download(), o.get_particles(), "finalise")


@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("scene", SCENES)
def test_free_running_bit_exact(pkg, oracle, scene, fp64, variant):
    """12 frames without re-seeding: GPU state == oracle(device_pow) state, bit for bit."""
    if variant not in (None, "morton") and (scene == "cubes8192" or (fp64 and variant == 0)):
        pytest.skip("alternative gather kernels run the dam-break scene (the plain walk in fp32 only): suite time")
    sc, side = get_scene(pkg, scene, fp64)
    s, _ = mk(pkg, oracle, sc, fp64, gather=variant)
    p, q = params_pair(pkg, oracle, side=side)
    want = oracle_run(oracle, ("free", scene, fp64), sc, fp64, q, (0, 2, 11))
    for frame in range(12):
        s.step(p)
        if frame in want:
            assert_state_equal(s.download(), want[frame], f"frame {frame}")


@pytest.mark.parametrize("split,fp64", [(0, False), (4, False), (5, False), (8, False), (5, True), (8, True)])
def test_split_build_bit_exact(pkg, oracle, split, fp64):
    """Option split_build: 0 = lambda builds the neighbour lists while it gathers; 4 / 5 = a list-build launch of
    its own (k_build_lists_op with nothing riding: ListOnlyOp, 2 / 4 pair loads per trip) followed by a list-driven
    lambda; 8 (default) = the same kernel with lambda riding on its flushes (k_build_lists_op<LambdaOp>).  Same
    candidates in the same order either way — identical bits, obstacles and overflow rows included."""
    sc, side = get_scene(pkg, "dam8192", fp64)
    sc = {k: v.copy() for k, v in sc.items()}
    sc["type"][::13] = 1
    s, _ = mk(pkg, oracle, sc, fp64, gather=1)
    s.set_option("split_build", split)
    p, q = params_pair(pkg, oracle, side=side)
    want = oracle_run(oracle, ("split", fp64), sc, fp64, q, (0, 5))
    for frame in range(6):
        s.step(p)
        if frame in want:
            assert_state_equal(s.download(), want[frame], f"frame {frame}")


@pytest.mark.parametrize("cell", [0, 1])
def test_cell_diffuse_bit_exact(pkg, oracle, cell):
    """Option cell_diffuse (default 1): all particles of a cell share one colour walk (k_diffuse_bricks +
    k_diffuse_apply) — the same running sums, so the same bits as one walk per particle (0), with and
    without obstacles (which force the per-cell global walk)."""
    for obstacles in (False, True):
        sc, side = get_scene(pkg, "dam8192", False)
        sc = {k: v.copy() for k, v in sc.items()}
        sc["colour"][::3] = (0.9, 0.2, 0.1, 0.5)  # something to diffuse
        if obstacles:
            sc["type"][::13] = 1
        s, o = mk(pkg, oracle, sc, False, gather=1)
        s.set_option("cell_diffuse", cell)
        p, q = params_pair(pkg, oracle, side=side)
        for frame in range(5):
            s.step(p)
            o.step(q)
        assert_state_equal(s.download(), o.get_particles(), f"cell={cell} obstacles={obstacles}")


@pytest.mark.parametrize("fp64,row_diffuse,cap", [(False, 1, 0), (False, 1, 24), (False, 0, 0), (True, 1, 0), (True, 1, 1)])
def test_row_diffuse_bit_exact(pkg, oracle, fp64, row_diffuse, cap):
    """Option row_diffuse (default 1, with row_major): the colour walk per cell on the row-major copy, one wave per 64-cell
    x-segment, runs staged through an LDS tile by LDS-DMA, sums applied in place (k_diffuse_rows).  Same candidates in the
    same order as the reference walk => the same bits as the oracle, and as the Morton-order per-cell walk (row_diffuse 0).
    cap = the tile in records: 24 and 1 force the walk-from-memory path for most / all rows.  With and without obstacles
    (skipped as candidates, unchanged as walkers) and with colours that differ per particle."""
    rng = np.random.default_rng(7)
    for obstacles in (False, True):
        sc, side = get_scene(pkg, "dam8192", fp64)
        sc = {k: v.copy() for k, v in sc.items()}
        sc["colour"][:] = rng.uniform(0.03, 1.0, sc["colour"].shape).astype(sc["colour"].dtype)
        if obstacles:
            sc["type"][::13] = 1
        s, o = mk(pkg, oracle, sc, fp64)
        s.set_option("row_diffuse", row_diffuse)
        s.set_option("diffuse_cap", cap)
        p, q = params_pair(pkg, oracle, side=side)
        for frame in range(4):
            s.step(p)
            o.step(q)
            assert_state_equal(s.download(), o.get_particles(), f"row_diffuse={row_diffuse} cap={cap} obstacles={obstacles} frame {frame}")


@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("pipeline", [0, 1])
def test_pipelined_readers_bit_exact(pkg, oracle, pipeline, fp64):
    """Option pipeline: software-pipelined list-driven lambda / delta-p (default: fp64 only) — same candidates in the same
    order, so identical bits either way, obstacles and overflowing rows (the pile) included."""
    sc, side = get_scene(pkg, "dam8192", fp64)
    sc = {k: v.copy() for k, v in sc.items()}
    sc["type"][::13] = 1
    sc["pos"][:300] = sc["pos"][0] + (np.arange(300)[:, None] % 7) * 0.5   # > 160 neighbours: rows overflow, particles walk
    s, o = mk(pkg, oracle, sc, fp64)
    s.set_option("pipeline", pipeline)
    p, q = params_pair(pkg, oracle, side=side)
    # the pile really overflows its rows (so the readers' walking fallback is what is being compared): the first list
    # build of the run marks more than 160 survivors as NBR_OVERFLOW
    probe = pkg.Solver(h=0.1, fp64=fp64)
    probe.set_option("pipeline", pipeline)
    probe.upload(**sc).stage("predict", p).stage("sort", p).stage("lambda", p)
    assert (probe.nbr_counts() == 0xFFFFFFFF).sum() >= 100
    for frame in range(4):
        s.step(p)
        o.step(q)
    assert_state_equal(s.download(), o.get_particles())


def two_tier_scene(pkg):
    """dam8192 (fp32) with 1 500 particles at ~1.3x the lattice's density and a pile of 300: lists within the 40-slot rows,
    lists that spill into a chunk (41..160 survivors) and lists beyond 160 (NBR_OVERFLOW)."""
    sc, side = get_scene(pkg, "dam8192", False)
    sc = {k: v.copy() for k, v in sc.items()}
    rng = np.random.default_rng(23)
    sc["pos"][:1500] = sc["pos"][4000] + rng.random((1500, 3)).astype(np.float32) * np.float32(95.0)   # ~1.3x the lattice's density
    sc["pos"][1500:1800] = sc["pos"][0] + (np.arange(300)[:, None] % 7) * 0.5                         # a pile: > 160 neighbours
    return sc, side


@pytest.mark.parametrize("split,pipeline,chunks", [(8, 0, 0), (8, 1, 0), (5, 0, 0), (0, 0, 0), (8, 0, 3), (8, 0, 1)])
def test_two_tier_lists_bit_exact(pkg, oracle, split, pipeline, chunks):
    """The neighbour lists keep 40 slots per particle in [block][slot][thread] rows and take a 120-slot chunk from a pool for
    the few longer ones (NbrLists, csrc/pbf_kernels.hpp).  A scene with all three kinds of particle — lists within the rows,
    lists that spill into a chunk (41..160 survivors), lists beyond 160 (NBR_OVERFLOW: the particle walks) — through every
    writer (split_build 8 / 5 / 0) and both readers; and with a pool of 3 chunks / 1 chunk, which most spilling particles
    find empty (they walk instead): identical bits every time."""
    sc, side = two_tier_scene(pkg)
    p, q = params_pair(pkg, oracle, side=side)
    probe = pkg.Solver(h=0.1)
    if chunks:
        probe.set_option("nbr_chunks", chunks)
    probe.set_option("split_build", split)
    probe.upload(**sc).stage("predict", p).stage("sort", p).stage("lambda", p)
    cnt = probe.nbr_counts()
    spill = ((cnt > 40) & (cnt <= 160)).sum()
    over = (cnt == 0xFFFFFFFF).sum()
    if chunks:
        assert spill <= chunks and over >= 200, (spill, over)     # the pool ran dry: the others walk
    else:
        assert spill >= 200 and over >= 100 and (cnt <= 40).sum() >= 1000, (spill, over)
    s = pkg.Solver(h=0.1)
    if chunks:
        s.set_option("nbr_chunks", chunks)
    s.set_option("split_build", split).set_option("pipeline", pipeline)
    s.upload(**sc)
    want = oracle_run(oracle, ("twotier",), sc, False, q, (0, 2))
    for frame in range(3):
        s.step(p)
        if frame in want:
            assert_state_equal(s.download(), want[frame], f"frame {frame}")


def test_list_builders_agree(pkg, oracle):
    """Every list builder applies ONE candidate filter (QuantFilter, csrc/pbf_kernels.hpp): on the two-tier scene the list
    lengths after the first build are the same whichever kernel wrote them — the Morton build with lambda riding
    (split_build 8) or with nothing riding (5 and 4; staging depths 16 and 24 too), the row-major build (the default: the same
    multiset, since its counts come back in row-slot order) and the tile build (gather 3: a list of at most 40 entries, or
    NBR_OVERFLOW — its rows have no second tier).

    nbr_chunks = one chunk per particle: on this scene some 4 300 lists spill beyond their 40 row slots and 2 000 more pass
    160, each of them takes a ticket, and the default pool holds n / 8 + 1024 = 2 048 chunks.  Which lanes find it empty (and
    are marked NBR_OVERFLOW whatever their length) is decided by the order of their atomics, so with the default pool two
    builds by the very same kernel disagree in a few hundred marks; a pool nobody finds empty leaves the filter alone to
    decide what is read back.  (test_two_tier_lists_bit_exact covers the pool that runs dry.)"""
    sc, side = two_tier_scene(pkg)
    p, _ = params_pair(pkg, oracle, side=side)

    def counts(**options):
        s = pkg.Solver(h=0.1)
        s.set_option("nbr_chunks", len(sc["id"]))
        for k, v in options.items():
            s.set_option(k, v)
        s.upload(**sc).stage("predict", p).stage("sort", p).stage("lambda", p)
        return s.nbr_counts()

    ref = counts(row_major=0, split_build=8)
    over = ref == 0xFFFFFFFF
    print("lists within the rows / spilled / overflowing:", int((ref <= 40).sum()), int(((ref > 40) & (ref <= 160)).sum()), int(over.sum()))
    # (all three kinds of list are there, as in test_two_tier_lists_bit_exact: nothing below holds vacuously)
    assert (ref <= 40).sum() >= 1000 and ((ref > 40) & (ref <= 160)).sum() >= 200 and over.sum() >= 100
    for options in ({"split_build": 5}, {"split_build": 4}, {"split_build": 5, "list_max": 16}, {"split_build": 5, "list_max": 24}):
        got = counts(row_major=0, **options)
        assert np.array_equal(got, ref), (options, int((got != ref).sum()))
    rows = counts()
    assert np.array_equal(np.sort(rows), np.sort(ref)), "row-major build"
    tiles = counts(row_major=0, gather=3)
    assert np.array_equal(tiles, np.where(ref <= 40, ref, 0xFFFFFFFF).astype(ref.dtype)), "tile build"


def test_no_lds_flag_bit_exact(pkg, oracle):
    """PBF_FLAG_NO_LDS: every gather stage (diffuse included) is the plain one-lane-per-particle walk."""
    sc, side = get_scene(pkg, "dam8192", False)
    s, o = mk(pkg, oracle, sc, False, flags=pkg.FLAG_NO_LDS, gather=1)
    p, q = params_pair(pkg, oracle, side=side)
    for frame in range(4):
        s.step(p)
        o.step(q)
    assert_state_equal(s.download(), o.get_particles())


def test_fused_diffuse_bit_exact(pkg, oracle):
    """Option fuse_diffuse: the colour diffusion rides on the first lambda launch's walk (same candidates,
    same order) — identical bits, obstacles included."""
    sc, side = get_scene(pkg, "cubes8192", False)
    sc = {k: v.copy() for k, v in sc.items()}
    sc["type"][::11] = 1
    s, o = mk(pkg, oracle, sc, False, flags=pkg.FLAG_STAGE_TIMING, gather=1)
    s.set_option("fuse_diffuse", 1)
    p, q = params_pair(pkg, oracle, side=side)
    for frame in range(4):
        s.step(p)
        o.step(q)
    assert_state_equal(s.download(), o.get_particles())
    # the fused launch really happened: no diffuse stage of its own was ever bracketed
    t = s.stage_times()
    assert t["sph-diffuse"][1] == 0 and t["sph-lambda"][1] == 16, t


def test_moving_box_bit_exact(pkg, oracle, variant):
    """benchmark.cpp:33,47: every frame runs with applyMotionSinXCosZ(param, frame); the grid (and
    its table length) moves with the box."""
    sc, side = get_scene(pkg, "cubes8192", False)
    s, o = mk(pkg, oracle, sc, False, gather=variant)
    base, q = params_pair(pkg, oracle, side=side)
    sizes = set()
    for frame in range(6):
        p = pkg.apply_motion(base, frame, False)
        off = oracle.motion_offset(frame, False)
        q.min_bound[:] = [float(np.float32(0) + np.float32(v)) for v in off]
        q.max_bound[:] = [float(np.float32(1000) + np.float32(v)) for v in off]
        assert list(p.min_bound) == list(q.min_bound) and list(p.max_bound) == list(q.max_bound)
        s.step(p)
        o.step(q)
        assert len(s.table()) == len(o.table())
        sizes.add(len(o.table()))
        assert_state_equal(s.download(), o.get_particles(), f"frame {frame}")


def test_edge_cases_bit_exact(pkg, oracle, variant):
    p, q = params_pair(pkg, oracle)
    s = pkg.Solver(h=0.1)
    if variant == "morton":
        s.set_option("row_major", 0)
    elif variant is not None:
        s.set_option("gather", variant)
    # empty: "Particles depleted" (ompsph.hpp:122-126) — a no-op, not an error
    z = dict(id=np.zeros(0, np.uint64), type=np.zeros(0, np.uint8), mass=np.zeros(0, np.float32),
             pos=np.zeros((0, 3), np.float32), vel=np.zeros((0, 3), np.float32), colour=np.zeros((0, 4), np.float32))
    s.upload(**z).step(p).sync()
    assert s.n == 0 and len(s.download()["id"]) == 0
    # single particle: free fall
    one = dict(id=[7], type=[0], mass=[1.0], pos=[[500, 500, 500]], vel=[[0, 0, 0]], colour=[[0.5, 0.5, 0.5, 1]])
    s.upload(**one).step(p)
    o = oracle.Oracle(False, device_pow=True)
    o.set_particles(**one)
    o.step(q)
    assert_state_equal(s.download(), o.get_particles(), "single")
    # ragged: 300 particles piled into ONE cell + particles far outside the grid (in no cell,
    # sph.hpp:206) + particles exactly on the bounds + exact duplicates (r = 0 between different ids)
    rng = np.random.default_rng(5)
    pile = (rng.random((300, 3)) * 40 + 480).astype(np.float32)
    outside = np.array([[5000, 500, 500], [500, -4000, 500], [900, 900, 30000]], np.float32)
    onb = np.array([[0, 0, 0], [1000, 1000, 1000], [0, 1000, 500], [0, 1000, 500]], np.float32)
    pos = np.concatenate([pile, outside, onb])
    n = len(pos)
    rag = dict(id=np.arange(n)[::-1].copy(), type=np.zeros(n, np.uint8), mass=np.ones(n, np.float32), pos=pos,
               vel=(rng.random((n, 3)).astype(np.float32) - 0.5), colour=rng.random((n, 4)).astype(np.float32))
    s.upload(**rag)
    o.set_particles(**rag)
    for frame in range(3):
        s.step(p)
        o.step(q)
        g, w = s.download(), o.get_particles()
        assert np.isfinite(g["pos"]).all()
        assert_state_equal(g, w, f"ragged frame {frame}")


def test_obstacles_and_wells_bit_exact(pkg, oracle, variant):
    """Obstacles follow the OpenCL backend (ocl/oclsph.cpp:66-69): fixed, lambda = 0, still
    neighbours.  Wells: ompsph.hpp:141-148."""
    sc, side = get_scene(pkg, "cubes1024", False)
    sc = {k: v.copy() for k, v in sc.items()}
    sc["type"][::7] = 1
    wells = [[300.0, 100.0, 300.0, 5000.0], [700.0, 50.0, 650.0, -2000.0]]
    s, o = mk(pkg, oracle, sc, False, gather=variant)
    p, q = params_pair(pkg, oracle, side=side, wells=wells)
    for frame in range(3):
        s.step(p)
        o.step(q)
        assert_state_equal(s.download(), o.get_particles(), f"frame {frame}")
    g = by_id(s.download())
    obs = g["type"] == 1
    assert obs.sum() > 100
    orig = by_id(sc)
    assert np.array_equal(g["pos"][obs], orig["pos"][obs]) and np.array_equal(g["vel"][obs], orig["vel"][obs])


def test_tile_overflow_falls_back_bit_exact(pkg, oracle):
    """gather = 3: a brick whose halo holds more records than the LDS tile takes the in-kernel global path (its rows
    then hold global indices, every kernel of the iteration takes the same decision); neighbours of that brick stay
    tiled.  5000 particles inside 3x3x3 cells force it."""
    rng = np.random.default_rng(11)
    pile = (rng.random((5000, 3)) * 140 + 430).astype(np.float32)
    far = (rng.random((3000, 3)) * 900 + 50).astype(np.float32)
    pos = np.concatenate([pile, far])
    n = len(pos)
    sc = dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n, np.float32), pos=pos,
              vel=np.zeros((n, 3), np.float32), colour=rng.random((n, 4)).astype(np.float32))
    s, o = mk(pkg, oracle, sc, False, gather=3)
    p, q = params_pair(pkg, oracle, iteration=2)
    s.step(p)
    o.step(q)
    assert_state_equal(s.download(), o.get_particles())


@pytest.mark.parametrize("iteration", [0, 1, 6])
def test_iteration_counts(pkg, oracle, iteration):
    """K = 0 (predict + sort + finalise only), 1, and the stock CLI's 6 (benchmark.cpp:24)."""
    sc, side = get_scene(pkg, "dam8192", False)
    s, o = mk(pkg, oracle, sc, False)
    p, q = params_pair(pkg, oracle, iteration=iteration, side=side)
    for _ in range(2):
        s.step(p)
        o.step(q)
    assert_state_equal(s.download(), o.get_particles())

@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("xsph,vort", [(1, 0), (0, 1), (1, 1)])
def test_xsph_vorticity_bit_exact(pkg, oracle, fp64, xsph, vort):
    """Opt-in extras the north star names but the reference lacks (only constants survive,
    sph_constants.h:13-14): checked against OUR restatement only — parity unpinned."""
    sc, side = get_scene(pkg, "dam8192", fp64)
    s, o = mk(pkg, oracle, sc, fp64)
    p, q = params_pair(pkg, oracle, side=side)
    p.xsph, p.vorticity, q.xsph, q.vorticity = xsph, vort, xsph, vort
    for frame in range(4):
        s.step(p)
        o.step(q)
    assert_state_equal(s.download(), o.get_particles())
    # and they do something: velocities differ from the plain solve
    s0, _ = mk(pkg, oracle, sc, fp64)
    p0, _ = params_pair(pkg, oracle, side=side)
    s0.steps(p0, 4)
    assert not np.array_equal(s0.download()["vel"], s.download()["vel"])


# ------------------------------------------------------------------------------------------ B


LATTICE1_TOL = {False: 5e-3, True: 1e-9}
SETTLED1_TOL = {False: 1e-3, True: 1e-9}


@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("scene", SCENES)
def test_one_step_vs_reference_pow(pkg, oracle, scene, fp64):
    """Against the oracle with std::pow exactly as ompsph.hpp:240 writes it."""
    sc, side = get_scene(pkg, scene, fp64)
    s, o = mk(pkg, oracle, sc, fp64, device_pow=False)
    p, q = params_pair(pkg, oracle, side=side)
    s.step(p)
    o.step(q)
    g, w = by_id(s.download()), by_id(o.get_particles())
    assert np.array_equal(g["id"], w["id"])
    d = np.linalg.norm(g["pos"].astype(np.float64) - w["pos"], axis=1)
    assert d.max() <= LATTICE1_TOL[fp64], d.max()
    s.steps(p, 30)  # settle
    st = s.download()
    o.set_particles(**st)
    s.step(p)
    o.step(q)
    g, w = by_id(s.download()), by_id(o.get_particles())
    d = np.linalg.norm(g["pos"].astype(np.float64) - w["pos"], axis=1)
    assert d.max() <= SETTLED1_TOL[fp64], d.max()
    lam_scale = 1.0
    dv = np.abs(g["vel"].astype(np.float64) - w["vel"]).max()
    assert dv <= (1e-3 if not fp64 else 1e-9) * lam_scale, dv


@pytest.mark.parametrize("nm,fp64", [("f32", False), ("f64", True)])
def test_against_committed_golden(pkg, golden_dir, nm, fp64):
    """tests/golden/oracle_selfcheck.npz holds oracle outputs (reference std::pow) committed as data:
    integer stages exact, floating point within B's tolerances; 3 free-running frames: statistics."""
    S = np.load(os.path.join(golden_dir, "oracle_selfcheck.npz"))
    sc, side = get_scene(pkg, "cubes1024", fp64)
    s = pkg.Solver(h=0.1, fp64=fp64)
    s.upload(**sc)
    p = pkg.default_params(4, side)
    s.stage("predict", p).stage("sort", p)
    assert np.array_equal(s.keys().astype(np.uint64), S[f"cubes1024_{nm}_keys"])
    assert np.array_equal(s.download()["id"], S[f"cubes1024_{nm}_sorted_ids"])
    s.stage("diffuse", p).stage("lambda", p)
    assert np.array_equal(s.pstar()[:, 3], S[f"cubes1024_{nm}_lambda1"])  # lambda has no pow in it
    s.stage("delta", p)
    d = np.abs(s.pstar()[:, :3].astype(np.float64) - S[f"cubes1024_{nm}_pstar1"]) * 500
    assert d.max() <= LATTICE1_TOL[fp64], d.max()
    s.upload(**sc)
    for frame in (1, 2, 3):
        s.step(p)
        if frame in (1, 3):
            g = by_id(s.download())
            d = np.linalg.norm(g["pos"].astype(np.float64) - S[f"cubes1024_{nm}_jacobi_f{frame}_pos"], axis=1)
            if frame == 1:
                assert d.max() <= LATTICE1_TOL[fp64], d.max()
            else:
                assert d.mean() <= (1e-2 if not fp64 else 1e-9) and np.percentile(d, 99) <= (0.1 if not fp64 else 1e-8)
            dc = np.abs(g["colour"].astype(np.float64) - S[f"cubes1024_{nm}_jacobi_f{frame}_colour"]).max()
            assert dc <= (1e-5 if not fp64 else 1e-12)

# ------------------------------------------------------------------------------------------ C


def test_fast_math_within_reference_noise_floor(pkg, oracle):
    sc, side = get_scene(pkg, "dam8192", False)
    s, o = mk(pkg, oracle, sc, False, flags=pkg.FLAG_FAST_MATH, device_pow=False)
    p, q = params_pair(pkg, oracle, side=side)
    s.steps(p, 30)
    o.set_particles(**s.download())
    s.step(p)
    o.step(q)
    g, w = by_id(s.download()), by_id(o.get_particles())
    d = np.linalg.norm(g["pos"].astype(np.float64) - w["pos"], axis=1)
    assert d.max() <= 5e-3, d.max()
    assert d.mean() <= 1e-4

# ------------------------------------------------------------------------------ other properties


@pytest.mark.parametrize("fp64", [False, True])
def test_run_to_run_determinism(pkg, fp64):
    sc, side = get_scene(pkg, "dam8192", fp64)
    outs = []
    for _ in range(2):
        s = pkg.Solver(h=0.1, fp64=fp64)
        s.upload(**sc)
        p = pkg.default_params(4, side)
        s.steps(p, 12)
        outs.append(s.download())
    assert_state_equal(outs[0], outs[1])


def test_aos_roundtrip_and_step(pkg):
    """pbf_upload_aos / pbf_download_aos with the reference's Particle<size_t,float> layout (56 B)."""
    from pbf_sph_amd import capi
    sc, side = get_scene(pkg, "cubes1024", False)
    n = len(sc["id"])
    dt = np.dtype([("id", "<u8"), ("type", "u1"), ("_pad", "u1", 3), ("mass", "<f4"), ("pos", "<f4", 3),
                   ("vel", "<f4", 3), ("colour", "<f4", 4)])
    assert dt.itemsize == 56
    a = np.zeros(n, dt)
    for k in FIELDS:
        a[k] = sc[k]
    a["_pad"] = 0xAB
    lay = capi.AosLayout(56, 0, 8, 12, 16, 28, 40)
    s = pkg.Solver(h=0.1)
    L = s.L
    assert L.pbf_upload_aos(s.ctx, n, a.ctypes.data_as(C.c_void_p), C.byref(lay)) == 0
    g = s.download()
    for k in FIELDS:
        assert np.array_equal(g[k], sc[k])
    p = pkg.default_params(4, side)
    s.step(p)
    b = a.copy()
    assert L.pbf_download_aos(s.ctx, b.ctypes.data_as(C.c_void_p), C.byref(lay)) == 0
    g = s.download()
    for k in FIELDS:
        assert np.array_equal(b[k], g[k])
    assert np.all(b["_pad"] == 0xAB)
    s2 = pkg.Solver(h=0.1)
    s2.upload(**sc).step(p)
    assert np.array_equal(s2.download()["pos"], g["pos"])
    # the download in two halves (what the shim's advance() does around pbf_surface): a surface extraction and even a
    # further step enqueued before _end do not change the image that travels
    c = a.copy()
    assert L.pbf_download_aos_begin(s.ctx, c.ctypes.data_as(C.c_void_p), C.byref(lay)) == 0
    assert L.pbf_download_aos_begin(s.ctx, c.ctypes.data_as(C.c_void_p), C.byref(lay)) != 0  # (one at a time)
    s.surface(p)
    s.step(p)
    assert L.pbf_download_aos_end(s.ctx) == 0
    assert L.pbf_download_aos_end(s.ctx) == 0  # (nothing open: a no-op)
    assert c.tobytes() == b.tobytes()


def test_error_paths(pkg):
    s = pkg.Solver(h=0.1)
    p = pkg.default_params(4, 1000.0)
    sc, _ = get_scene(pkg, "cubes1024", False)
    s.upload(**sc)
    with pytest.raises(pkg.PbfError):
        s.stage("lambda", p)  # needs sort first
    with pytest.raises(pkg.PbfError):
        s.stage("sort", p)  # needs predict first
    bad = pkg.default_params(4, 1000.0)
    bad.dt = 0.0
    with pytest.raises(pkg.PbfError):
        s.step(bad)
    huge = pkg.default_params(4, 1000.0)
    huge.max_bound[0] = 1e6  # > 1023 cells per axis: beyond the 10-bit Morton range (curves.h:72-88)
    with pytest.raises(pkg.PbfError):
        s.step(huge)
    s.step(p).sync()  # still usable afterwards


def test_stage_timing(pkg):
    sc, side = get_scene(pkg, "dam8192", False)
    s = pkg.Solver(h=0.1, flags=pkg.FLAG_STAGE_TIMING)
    s.upload(**sc)
    p = pkg.default_params(4, side)
    s.steps(p, 3)
    t = s.stage_times()
    stages = {"advect+zindex", "sortz+gridtable", "sph-diffuse", "sph-lambda", "sph-delta", "sph-finalise"}
    # "stage/part" entries are single kernels inside a stage (the neighbour-list build of the lambda stage)
    assert {k for k in t if "/" not in k} == stages and set(t) - stages == {"sph-lambda/list-build"}
    assert t["sph-lambda"][1] == 12 and t["sph-delta"][1] == 12 and t["advect+zindex"][1] == 3
    # default (split_build 8): the list build and lambda are ONE kernel, the part entry stays empty
    assert t["sph-lambda/list-build"][1] == 0
    assert all(ms > 0 for k, (ms, _) in t.items() if "/" not in k)
    s.set_option("split_build", 5)  # the build as a launch of its own: timed as a part of the lambda stage
    s.reset_stage_times()
    s.steps(p, 3)
    t = s.stage_times()
    assert t["sph-lambda/list-build"][1] == 12 and 0 < t["sph-lambda/list-build"][0] < t["sph-lambda"][0]


@pytest.mark.parametrize("nominal,fp64", [(262144, False), (1048576, False), (1048576, True), (4194304, False)])
def test_full_size_properties(pkg, nominal, fp64):
    """BASELINE.json sizes (configs 2, 3 and 5: 256 K fp32, 1 M fp32, 1 M fp64; and config 4's 4 M column on ONE GPU):
    size-independent properties instead of the oracle."""
    sc, side = pkg.scene_dambreak(nominal, fp64)
    n = len(sc["id"])
    s = pkg.Solver(h=0.1, fp64=fp64)
    s.upload(**sc)
    p = pkg.default_params(4, side)
    s.steps(p, 5)
    s.stage("predict", p).stage("sort", p)
    keys, table = s.keys().astype(np.int64), s.table().astype(np.int64)
    assert np.all(np.diff(keys) >= 0)                                   # sortedness
    tn = len(table)
    inside = keys[keys < tn]
    cnt = np.bincount(inside, minlength=tn)
    assert np.array_equal(table, np.concatenate([[0], np.cumsum(cnt)[:-1]]))  # table = exclusive scan of counts
    g = s.download()
    assert np.array_equal(np.sort(g["id"]), np.arange(n, dtype=np.uint64))    # a permutation: nothing lost
    s.stage("diffuse", p)
    for _ in range(4):
        s.stage("lambda", p).stage("delta", p)
    s.stage("finalise", p)
    g1 = s.download()
    assert np.isfinite(g1["pos"]).all() and np.isfinite(g1["vel"]).all()
    assert g1["pos"].min() >= 0 and g1["pos"].max() <= side                   # clamp (ompsph.hpp:246)
    assert np.all((g1["colour"] >= g1["colour"].dtype.type(0.03)) & (g1["colour"] <= 1.0))  # clamp (ompsph.hpp:204)
    # idempotence of the sort: re-sorting already sorted keys keeps the order (stable)
    s.stage("predict", p).stage("sort", p)
    k2 = s.keys().astype(np.int64)
    assert np.all(np.diff(k2) >= 0)
    ids2 = s.download()["id"]
    same_key_runs = np.flatnonzero(np.diff(k2) == 0)
    assert len(ids2) == n and len(same_key_runs) > 0
    # run-to-run: a second solver reaches the identical state
    s2 = pkg.Solver(h=0.1, fp64=fp64)
    s2.upload(**sc)
    s2.steps(p, 6)
    assert np.array_equal(s2.download()["pos"], g1["pos"])


def test_pile_up_in_one_cell_sorts_in_bounded_time(pkg, oracle):
    """50 000 particles inside ONE grid cell (+ 3 000 outside the grid: the overflow bucket, ordered by (key, source)):
    the sort's in-cell rank would be O(m^2) per cell; cells above BIG_CELL members take the segment sort instead
    (k_sort_big_cells).  K = 0 (predict + sort + diffuse + finalise): the permutation and every field equal the
    oracle's stable sort, bit for bit, and the step stays far below the quadratic cost."""
    import time
    rng = np.random.default_rng(3)
    pile = (rng.random((50000, 3)) * 40 + np.array([505, 505, 505])).astype(np.float32)   # one 50-unit cell
    outside = (rng.random((3000, 3)) * 1000 + np.array([3000, 0, 0])).astype(np.float32)   # x beyond the grid
    far = (rng.random((4000, 3)) * 900 + 50).astype(np.float32)
    pos = np.concatenate([pile, outside, far])
    n = len(pos)
    perm = rng.permutation(n)
    sc = dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n, np.float32), pos=pos[perm],
              vel=np.zeros((n, 3), np.float32), colour=rng.random((n, 4)).astype(np.float32))
    s, o = mk(pkg, oracle, sc, False)
    p, q = params_pair(pkg, oracle, iteration=0)
    p.constant_force[1] = 0.0   # keep the pile in its cell
    q.constant_force[1] = 0.0
    s.stage("predict", p).stage("sort", p).sync()
    o.predict(q).sort(q).grid_table(q)
    keys = s.keys().astype(np.int64)
    assert np.bincount(keys[keys < len(s.table())]).max() >= 50000
    assert_state_equal(s.download(), o.get_particles(), "pile-up sort")
    t0 = time.perf_counter()
    for _ in range(5):
        s.stage("predict", p).stage("sort", p)
    s.sync()
    assert (time.perf_counter() - t0) / 5 < 0.05, "sort of a 50 000-particle cell took too long"


@pytest.mark.parametrize("coop", [2, 4, 8])
@pytest.mark.parametrize("fp64", [False, True])
def test_wave_cooperative_reader_within_tolerance(pkg, oracle, coop, fp64):
    """Option "coop": `coop` lanes share one particle's neighbour list in lambda / delta-p and reduce the kernel sums
    with wave shuffles (north_star: "wavefront-wide __shfl reductions for the per-particle kernel sums").  The
    summation order differs from the reference walk, so the bar is the stated tolerance, not bit-equality: one step
    from a settled state <= 1e-3 world units (fp32; box = 1100), lists / keys / sort unchanged (integer-exact);
    deterministic run to run."""
    sc, side = get_scene(pkg, "dam8192", fp64)
    s, o = mk(pkg, oracle, sc, fp64)
    p, q = params_pair(pkg, oracle, side=side)
    s.steps(p, 30)  # settle with the default (bit-exact) reader
    st = s.download()
    outs = []
    for _ in range(2):
        c = pkg.Solver(h=0.1, fp64=fp64)
        c.set_option("coop", coop)
        c.upload(**st)
        c.step(p)
        outs.append(c.download())
    assert_state_equal(outs[0], outs[1], "coop run-to-run")
    o.set_particles(**st)
    o.step(q)
    g, w = outs[0], o.get_particles()
    assert np.array_equal(g["id"], w["id"])                      # same sort, same permutation
    d = np.linalg.norm(g["pos"].astype(np.float64) - w["pos"], axis=1)
    assert d.max() <= (1e-3 if not fp64 else 1e-9), d.max()
    assert not np.array_equal(g["pos"], w["pos"])  # it really is another summation order, in either precision
    dv = np.abs(g["vel"].astype(np.float64) - w["vel"]).max()
    assert dv <= (1e-3 if not fp64 else 1e-9), dv


def test_ranged_sqrt_and_divide_are_the_ieee_ones(pkg):
    """The precise pair terms use a sqrt (one v_rsq + a Heron step) and divides (Newton from a seed, one residual
    correction) trimmed to their operand range: swept on the device against the compiler's IEEE forms over every fp32
    value (sqrt, x >= 2^-75), every fp32 d2 whose root lies in [1e-8, h] for (h - r)^2 / r — h = the context's 0.1 and
    three more —, every fp32 numerator for the two constant divisors of delta-p.  Not one mismatch allowed, but for the
    sign of one zero quotient that is only ever squared."""
    s = pkg.Solver(h=0.1)
    bad = np.zeros(4, np.uint64)
    s._chk(s.L.pbf_selftest_math(s.ctx, bad.ctypes.data_as(C.c_void_p)), "pbf_selftest_math")
    assert bad[0] == 0 and bad[1] == 0 and bad[2] <= 1 and bad[3] == 0, bad


def test_fp64_trimmed_sqrt_and_divide_agree_with_the_ieee_ones(pkg):
    """fp64 pair terms (round 3): sqrt = the compiler's own v_rsq_f64 + Goldschmidt + two-correction sequence without its
    rescale / class wrappers (identical by construction for x >= 2^-767), divides = Newton from a seed with one
    exact-residual fma correction.  2^64 operands cannot be swept: 1.07e10 pseudo-random operands per category (4.3e10 in
    all; every binade of the stated ranges equally often + the pair terms' own ranges densely) against the compiler's
    IEEE sqrt / divide on the device — not one mismatch allowed."""
    s = pkg.Solver(h=0.1, fp64=True)
    bad = np.zeros(4, np.uint64)
    s._chk(s.L.pbf_selftest_math(s.ctx, bad.ctypes.data_as(C.c_void_p)), "pbf_selftest_math")
    assert not bad.any(), bad


@pytest.mark.parametrize("fp64", [False, True])
def test_steps_fuses_finalise_and_predict_bit_exact(pkg, oracle, fp64):
    """pbf_steps runs finalise(t) + predict(t + 1) as ONE kernel between two steps of a call (option fuse_predict,
    default on; the last step of a call stays unfused, so the state a caller sees is the finalised one): same bits
    as step-by-step calls and as the oracle — obstacles and a gravity well included."""
    sc, side = get_scene(pkg, "dam8192", fp64)
    sc = {k: v.copy() for k, v in sc.items()}
    sc["type"][::17] = 1
    p, q = params_pair(pkg, oracle, side=side, wells=[(0.5 * side, 0.4 * side, 0.5 * side, 900.0)])
    a, o = mk(pkg, oracle, sc, fp64)          # fused: 2 calls of 4 steps
    b = pkg.Solver(h=0.1, fp64=fp64)          # step by step
    b.upload(**sc)
    c = pkg.Solver(h=0.1, fp64=fp64)          # pbf_steps with the fusion off
    c.upload(**sc)
    c.set_option("fuse_predict", 0)
    for chunk in range(2):
        a.steps(p, 4)
        c.steps(p, 4)
        for _ in range(4):
            b.step(p)
            o.step(q)
        ga, gb, gc = a.download(), b.download(), c.download()
        for k in ga:
            assert np.array_equal(ga[k], gb[k]) and np.array_equal(ga[k], gc[k]), (chunk, k)
        assert_state_equal(ga, o.get_particles(), f"chunk {chunk}")


@pytest.mark.parametrize("iteration", [0, 1])
def test_steps_fusion_with_few_iterations(pkg, oracle, iteration):
    """pbf_steps' fused finalise(t) + predict(t + 1) with K = 0 (predict, sort, finalise only) and K = 1: equal to the
    oracle."""
    sc, side = get_scene(pkg, "dam8192", False)
    s, o = mk(pkg, oracle, sc, False)
    p, q = params_pair(pkg, oracle, iteration=iteration, side=side)
    s.steps(p, 3)
    for _ in range(3):
        o.step(q)
    assert_state_equal(s.download(), o.get_particles())


@pytest.mark.parametrize("fp64", [False, True])
def test_graph_replay_bit_exact(pkg, oracle, fp64):
    """pbf_steps can replay each distinct step as a captured hipGraph (option graph; off by default: measured slower than
    eager launches): the buffer roles rotate
    with a short period, so after a few captures every step is a replay.  Same launches, same arguments => the same
    bits as the eager loop and as the oracle; a moving box (parameters change every frame) falls back to eager."""
    sc, side = get_scene(pkg, "dam8192", fp64)
    p, q = params_pair(pkg, oracle, side=side)
    a = pkg.Solver(h=0.1, fp64=fp64)
    a.set_option("graph", 1)
    a.upload(**sc)
    for _ in range(4):
        a.steps(p, 4)          # 16 frames, several calls
    captured, replayed, on = a.graph_stats()
    assert on and 1 <= captured <= 12 and replayed >= 16 - 1 - captured, (captured, replayed, on)
    b = pkg.Solver(h=0.1, fp64=fp64)
    b.set_option("graph", 0)
    b.upload(**sc)
    b.steps(p, 16)
    assert b.graph_stats()[:2] == (0, 0)
    assert_state_equal(a.download(), b.download(), "graph vs eager")
    if not fp64:
        o = oracle.Oracle(fp64, device_pow=True)
        o.set_particles(**sc)
        for _ in range(16):
            o.step(q)
        assert_state_equal(a.download(), o.get_particles(), "graph vs oracle")
    # a box that moves every frame never repeats a step: graphs switch themselves off, results stay right
    c = pkg.Solver(h=0.1, fp64=fp64)
    c.set_option("graph", 1)
    c.upload(**sc)
    d = pkg.Solver(h=0.1, fp64=fp64)
    d.set_option("graph", 0)
    d.upload(**sc)
    for frame in range(14):
        pm = pkg.apply_motion(p, frame, fp64)
        c.steps(pm, 1)
        d.steps(pm, 1)
    assert c.graph_stats()[2] is False
    assert_state_equal(c.download(), d.download(), "moving box")
