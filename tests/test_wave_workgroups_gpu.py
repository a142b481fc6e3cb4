"""The row iteration kernels at workgroup widths of 64, 128 and 256 lanes (options "build_wg" / "reader_wg", "iter_wg" for both;
csrc/pbf_kernels.hpp iter_unit).  A workgroup is a unit of a 256-lane chunk; what a lane computes, and where its list lies, does
not depend on the width.  Held here with no tolerance: every width gives the oracle's bits stage by stage over two solver
iterations (lambda, pStar after delta-p, the final state), and the bytes of the 256-wide run (those and the list lengths — but for
WHICH of the lists beyond the rows walk when the pool of chunks runs dry, which is the lanes' order of arrival at any width:
assert_counts_agree), on

  * the staircase scene (n = 1 mod 64: a last unit of one lane; with obstacles, units whose lanes all leave at op.begin beside
    sibling units that run on), under its own condition asserts;
  * the two-tier scene: lists beyond the rows' 40 slots (pool chunks, put_any) and NBR_OVERFLOW walkers, alone in a one-wave
    workgroup;
  * 1, 63, 64, 65, 255 and 257 particles in one row of cells;
  * the edge scene with walkers in no cell (ROW_FALLBACK: the serial walk inside a one-wave workgroup);

in fp32 and fp64, with and without obstacles.  Lists written at one width are read at another, both ways, in one context."""
import numpy as np
import pytest

from test_hip_parity import assert_state_equal, params_pair, two_tier_scene
from test_row_gathers_gpu import OVERFLOW, edge_scene, scene_of
from test_tail_trips_gpu import assert_every_width_runs, sched_probe, staircase_scene

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128, 256)
FP = pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
OBST = pytest.mark.parametrize("obstacles", [False, True], ids=["free", "obstacles"])

_ORACLE = {}


def oracle_stages(oracle, key, sc, fp64, q):
    """the oracle's keys, lambda and pStar of two solver iterations and its final state: computed once per scene, never changed"""
    if key not in _ORACLE:
        o = oracle.Oracle(fp64, device_pow=True)
        o.set_particles(**sc)
        o.predict(q)
        o.sort(q).grid_table(q)
        o.diffuse(q)
        want = {"keys": np.array(o.keys(), copy=True)}
        for it in range(2):
            o.lambda_(q)
            want["lambda", it] = np.array(o.lambdas(), copy=True)
            o.delta(q)
            want["pstar", it] = np.array(o.pstar(), copy=True)
        o.finalise(q)
        want["final"] = {k: np.array(v, copy=True) for k, v in o.get_particles().items()}
        _ORACLE[key] = want
    return _ORACLE[key]


def run_stages(pkg, sc, fp64, p, want, widths, check=None):
    """One context through predict, sort, diffuse, two solver iterations and finalise, every stage against the oracle.
    widths(it) -> (build_wg, reader_wg) of iteration `it`.  Returns what the run left, for the byte comparison."""
    s = pkg.Solver(h=0.1, fp64=fp64)
    s.upload(**sc)
    for stage in ("predict", "sort", "diffuse"):
        s.stage(stage, p)
    assert np.array_equal(s.keys().astype(np.uint64), want["keys"])
    got = {}
    for it in range(2):
        build, reader = widths(it)
        if build == reader:
            s.set_option("iter_wg", build)  # (sets both sites)
        else:
            s.set_option("build_wg", build).set_option("reader_wg", reader)
        s.stage("lambda", p)
        got["lambda", it], got["counts", it] = s.pstar()[:, 3].copy(), s.nbr_counts()
        if it == 0 and check is not None:
            check(s)
        assert np.array_equal(got["lambda", it], want["lambda", it]), ("lambda", it, build, reader)
        s.stage("delta", p)
        got["pstar", it] = s.pstar()[:, :3].copy()
        assert np.array_equal(got["pstar", it], want["pstar", it]), ("delta", it, build, reader)
    s.stage("finalise", p)
    final = s.download()
    assert_state_equal(final, want["final"], f"finalise {widths(0)} {widths(1)}")
    got.update(final)
    return got


def every_width(pkg, oracle, key, sc, fp64, side=1000.0, check=None):
    p, q = params_pair(pkg, oracle, side=side)
    want = oracle_stages(oracle, key + (fp64,), sc, fp64, q)
    got = {}
    for wg in WIDTHS:
        got[wg] = run_stages(pkg, sc, fp64, p, want, lambda it, wg=wg: (wg, wg), check)
    for wg in WIDTHS[:-1]:
        for k, v in got[256].items():
            if k[0] == "counts":
                assert_counts_agree(got[wg][k], v, (wg, k))
            else:
                assert got[wg][k].tobytes() == v.tobytes(), (wg, k)
    return got[256]


def assert_counts_agree(a, b, what):
    """The list lengths of two builds of one pStar.  Byte for byte — except where the pool decides: a list beyond the rows' 40
    slots takes its chunk by an atomic ticket, and when the pool runs dry (the two-tier scene asks for three times its chunks)
    WHICH of those lists walk instead (NBR_OVERFLOW) is the order the lanes arrived in, different from launch to launch at one
    width too.  So: equal wherever neither build marked the list overflowed, and a list only one of them marked is one that
    needed a chunk in the other (longer than 40)."""
    a, b = a.astype(np.int64), b.astype(np.int64)
    oa, ob = a == OVERFLOW, b == OVERFLOW
    both = ~oa & ~ob
    assert np.array_equal(a[both], b[both]), what
    assert np.all(b[oa & ~ob] > 40) and np.all(a[ob & ~oa] > 40), what
    if not (oa ^ ob).any():
        assert a.tobytes() == b.tobytes(), what


def as_type(sc, fp64):
    dt = np.float64 if fp64 else np.float32
    return {k: (v.astype(dt) if v.dtype.kind == "f" else v.copy()) for k, v in sc.items()}


@FP
@OBST
def test_staircase_every_width(pkg, oracle, fp64, obstacles):
    every_width(pkg, oracle, ("staircase", obstacles), staircase_scene(fp64, obstacles), fp64, check=assert_every_width_runs)


def two_tier(pkg, fp64, obstacles):
    sc, side = two_tier_scene(pkg)
    sc = as_type(sc, fp64)
    if obstacles:
        sc["type"][6::13] = 1
    return sc, side


def assert_both_tiers(s):
    """Condition, not a skip: lists within the rows, lists in a pool chunk and lists that overflowed (walkers) all occur.
    (The scene's own test asks for 200 / 100 / 1000 without obstacles; one particle in thirteen is an obstacle here.)"""
    cnt = s.nbr_counts().astype(np.int64)
    spill, over, rows = ((cnt > 40) & (cnt <= 160)).sum(), (cnt == OVERFLOW).sum(), ((cnt > 0) & (cnt <= 40)).sum()
    print("two tiers: rows", rows, "chunk", spill, "overflow", over)
    assert spill >= 150 and over >= 80 and rows >= 900, (spill, over, rows)


@FP
@OBST
def test_two_tier_lists_every_width(pkg, oracle, fp64, obstacles):
    sc, side = two_tier(pkg, fp64, obstacles)
    every_width(pkg, oracle, ("twotier", obstacles), sc, fp64, side=side, check=assert_both_tiers)


@FP
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257])
def test_particle_counts_in_one_cell_row(pkg, oracle, fp64, n):
    """n particles in the 18 cells of one x-row (cell = 50 units): a last unit of 1, 63, 64 lanes, a chunk of one unit, one lane
    past a chunk; obstacles from 63 on"""
    rng = np.random.default_rng(100 + n)
    pos = np.array([55.0, 255.0, 255.0]) + rng.random((n, 3)) * np.array([890.0, 40.0, 40.0])
    every_width(pkg, oracle, ("row", n), scene_of(pos, fp64, n, obstacles=n >= 63), fp64)


@FP
@OBST
def test_walkers_in_no_cell_every_width(pkg, oracle, fp64, obstacles):
    """the edge scene: seven particles outside the table (ROW_FALLBACK), a pile beyond 160 slots, lists of 0, 1, 39, 40, 41"""
    def check(s):
        keys, table = s.keys().astype(np.int64), s.table()
        assert (keys >= len(table) - 1).sum() >= 5, "no walker outside the table"
        assert OVERFLOW in set(s.nbr_counts().tolist())

    every_width(pkg, oracle, ("edge", obstacles), edge_scene(fp64, obstacles), fp64, check=check)


@FP
@pytest.mark.parametrize("first", [(64, 256), (256, 64), (128, 64)], ids=lambda w: f"build{w[0]}-read{w[1]}")
def test_lists_written_at_one_width_are_read_at_another(pkg, oracle, fp64, first):
    """one context; iteration 0 builds at first[0] and reads at first[1], iteration 1 the other way round"""
    sc, side = two_tier(pkg, fp64, True)
    p, q = params_pair(pkg, oracle, side=side)
    want = oracle_stages(oracle, ("twotier", True, fp64), sc, fp64, q)
    run_stages(pkg, sc, fp64, p, want, lambda it: first if it == 0 else first[::-1], assert_both_tiers)


def test_row_diffusion_runs_of_every_remainder(pkg, oracle):
    """k_diffuse_rows' read-ahead fold takes four records per trip and 0 .. 3 after its last one (a two-buffer form of it, eight
    per turn, was measured for this change and not kept): in the staircase scene (cells of 1 .. 10 particles, three-cell runs of
    9 .. 24 and one of 40) a lane's sub-run takes every length modulo 8.  One step stage by stage, without obstacles (the
    untyped fold) and with: the state, colours included, is the oracle's."""
    for obstacles in (False, True):
        sc = staircase_scene(False, obstacles)
        p, q = params_pair(pkg, oracle)
        s = pkg.Solver(h=0.1)
        s.upload(**sc)
        o = oracle.Oracle(False, device_pow=True)
        o.set_particles(**sc)
        for stage in ("predict", "sort", "diffuse"):
            s.stage(stage, p)
        o.predict(q)
        o.sort(q).grid_table(q)
        o.diffuse(q)
        keys = s.keys().astype(np.int64)
        _, runs = sched_probe.row_run_lengths(keys)
        assert {int(v) % 8 for v in runs[runs > 0]} == set(range(8)), "sub-run lengths modulo 8"
        for stage in ("lambda", "delta", "finalise"):
            s.stage(stage, p)
        o.lambda_(q)
        o.delta(q)
        o.finalise(q)
        assert_state_equal(s.download(), o.get_particles(), f"obstacles={obstacles}")


def test_widths_other_than_64_128_256_are_refused(pkg):
    s = pkg.Solver(h=0.1)
    for name in ("iter_wg", "build_wg", "reader_wg"):
        for bad in (0, 32, 96, 192, 512, -64):
            with pytest.raises(pkg.PbfError):
                s.set_option(name, bad)
        for good in WIDTHS:
            s.set_option(name, good)
