"""The iteration kernels on the row-major copy take their candidates from a 32-bit byte offset off the array's base
(load_at, csrc/pbf_kernels.hpp), and the list build's drain reads the staged slots of a trip in one straight block, taken or
not.  The rule both stand on: an entry from a slot at or beyond a list's length — stale or uninitialised memory — is
selected away before it becomes an address.  Held here, bit for bit and with no tolerance, against the oracle and against
the plain per-particle walk (gather = 0):

  1. stale entries are never used: a dense scene, then a sparse one on the SAME context (the rows then hold the dense
     scene's entries beyond every list's end), and the other way round;
  2. list lengths at the trip edges: 0, 1, 39, 40, 41 (the first chunk entry) and NBR_OVERFLOW in one scene, and the
     staircase scene's remainders of 8;
  3. n = 1, 63, 65, 257; walkers in no cell (ROW_FALLBACK); obstacles leaving a live wave;
  4. all of it in fp64 (the offset is slot << 5 there), and a static collider (DeltaOp<.., COLLIDE_STATIC> shares load_at);
  5. two solver iterations stage by stage: a wrong candidate shows in the stage that read it.
"""
import numpy as np
import pytest

from test_collider_gpu import BOX_LATTICE, plane_through, set_lattice
from test_hip_parity import assert_state_equal, mk, oracle_run, params_pair
from test_tail_trips_gpu import assert_every_width_runs, staircase_scene

pytestmark = pytest.mark.gpu

OVERFLOW = 0xFFFFFFFF
REACH = 50.0          # h * scale with h = 0.1, scale = 500: the radius of a neighbourhood in world units
FP = pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])


def scene_of(pos, fp64, seed, obstacles=False):
    rng = np.random.default_rng(seed)
    n = len(pos)
    dt = np.float64 if fp64 else np.float32
    ty = np.zeros(n, np.uint8)
    if obstacles:
        ty[::13] = 1                                          # lanes that leave at op.begin while their wave goes on
    return dict(id=np.arange(n, dtype=np.uint64), type=ty, mass=np.ones(n, dt), pos=np.asarray(pos).astype(dt),
                vel=np.zeros((n, 3), dt), colour=rng.uniform(0.03, 1.0, (n, 4)).astype(dt))


def within_reach(pos):
    """per particle: how many particles (itself included, as the lists include it) lie within REACH — float64, all pairs"""
    p = np.asarray(pos, np.float64)
    out = np.empty(len(p), np.int64)
    for a in range(0, len(p), 512):
        d = p[a:a + 512, None, :] - p[None, :, :]
        out[a:a + 512] = ((d * d).sum(-1) <= REACH * REACH).sum(1)
    return out


def blob(rng, n=1100):
    """a 340 x 200 x 200 block whose density rises along x from 0.3 to 1.7 times the one that puts 40 particles into a
    neighbourhood (7.6e-5 per unit volume): lists of every length from a few to about 70"""
    x = 340.0 * (np.sqrt(rng.random(n) * (1.7 ** 2 - 0.3 ** 2) + 0.3 ** 2) - 0.3) / 1.4   # (density linear in x)
    return np.stack([300.0 + x, 400.0 + 200.0 * rng.random(n), 400.0 + 200.0 * rng.random(n)], 1)


_EDGE = {}


def edge_positions():
    """The blob, loners (a list of one: the particle itself), pairs, a pile beyond the 160 slots of a list, a clump outside
    the grid (walkers in no cell: ROW_FALLBACK) — n = 1 (mod 64), uploaded unsorted.  Checked when written, on the CPU:
    the true neighbourhoods bracket every length the test asks the lists for (a list holds a superset of its particle's
    neighbourhood; the exact lengths are asserted from nbr_counts() where the scene is used)."""
    if "pos" not in _EDGE:
        rng = np.random.default_rng(1907)
        parts = [blob(rng)]
        parts.append(np.array([[60.0 + 120.0 * k, 80.0, 90.0] for k in range(6)]))                      # loners
        parts.append(np.array([[70.0 + 130.0 * (k // 2) + 20.0 * (k % 2), 900.0, 80.0] for k in range(8)]))  # pairs
        parts.append(np.array([800.0, 800.0, 800.0]) + 12.0 * rng.random((200, 3)))                      # a pile: > 160
        parts.append(np.array([5000.0, 500.0, 500.0]) + 30.0 * rng.random((5, 3)))                       # in no cell
        parts.append(np.array([[500.0, -4000.0, 500.0], [900.0, 900.0, 30000.0]]))
        pos = np.concatenate(parts)
        pad = (1 - len(pos)) % 64
        pos = np.concatenate([pos, np.array([[100.0 + 90.0 * (k % 9), 100.0 + 90.0 * (k // 9), 900.0] for k in range(pad)]).reshape(pad, 3)])  # loners
        near = within_reach(pos)
        assert len(pos) % 64 == 1 and len(pos) <= 4096, len(pos)
        assert (near == 1).sum() >= 6 and (near == 2).sum() >= 8 and (near > 160).sum() >= 200, np.bincount(near)[:4]
        for k in range(30, 48):                              # the lengths around the rows' 40 slots are all populated
            assert (near == k).sum() >= 5, (k, (near == k).sum())
        _EDGE["pos"] = pos[rng.permutation(len(pos))]
    return _EDGE["pos"]


def edge_scene(fp64, obstacles=False):
    return scene_of(edge_positions(), fp64, 7, obstacles)


def sparse_scene(fp64, n):
    """n particles scattered over the box: 1.5 neighbours on average, lists of 1 to about 6, and obstacles (lists of 0)"""
    rng = np.random.default_rng(311)
    return scene_of(20.0 + 960.0 * rng.random((n, 3)), fp64, 8, obstacles=True)


def counts_after_first_build(pkg, sc, fp64, p, chunks=0):
    s = pkg.Solver(h=0.1, fp64=fp64)
    if chunks:
        s.set_option("nbr_chunks", chunks)
    s.upload(**sc).stage("predict", p).stage("sort", p).stage("lambda", p)
    return s.nbr_counts().astype(np.int64)


def stage_by_stage(pkg, oracle, sc, fp64, check=None):
    """predict, sort, diffuse, then two solver iterations: lambda's bits, then delta-p's, against the oracle and against the
    plain walk, then finalise"""
    s, o = mk(pkg, oracle, sc, fp64)
    g, _ = mk(pkg, oracle, sc, fp64, gather=0)
    p, q = params_pair(pkg, oracle)
    for stage in ("predict", "sort", "diffuse"):
        s.stage(stage, p), g.stage(stage, p)
    o.predict(q)
    o.sort(q).grid_table(q)
    o.diffuse(q)
    assert np.array_equal(s.keys().astype(np.uint64), o.keys())
    for it in range(2):
        s.stage("lambda", p), g.stage("lambda", p)
        o.lambda_(q)
        if it == 0 and check is not None:
            check(s)
        assert np.array_equal(s.pstar()[:, 3], o.lambdas()), ("lambda", it)
        assert np.array_equal(s.pstar()[:, 3], g.pstar()[:, 3]), ("lambda", it)
        s.stage("delta", p), g.stage("delta", p)
        o.delta(q)
        assert np.array_equal(s.pstar()[:, :3], o.pstar()), ("delta", it)
        assert np.array_equal(s.pstar()[:, :3], g.pstar()[:, :3]), ("delta", it)
    s.stage("finalise", p)
    o.finalise(q)
    assert_state_equal(s.download(), o.get_particles(), "finalise")


# ---- 1. stale entries -------------------------------------------------------------------------------------------------------
@FP
@pytest.mark.parametrize("order", ["dense-sparse", "sparse-dense"])
def test_stale_entries_beyond_a_lists_end_are_never_used(pkg, oracle, fp64, order):
    dense = edge_scene(fp64)
    sparse = sparse_scene(fp64, len(dense["id"]) - 64)
    p, q = params_pair(pkg, oracle)
    cd, cs = counts_after_first_build(pkg, dense, fp64, p), counts_after_first_build(pkg, sparse, fp64, p)
    live = cd[cd != OVERFLOW]
    assert (live >= 38).sum() >= 200 and ((live > 40) & (live <= 160)).sum() >= 50, np.bincount(live)[36:44]
    assert cs.max() <= 10 and (cs == 0).sum() >= 50 and (cs == 1).sum() >= 100, np.bincount(cs)
    first, second = (dense, sparse) if order == "dense-sparse" else (sparse, dense)
    s = pkg.Solver(h=0.1, fp64=fp64)
    s.upload(**first).step(p)
    s.upload(**second).step(p)                               # the rows still hold the first scene's lists
    fresh = pkg.Solver(h=0.1, fp64=fp64)
    fresh.upload(**second).step(p)
    want = oracle_run(oracle, ("row-gathers", order.split("-")[1], fp64), second, fp64, q, (0,))[0]
    got = s.download()
    assert_state_equal(got, want, "against the oracle")
    assert_state_equal(got, fresh.download(), "against a fresh context")


# ---- 2. and 5. list lengths at the trip edges, stage by stage ---------------------------------------------------------------
@FP
def test_list_lengths_at_the_trip_edges_stage_by_stage(pkg, oracle, fp64):
    sc = edge_scene(fp64, obstacles=True)

    def check(s):
        cnt = s.nbr_counts().astype(np.int64)
        have = set(cnt.tolist())
        assert {0, 1, 39, 40, 41} <= have and OVERFLOW in have, sorted(have)[:60]
        print("lists:", np.bincount(cnt[cnt != OVERFLOW], minlength=48)[:48], "overflowed:", (cnt == OVERFLOW).sum())

    stage_by_stage(pkg, oracle, sc, fp64, check)


@FP
def test_one_chunk_in_the_pool_sends_the_others_walking(pkg, oracle, fp64):
    """nbr_chunks = 1: one list gets the chunk, every other list beyond the rows overflows and walks its runs."""
    sc = edge_scene(fp64)
    p, q = params_pair(pkg, oracle)
    cnt = counts_after_first_build(pkg, sc, fp64, p, chunks=1)
    assert ((cnt > 40) & (cnt <= 160)).sum() <= 1 and (cnt == OVERFLOW).sum() >= 250, np.bincount(cnt[cnt != OVERFLOW])
    s = pkg.Solver(h=0.1, fp64=fp64)
    s.set_option("nbr_chunks", 1)
    s.upload(**sc).step(p)
    want = oracle_run(oracle, ("row-gathers", "dense", fp64), sc, fp64, q, (0,))[0]
    assert_state_equal(s.download(), want, "one chunk")


@FP
@pytest.mark.parametrize("obstacles", [False, True])
def test_staircase_remainders_stage_by_stage(pkg, oracle, fp64, obstacles):
    stage_by_stage(pkg, oracle, staircase_scene(fp64, obstacles), fp64, assert_every_width_runs)


# ---- 3. odd n -----------------------------------------------------------------------------------------------------------------
@FP
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_n_that_is_no_multiple_of_a_wave_or_a_block(pkg, oracle, fp64, n):
    """the n particles of the blob nearest its dense end (lists that reach into a chunk from 63 on), one of them moved
    outside the grid from 63 on, obstacles from 65 on"""
    pos = blob(np.random.default_rng(77))
    pos = pos[np.argsort(np.abs(pos - np.array([640.0, 500.0, 500.0])).max(1))[:n]].copy()
    if n >= 63:
        pos[5] = [5000.0, 500.0, 500.0]
    stage_by_stage(pkg, oracle, scene_of(pos, fp64, n, obstacles=n >= 65), fp64)


# ---- 4. a static collider -----------------------------------------------------------------------------------------------------
@FP
def test_static_collider_reads_the_same_candidates(pkg, fp64):
    sc = edge_scene(fp64, obstacles=True)
    dt = np.float64 if fp64 else np.float32
    lat, phi64, _ = plane_through(sc, dt)
    p = pkg.default_params(4, 1000.0)
    got = {}
    for path in ("rows", "plain"):
        s = pkg.Solver(h=0.1, fp64=fp64)
        if path == "plain":
            s.set_option("row_major", 0).set_option("gather", 0)
        s.upload(**sc)
        set_lattice(s, lat, phi64, BOX_LATTICE["spacing"])
        for _ in range(2):
            s.step(p)
        got[path] = s.download()
        got[path]["pstar"] = s.pstar()
    off = pkg.Solver(h=0.1, fp64=fp64)
    off.upload(**sc)
    for _ in range(2):
        off.step(p)
    assert not np.array_equal(off.download()["pos"], got["rows"]["pos"])   # the collider does act on this scene
    for k in got["rows"]:
        assert got["rows"][k].tobytes() == got["plain"][k].tobytes(), k
