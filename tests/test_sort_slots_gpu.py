"""The sort stage places every particle by the slot its histogram atomic handed out (cellSlot: written by k_predict,
k_finalise_predict and the slab assembly, read by k_scatter_slots, which also stores the occupied buckets back to zero).
Which member of a cell gets which slot is arbitrary; k_rank_move ranks cell-mates by source index, so the result is
std::stable_sort's — the oracle's (JACOBI, SORT_STABLE), bit for bit:

  * several steps in a row, through steps() (finalise + predict fused), step() and the staged API: a histogram that did
    not return to zero, or a slot that belongs to another histogram, shows in steps 2 and 3;
  * one cell of exactly BIG_CELL, BIG_CELL + 1 and BIG_CELL + 2 members: the pile-up is announced by the member whose
    slot equals BIG_CELL;
  * the overflow bucket (particles outside the grid, several keys): ordered by (key, source index);
  * 66 such cells, and 66 with the overflow bucket as the 67th: k_sort_big_cells has 64 workgroups and strides over the list;
  * each with option row_major 1 (two tables, the row table's populations gathered from the histogram) and 0.

The scenes run with K = 0 solver iterations: 20 000 particles at random in 10^3 cells are far from a fluid at rest, and
nothing of this stage depends on what the iterations do (tests/test_hip_parity.py holds those to the oracle)."""
import numpy as np
import pytest

import trip_scenes as T
from slab_engines import spread10

pytestmark = pytest.mark.gpu

BIG_CELL = 2048      # csrc/pbf_kernels.hpp
PBF_ERR_STATE = -4   # include/pbf_hip.h
CELL = 50.0          # world units per cell: h * scale
SIDE = 300.0         # max_bound: 6 cells of box + 2 cells of padding on either side = 10 cells per axis


def scene(pos, vel=None, seed=1):
    n = len(pos)
    rng = np.random.default_rng(seed)
    return dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n, np.float32),
                pos=np.asarray(pos, np.float32), vel=np.zeros((n, 3), np.float32) if vel is None else vel,
                colour=rng.uniform(0.0, 1.0, (n, 4)).astype(np.float32))


def cell_of(pos):
    """cell coordinates of world positions at rest ((pos / scale - minExtent) / h with minExtent = -2 h)"""
    return np.floor(np.asarray(pos, np.float64) / CELL + 2.0).astype(np.int64)


def random_box(n=20000, seed=7):
    """n particles over all 10^3 cells of the grid; |v| so that about a third leave their cell per step: a step moves a
    particle by v dt scale = 6.2 v world units, v uniform in +-2 => |d| / 50 = 0.124 per axis, 1 - 0.876^3 = 0.33"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-2 * CELL, SIDE + 2 * CELL, (n, 3))
    vel = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    return scene(pos, vel, seed)


def params(pkg, oracle, iteration=0):
    p = pkg.default_params(iteration, SIDE)
    q = oracle.make_params(iteration=iteration, max_bound=(SIDE,) * 3, mode=oracle.JACOBI, sort=oracle.SORT_STABLE)
    return p, q


def solver(pkg, sc, row_major):
    s = pkg.Solver(h=0.1)
    s.set_option("row_major", row_major)
    s.upload(**sc)
    return s


def assert_state_equal(g, w, what):
    for k in ("id", "type", "mass", "pos", "vel", "colour"):
        assert np.array_equal(g[k], w[k]), (what, k)


_RUN = {}


def oracle_steps(pkg, oracle):
    """the oracle's state after steps 1, 2, 3 of the random box (computed once) and the fraction that changed cell"""
    if not _RUN:
        sc = random_box()
        _, q = params(pkg, oracle)
        o = oracle.Oracle(False, device_pow=True)
        o.set_particles(**sc)
        states, moved = [], []
        for _ in range(3):
            before = {int(i): tuple(c) for i, c in zip(sc["id"], cell_of(sc["pos"]))} if not states else \
                {int(i): tuple(c) for i, c in zip(states[-1]["id"], cell_of(states[-1]["pos"]))}
            o.step(q)
            st = {k: np.array(v, copy=True) for k, v in o.get_particles().items()}
            moved.append(np.mean([before[int(i)] != tuple(c) for i, c in zip(st["id"], cell_of(st["pos"]))]))
            states.append(st)
        _RUN["sc"], _RUN["states"], _RUN["moved"] = sc, states, moved
    return _RUN["sc"], _RUN["states"], _RUN["moved"]


@pytest.mark.parametrize("row_major", [1, 0])
def test_multi_step_order(pkg, oracle, row_major):
    sc, want, moved = oracle_steps(pkg, oracle)
    assert all(0.2 < m < 0.5 for m in moved), moved  # the scene does what it is for: about a third change cell per step
    p, _ = params(pkg, oracle)
    s = solver(pkg, sc, row_major)
    for k in range(3):  # three single steps: k_predict is the histogram's producer
        s.step(p)
        assert_state_equal(s.download(), want[k], f"step() {k + 1}")
    for count in (1, 2, 3):  # one steps() call: from its second step on, k_finalise_predict is
        s = solver(pkg, sc, row_major)
        s.steps(p, count)
        assert_state_equal(s.download(), want[count - 1], f"steps(p, {count})")
    # and the two mixed: a fused predict behind a plain one, and the other way round
    s = solver(pkg, sc, row_major)
    s.step(p)
    s.steps(p, 2)
    assert_state_equal(s.download(), want[2], "step() + steps(p, 2)")


@pytest.mark.parametrize("row_major", [1, 0])
def test_staged_api(pkg, oracle, row_major):
    sc = random_box()
    p, q = params(pkg, oracle)
    s = solver(pkg, sc, row_major)
    o = oracle.Oracle(False, device_pow=True)
    o.set_particles(**sc)
    for rnd in range(3):
        s.stage("predict", p)
        o.predict(q)
        assert np.array_equal(s.keys().astype(np.uint64), o.keys()), rnd
        if rnd == 1:  # a predict whose histogram never reaches a sort must not leak into the next one's (predict moves
            s.stage("predict", p)  # the velocities on: the oracle predicts twice too)
            o.predict(q)
            assert np.array_equal(s.keys().astype(np.uint64), o.keys()), rnd
        s.stage("sort", p)
        o.sort(q).grid_table(q)
        assert np.array_equal(s.keys().astype(np.uint64), o.keys()), rnd
        assert np.array_equal(s.table().astype(np.uint64), o.table()), rnd
        assert_state_equal(s.download(), o.get_particles(), f"sort {rnd}")
        rc = s.L.pbf_stage_sort(s.ctx, p)  # the scatter consumed the histogram and its slots: never twice
        assert rc == PBF_ERR_STATE, rc
        s.stage("finalise", p)
        o.finalise(q)
    assert_state_equal(s.download(), o.get_particles(), "finalise")


def pile_scene(members, seed):
    """`members` particles in ONE cell, mixed at random among 500 others spread over the box"""
    rng = np.random.default_rng(seed)
    pile = np.array([3, 4, 5]) * CELL - 2 * CELL + rng.uniform(5.0, 45.0, (members, 3))
    rest = rng.uniform(0.0, SIDE, (700, 3))
    rest = rest[~np.all(cell_of(rest) == (3, 4, 5), axis=1)][:500]  # (none of them in the pile's cell)
    pos = np.concatenate([pile, rest])[rng.permutation(members + 500)]
    return scene(pos, None, seed)


@pytest.mark.parametrize("row_major", [1, 0])
@pytest.mark.parametrize("members", [BIG_CELL, BIG_CELL + 1, BIG_CELL + 2])
def test_big_cell_edge(pkg, oracle, members, row_major):
    sc = pile_scene(members, members)
    cells = cell_of(sc["pos"])
    assert len(cells) == members + 500 and np.sum(np.all(cells == (3, 4, 5), axis=1)) == members
    p, q = params(pkg, oracle)
    p.constant_force[:] = (0.0, 0.0, 0.0)  # at rest: the pile stays the pile in the second round
    q.constant_force[:] = (0.0, 0.0, 0.0)
    s = solver(pkg, sc, row_major)
    o = oracle.Oracle(False, device_pow=True)
    o.set_particles(**sc)
    for rnd in range(2):  # (the second round sorts the sorted set: its histogram starts from what the first one left)
        s.stage("predict", p)
        s.stage("sort", p)
        o.predict(q)
        o.sort(q).grid_table(q)
        assert np.array_equal(s.keys().astype(np.uint64), o.keys()), rnd
        assert np.array_equal(s.table().astype(np.uint64), o.table()), rnd
        assert np.array_equal(s.download()["id"], o.get_particles()["id"]), rnd
        if rnd == 0:  # stable: cell-mates keep their source order (ids are source indices)
            k, src = o.keys(), s.download()["id"].astype(np.int64)
            same = k[1:] == k[:-1]
            assert np.all(src[1:][same] > src[:-1][same])


@pytest.mark.parametrize("row_major", [1, 0])
def test_overflow_bucket(pkg, oracle, row_major):
    rng = np.random.default_rng(11)
    inside = rng.uniform(0.0, SIDE, (2000, 3))
    # outside the table: cells 16 .. 23 along x put a key above tableN = morton(10, 10, 10) = 3640 whatever y and z are
    outside = np.stack([rng.uniform(14 * CELL, 22 * CELL, 300), rng.uniform(0.0, SIDE, 300),
                        rng.uniform(0.0, SIDE, 300)], axis=1)
    pos = np.concatenate([inside, outside])[rng.permutation(2300)]
    sc = scene(pos, None, 11)
    p, q = params(pkg, oracle)
    s = solver(pkg, sc, row_major)
    o = oracle.Oracle(False, device_pow=True)
    o.set_particles(**sc)
    s.stage("predict", p)
    before = s.keys().astype(np.int64)  # by source index
    s.stage("sort", p)
    o.predict(q)
    o.sort(q).grid_table(q)
    assert np.array_equal(s.table().astype(np.uint64), o.table())
    table_n = 7 * (spread10(10))  # morton(10, 10, 10)
    assert table_n == 3640
    out = before >= table_n
    assert int(out.sum()) == 300 and len(np.unique(before[out])) >= 5, int(out.sum())
    got = s.download()["id"].astype(np.int64)
    assert np.array_equal(got, o.get_particles()["id"].astype(np.int64))
    assert np.array_equal(got, np.lexsort((np.arange(2300), before)))  # (key, source index); ids are source indices
    assert np.array_equal(s.keys().astype(np.int64), before[got])
    s.stage("finalise", p)
    s.step(p)  # and a whole step behind it, from the histogram the pile-up's scatter left
    o.finalise(q)
    o.step(q)
    assert_state_equal(s.download(), o.get_particles(), "step after the overflow sort")


_PILES = {}


def piles_reference(pkg, oracle, overflow):
    """the oracle's keys, table and ids after each of two rounds of predict + sort, and its state after a whole step behind
    them (computed once per scene)"""
    if overflow not in _PILES:
        sc = T.piles_scene(overflow)
        q = oracle.make_params(iteration=0, force=(0.0, 0.0, 0.0), max_bound=(T.PILE_SIDE,) * 3, mode=oracle.JACOBI,
                               sort=oracle.SORT_STABLE)
        o = oracle.Oracle(False, device_pow=True)
        o.set_particles(**sc)
        rounds = []
        for _ in range(2):
            o.predict(q)
            T.check_pile_trips(o.keys(), overflow)  # more listed cells than k_sort_big_cells has workgroups, in both rounds
            o.sort(q).grid_table(q)
            rounds.append((o.keys(), o.table(), o.get_particles()["id"]))
        o.finalise(q)
        o.step(q)
        _PILES[overflow] = sc, rounds, o.get_particles()
    return _PILES[overflow]


@pytest.mark.parametrize("row_major", [1, 0])
@pytest.mark.parametrize("overflow", [False, True], ids=["piles", "piles+overflow"])
def test_more_big_cells_than_sort_workgroups(pkg, oracle, overflow, row_major):
    """k_sort_big_cells runs 64 workgroups, one listed cell each and then the cell 64 further on: 66 cells of BIG_CELL + 1
    members (and, with the overflow bucket over BIG_CELL as well, 67 — that one ordered by (key, source)) put two (three)
    cells into the second trip.  At rest, K = 0; the second round starts from the histogram the first one left."""
    sc, rounds, final = piles_reference(pkg, oracle, overflow)
    p = pkg.default_params(0, T.PILE_SIDE)
    p.constant_force[:] = (0.0, 0.0, 0.0)
    s = solver(pkg, sc, row_major)
    for rnd, (keys, table, ids) in enumerate(rounds):
        s.stage("predict", p)
        s.stage("sort", p)
        assert np.array_equal(s.keys().astype(np.uint64), keys), rnd
        assert np.array_equal(s.table().astype(np.uint64), table), rnd
        assert np.array_equal(s.download()["id"], ids), rnd
    s.stage("finalise", p)
    s.step(p)
    assert_state_equal(s.download(), final, "step after the piles")
