"""The last trip of the list build's test loop is cut to what the wave's longest lane has left (csrc/pbf_kernels.hpp
narrowest_trip; the same cut in the build's drain and in the list reader's head loop was measured and not kept,
profiles/tail_trips_1m.md).  A scene whose waves end their rows AND their lists at every remainder of a full trip — so every
width of the last trip, and the loop without one, runs — must give the bits of the oracle and of the plain per-particle
walk (gather = 0, k_gather_global), stage by stage over two solver iterations."""
import importlib.util
import os

import numpy as np
import pytest

from test_hip_parity import assert_state_equal, mk, oracle_run, params_pair, two_tier_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("sched_probe", os.path.join(ROOT, "tools", "sched_probe.py"))
sched_probe = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sched_probe)

CELL = 50.0   # h * scale with h = 0.1, scale = 500; the box [0, 1000]^3 is 20 cells a side
# one group = three adjacent (y, z) rows of 18 cells along x whose populations cycle 1 .. m, the top cell of a cycle holding
# m + k: the longest run of three cells is 3 m - 3 + k — one group for every length from 9 to 24
GROUPS = [(m, k) for m in (4, 5, 6, 7, 8) for k in (0, 1, 2)] + [(9, 0)]


def staircase_scene(fp64, obstacles=False):
    rng = np.random.default_rng(2013)
    cells = []                                               # (x, y, z, population)
    spots = [(y0, z) for z in (1, 4, 7, 10, 13, 16) for y0 in (1, 6, 11)]
    for g, (m, k) in enumerate(GROUPS):
        y0, z = spots[g]
        for row in range(3):
            for x in range(1, 19):
                step = (x - 1 + 3 * row + g) % m             # (the rows of a group out of phase: lanes of one wave differ)
                cells.append((x, y0 + row, z, step + 1 + (k if step == m - 1 else 0)))
    # one run of several full trips and runs shorter than one pair load: cells of 1 and 2 with nobody around them (lanes done
    # before their wave's first trip ends), and a cell of 1 beside the cell of 40 in y (that wave's longest run in the row
    # dy = +1 is ONE candidate)
    cells += [(3, 3, 19, 1), (10, 7, 19, 2), (10, 10, 19, 40), (10, 11, 19, 1), (16, 16, 19, 2)]
    n = sum(c for _, _, _, c in cells)
    cells.append((16, 3, 19, (1 - n) % 64))                  # n = 1 (mod 64): the last wave is partial
    pos = np.concatenate([(np.array([x, y, z]) + 0.1 + 0.8 * rng.random((c, 3))) * CELL for x, y, z, c in cells if c])
    n = len(pos)
    assert n % 64 == 1 and n <= 4096, n
    dt = np.float64 if fp64 else np.float32
    perm = rng.permutation(n)                                # upload unsorted
    ty = np.zeros(n, np.uint8)
    if obstacles:
        ty[::13] = 1                                         # lanes that leave at op.begin while their wave goes on voting
    return dict(id=np.arange(n, dtype=np.uint64), type=ty, mass=np.ones(n, dt), pos=pos[perm].astype(dt),
                vel=np.zeros((n, 3), dt), colour=rng.uniform(0.03, 1.0, (n, 4)).astype(dt))


def assert_every_width_runs(s):
    """Condition, not a skip: over the scene's waves (64 consecutive row slots) the longest run takes every remainder
    1 .. 8 of the build's 8-slot trip and the longest list every remainder of the reader's 8-entry trip."""
    keys, table, cnt = s.keys().astype(np.int64), s.table(), s.nbr_counts().astype(np.int64)
    assert keys.max() < len(table) - 1, "a walker in no cell: the run-length formula does not describe it"
    assert np.all(np.diff(keys) >= 0)
    assert not np.any(cnt == 0xFFFFFFFF), "an overflowed list: no head loop for it"
    _, L = sched_probe.row_run_lengths(keys)
    lmax, cmax = sched_probe.wave_maxima(cnt, L)             # cnt is in row-slot order already
    runs = lmax[lmax > 0]
    got = {int(v) for v in (runs - 1) % 8 + 1}
    assert got == set(range(1, 9)), ("run remainders", sorted(got))
    assert runs.min() < 2 and runs.max() >= 40, (runs.min(), runs.max())  # shorter than a pair load; several full trips
    head = np.minimum(cmax, 40)
    got = {int(v) for v in head % 8}
    assert got == set(range(8)), ("list remainders", sorted(got))
    return lmax, cmax


@pytest.mark.parametrize("obstacles", [False, True])
@pytest.mark.parametrize("fp64", [False, True])
def test_staircase_every_last_trip_width_bit_exact(pkg, oracle, fp64, obstacles):
    sc = staircase_scene(fp64, obstacles)
    s, o = mk(pkg, oracle, sc, fp64)
    g, _ = mk(pkg, oracle, sc, fp64, gather=0)
    p, q = params_pair(pkg, oracle)
    for stage in ("predict", "sort", "diffuse"):
        s.stage(stage, p), g.stage(stage, p)
    o.predict(q)
    o.sort(q).grid_table(q)
    o.diffuse(q)
    assert np.array_equal(s.keys().astype(np.uint64), o.keys())
    for it in range(2):  # (the second iteration tests candidates that have left their cells)
        s.stage("lambda", p), g.stage("lambda", p)
        o.lambda_(q)
        if it == 0:
            lmax, cmax = assert_every_width_runs(s)
            print("wave maxima: runs", np.bincount(lmax[lmax > 0] % 8, minlength=8), "lists", np.bincount(np.minimum(cmax, 40) % 8, minlength=8))
        assert np.array_equal(s.pstar()[:, 3], o.lambdas()), it
        assert np.array_equal(s.pstar()[:, 3], g.pstar()[:, 3]), it
        s.stage("delta", p), g.stage("delta", p)
        o.delta(q)
        assert np.array_equal(s.pstar()[:, :3], o.pstar()), it
        assert np.array_equal(s.pstar()[:, :3], g.pstar()[:, :3]), it
    s.stage("finalise", p)
    o.finalise(q)
    assert_state_equal(s.download(), o.get_particles(), "finalise")


@pytest.mark.parametrize("chunks", [0, 1])
def test_two_tier_lists_next_to_the_last_trip(pkg, oracle, chunks):
    """Lists that spill into a chunk or walk, next to the last trip of the head loop: one step of the default path."""
    sc, side = two_tier_scene(pkg)
    p, q = params_pair(pkg, oracle, side=side)
    s = pkg.Solver(h=0.1)
    if chunks:
        s.set_option("nbr_chunks", chunks)
    s.upload(**sc)
    want = oracle_run(oracle, ("twotier",), sc, False, q, (0, 2))
    s.step(p)
    assert_state_equal(s.download(), want[0], "frame 0")
