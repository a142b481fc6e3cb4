"""The scenes of tests/trip_scenes.py really enter the second trips — checked with the CPU twin, the oracle and NumPy alone,
before anything is sent to a GPU.  The GPU files (test_slab_trips_gpu.py, test_scene_trips_gpu.py, test_sort_slots_gpu.py)
assert the same conditions again on the runs they compare."""
import numpy as np
import pytest

import scene_cases as S
import trip_scenes as T
from test_slab_cpu import launch


def test_box_scene_moves():
    sc, side = T.box_scene(102400)
    again, _ = T.box_scene(102400)
    assert all(np.array_equal(sc[k], again[k]) for k in sc)      # a fixed seed: every rank builds the same particles
    assert side == 1000.0 and np.array_equal(sc["id"], np.arange(102400))
    cells = np.floor(sc["pos"].astype(np.float64) / T.CELL).astype(np.int64)
    assert cells.min() >= 0 and np.array_equal(cells.max(axis=0), (19, 15, 15))
    per_cell = np.bincount((cells[:, 0] * 16 + cells[:, 1]) * 16 + cells[:, 2], minlength=20 * 256)
    assert per_cell.min() > 0 and abs(per_cell.mean() - 20.0) < 1e-9
    # a step moves a particle by v dt scale = 6.225 v (no force along x and z; gravity adds 0.76 along y): about a third
    # change cell
    after = np.floor((sc["pos"].astype(np.float64) + 6.225 * sc["vel"]) / T.CELL).astype(np.int64)
    moved = np.mean(np.any(after != cells, axis=1))
    assert 0.25 < moved < 0.4, moved
    assert len(np.unique(sc["colour"])) > 100000
    sc64, _ = T.box_scene(102400, fp64=True)
    assert sc64["pos"].dtype == np.float64 and np.array_equal(sc64["pos"].astype(np.float32), sc["pos"])


@pytest.mark.parametrize("steps,iteration,fp64", [(3, 0, False), (2, 0, True), (3, 1, False)], ids=["fp32", "fp64", "K1"])
def test_slab_step_scene_enters_the_second_trips(oracle, pkg, tmp_path, steps, iteration, fp64):
    args = ("--scene", T.STEP_SCENE, "--steps", str(steps), "--iteration", str(iteration), "--cuts", T.STEP_CUTS) + \
        (("--fp64",) if fp64 else ())
    ora = launch(T.STEP_WORLD, str(tmp_path), "--engine", "oracle", "--trace", *args)
    T.check_step_trips(ora, steps)
    ids = np.sort(np.concatenate([r["id"] for r in ora]))
    assert np.array_equal(ids, np.arange(102400, dtype=np.uint64))
    assert all(np.isfinite(r[k]).all() for r in ora for k in ("pos", "vel", "colour"))
    assert all(int(r["exchanges"]) == steps * (2 + 2 * iteration) for r in ora)


def test_staged_scene_enters_the_second_trips(oracle, pkg, tmp_path):
    ora = launch(T.STAGED_WORLD, str(tmp_path), "--engine", "oracle", "--trace", "--scene", T.STAGED_SCENE, "--steps", "2",
                 "--iteration", "0", "--cuts", T.STAGED_CUTS)
    T.check_staged_trips(ora, 2)
    assert all(int(r["migrated"]) > 0 and int(r["ghosts"]) > 0 for r in ora)
    ids = np.sort(np.concatenate([r["id"] for r in ora]))
    assert np.array_equal(ids, np.arange(286720, dtype=np.uint64))


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_drain_scene_enters_the_second_trip(oracle, fp64):
    dt = np.float64 if fp64 else np.float32
    sc = T.drain_scene(fp64)
    assert len(sc["id"]) == T.DRAIN_N == 263245 and (sc["type"] == 1).sum() == len(range(17, T.DRAIN_N, 50))
    tiles = np.arange(T.DRAIN_N) // T.DRAIN_TILE
    assert tiles.max() == 257 and np.array_equal(np.unique(tiles[sc["type"] == 1]), np.arange(258))
    want = S.np_drain(sc, T.DRAINS_MIXED, dt)
    T.check_drain_trips(sc, want)
    o = oracle.Oracle(fp64, device_pow=True)       # (the oracle's drain and the NumPy one agree: either is the reference)
    o.set_particles(**sc)
    assert S.same(o.drain(T.DRAINS_MIXED).get_particles(), want)
    # the Z-sorted set behind a step: the second drain takes a good part of what is left
    q = oracle.make_params(iteration=0, max_bound=(T.DRAIN_SIDE,) * 3, mode=oracle.JACOBI, sort=oracle.SORT_STABLE)
    o.step(q)
    mid = o.get_particles()
    again = S.np_drain(mid, T.DRAINS_SECOND, dt)
    assert 0.05 < 1.0 - len(again["id"]) / len(mid["id"]) < 0.5
    assert len(again["id"]) > 128 * T.DRAIN_TILE                           # still many tiles
    # nothing / everything
    assert S.same(S.np_drain(sc, T.DRAINS_NOWHERE, dt), sc)
    rest = S.np_drain(sc, T.DRAINS_ALL, dt)
    assert np.array_equal(rest["id"], sc["id"][sc["type"] == 1])
    # the sheet behind particle 263 244: the drains take part of it
    grown = S.np_emit(sc, T.SHEET_SOURCES, dt)
    assert len(grown["id"]) == T.DRAIN_N + T.SHEET_COUNT and (grown["id"][T.DRAIN_N:] == 900001).all()
    left = S.np_drain(grown, T.SHEET_DRAINS, dt)
    sheet_left = int((left["id"] == 900001).sum())
    assert 0 < sheet_left < T.SHEET_COUNT, sheet_left
    assert len(left["id"]) - sheet_left < T.DRAIN_N


@pytest.mark.parametrize("overflow", [False, True], ids=["piles", "piles+overflow"])
def test_pile_scene_lists_more_cells_than_workgroups(oracle, overflow):
    sc = T.piles_scene(overflow)
    n = T.PILES * (T.BIG_CELL + 1) + 500 + (T.BIG_CELL + 52 if overflow else 0)
    assert len(sc["id"]) == n
    cells = T.pile_cell_of(sc["pos"])
    inside = np.all((cells >= 2) & (cells < 12), axis=1)
    code, members = np.unique(cells[inside] @ (1, 14, 196), return_counts=True)
    big = code[members > T.BIG_CELL]
    assert len(big) == T.PILES and (members[members > T.BIG_CELL] == T.BIG_CELL + 1).all()
    xyz = np.stack([big % 14, big // 14 % 14, big // 196], axis=1)
    gap = np.abs(xyz[:, None, :] - xyz[None, :, :]).max(axis=2)
    assert (gap[~np.eye(len(big), dtype=bool)] >= 2).all()     # no two piles are neighbours
    assert not np.array_equal(sc["pos"], sc["pos"][np.lexsort(cells.T)])   # (upload order is not cell order)
    q = oracle.make_params(iteration=0, force=(0.0, 0.0, 0.0), max_bound=(T.PILE_SIDE,) * 3, mode=oracle.JACOBI,
                           sort=oracle.SORT_STABLE)
    o = oracle.Oracle(False, device_pow=True)
    o.set_particles(**sc)
    o.predict(q)
    T.check_pile_trips(o.keys(), overflow)
    o.sort(q).grid_table(q)
    assert len(o.table()) == T.PILE_TABLE_N                      # the grid the scene was built for
