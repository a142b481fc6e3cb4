"""Slab mode re-counts the re-assembled set (owned particles + the neighbours' copies) with k_count_keys, which is then the
producer of the slots the sort's scatter places by (cellSlot).  A small case of its own: the two cubes at a nominal 4 000 particles (3 456), two ranks sharing
cuda:0, the cut through both cubes, three steps, driven by slab.py's Python protocol (engine "hip": predict, migrate,
ghosts, k_count_keys, sort, ...).

  * two ranks == the CPU twin's two ranks (tests/slab_engines.py: the same protocol on the oracle), bit for bit;
  * two ranks == one rank of the same driver: the same particles, nothing lost or duplicated, and positions to
    summation-order noise — a rank's copies sit behind its own particles, so the order INSIDE a cell, and with it the
    order of the fp32 sums, differs from the single rank's (the bound is tests/test_slab_gpu.py's for this scene family)."""
import numpy as np
import pytest

from test_slab_cpu import launch, merged

pytestmark = pytest.mark.gpu


def test_two_ranks_equal_one_rank(pkg, tmp_path):
    args = ("--scene", "cubes4000", "--steps", "3")
    two = launch(2, str(tmp_path / "two"), "--engine", "hip", "--cuts", "x:210", *args)
    twin = launch(2, str(tmp_path / "twin"), "--engine", "oracle", "--cuts", "x:210", *args)
    one = launch(1, str(tmp_path / "one"), "--engine", "hip", "--cuts", "even", *args)
    for r in range(2):
        for k in ("id", "pos", "vel", "colour", "type"):
            assert np.array_equal(two[r][k], twin[r][k]), (r, k)
        assert int(two[r]["ghosts"]) == int(twin[r]["ghosts"]) > 0
    got, want = merged(two), merged(one)
    assert len(want["id"]) == len(pkg.scene_cubes(4000)["id"])
    assert np.array_equal(got["id"], want["id"])
    assert np.array_equal(got["type"], want["type"])
    d = np.linalg.norm(got["pos"].astype(np.float64) - want["pos"], axis=1)
    assert d.max() <= 2e-2 and d.mean() <= 1e-4, (d.max(), d.mean())
