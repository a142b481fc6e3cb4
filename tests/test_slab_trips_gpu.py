"""The slab selects beyond their first single-workgroup trip (scenes and conditions: tests/trip_scenes.py; the conditions
alone, without a GPU: tests/test_scan_trips_cpu.py).  Every test of tests/test_slab_gpu.py gives a rank at most 8 tiles of
1 024 array slots, so the loops of k_slab_scan (64 tiles a trip), k_slab_arrival_ghosts (256 arrivals a trip) and k_sel_scan
(256 tiles a trip) run once there and their carries are never read.  Here:

  * pbf_slab_step, three ranks, the middle one on more than 66 tiles with all four classes of slab_classes4 selected behind
    tile 64, and more than 256 arrivals of which one behind the 256th lands in a boundary column;
  * the staged API (pbf_slab_migrate / pbf_slab_ghosts, driven by slab.py), two ranks, one on more than 258 tiles with
    migrants, stayers and boundary copies behind tile 256;

each bit for bit against the CPU twin.  K = 0 solver iterations but for one case (nothing of the assembly depends on what the
iterations do, and the twin stays fast); the colour diffusion runs every step and reads the copies, so a copy in the wrong
wire slot shows in its neighbours' colours — and in the K = 1 case a field refresh reads ghostSrcL/R entries the late tiles
wrote."""
import numpy as np
import pytest

import trip_scenes as T
from test_slab_cpu import launch, merged

pytestmark = pytest.mark.gpu


def assert_ranks_equal(hip, ora, particles):
    for r, (h, o) in enumerate(zip(hip, ora)):
        for k in ("id", "type", "pos", "vel", "colour"):
            assert np.array_equal(h[k], o[k]), (r, k)
    assert np.array_equal(merged(hip)["id"], np.arange(particles, dtype=np.uint64))   # nothing lost, nothing twice


@pytest.mark.parametrize("steps,iteration,fp64", [(3, 0, False), (2, 0, True), (3, 1, False)], ids=["fp32", "fp64", "K1"])
def test_slab_step_beyond_64_tiles(pkg, tmp_path, steps, iteration, fp64):
    args = ("--scene", T.STEP_SCENE, "--steps", str(steps), "--iteration", str(iteration), "--cuts", T.STEP_CUTS) + \
        (("--fp64",) if fp64 else ())
    ora = launch(T.STEP_WORLD, str(tmp_path / "ora"), "--engine", "oracle", "--trace", *args)
    T.check_step_trips(ora, steps)
    hip = launch(T.STEP_WORLD, str(tmp_path / "hip"), "--engine", "hipc", *args)
    assert hip[1]["pos"].dtype == (np.float64 if fp64 else np.float32)
    assert_ranks_equal(hip, ora, 102400)
    for r in range(T.STEP_WORLD):  # 2 assembly rounds + 2K field refreshes per step, nothing else
        assert int(hip[r]["exchanges"]) == steps * (2 + 2 * iteration), (r, int(hip[r]["exchanges"]))


def test_staged_api_beyond_256_tiles(pkg, tmp_path):
    steps = 2
    args = ("--scene", T.STAGED_SCENE, "--steps", str(steps), "--iteration", "0", "--cuts", T.STAGED_CUTS)
    ora = launch(T.STAGED_WORLD, str(tmp_path / "ora"), "--engine", "oracle", "--trace", *args)
    T.check_staged_trips(ora, steps)
    hip = launch(T.STAGED_WORLD, str(tmp_path / "hip"), "--engine", "hip", *args)
    assert_ranks_equal(hip, ora, 286720)
    for r in range(T.STAGED_WORLD):
        assert int(hip[r]["migrated"]) == int(ora[r]["migrated"]) > 0
        assert int(hip[r]["ghosts"]) == int(ora[r]["ghosts"]) > 0
        assert int(hip[r]["exchanges"]) == int(ora[r]["exchanges"]) == steps * 2
