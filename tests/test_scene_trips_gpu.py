"""Drains on more tiles than k_drain_scan takes in one trip (256 tiles of 1 024 particles): 263 245 particles in upload order
= 256 tiles, one full tile in the second trip and a partial last one, every tile with fluid and obstacles.  The survivors'
bases behind tile 255 are the first trip's carry plus the second's prefix; tests/test_scene_resident_gpu.py stays at 2 tiles.
Bit for bit against the NumPy restatement of tests/scene_cases.py and the oracle; the scene and its conditions are in
tests/trip_scenes.py (checked without a GPU by tests/test_scan_trips_cpu.py)."""
import numpy as np
import pytest

import scene_cases as S
import trip_scenes as T

pytestmark = pytest.mark.gpu
BOTH = pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
_SCENES = {}


def scene(fp64):
    if fp64 not in _SCENES:
        _SCENES[fp64] = T.drain_scene(fp64)
    return {k: v.copy() for k, v in _SCENES[fp64].items()}


def make(pkg, oracle, sc, fp64, reserve=0):
    s = pkg.Solver(h=S.H, fp64=fp64)
    if reserve:
        s.reserve(reserve)
    s.upload(**sc)
    q = oracle.make_params(iteration=0, max_bound=(T.DRAIN_SIDE,) * 3, mode=oracle.JACOBI, sort=oracle.SORT_STABLE)
    return s, pkg.default_params(0, T.DRAIN_SIDE), q


@BOTH
def test_mixed_drain(pkg, oracle, fp64):
    dt = np.float64 if fp64 else np.float32
    sc = scene(fp64)
    want = S.np_drain(sc, T.DRAINS_MIXED, dt)
    T.check_drain_trips(sc, want)
    s, p, q = make(pkg, oracle, sc, fp64)
    s.set_drains(T.DRAINS_MIXED).stage("scene", p)
    assert s.n == len(want["id"])
    assert S.same(s.download(), want)                  # the order kept, every field
    # a step behind it (the drains still set: they find nothing more) against the oracle
    o = oracle.Oracle(fp64, device_pow=True)
    o.set_particles(**want)
    s.step(p)
    S.oracle_frame(oracle, o, q, [], T.DRAINS_MIXED)
    mid = o.get_particles()
    assert s.n == len(mid["id"]) == len(want["id"]) and S.same(s.download(), mid)
    # and the Z-sorted set drained again, elsewhere
    again = S.np_drain(mid, T.DRAINS_SECOND, dt)
    assert 0 < len(again["id"]) < 0.95 * len(mid["id"])
    s.set_drains(T.DRAINS_SECOND).stage("scene", p)
    assert s.n == len(again["id"]) and S.same(s.download(), again)


@BOTH
def test_nothing_drained(pkg, oracle, fp64):
    sc = scene(fp64)
    s, p, _ = make(pkg, oracle, sc, fp64)
    s.set_drains(T.DRAINS_NOWHERE)
    before = s.scene_host_syncs()
    s.stage("scene", p)
    assert s.scene_host_syncs() == before + 1
    assert s.n == T.DRAIN_N and S.same(s.download(), sc)


@BOTH
def test_everything_drained(pkg, oracle, fp64):
    sc = scene(fp64)
    want = {k: v[sc["type"] == 1] for k, v in sc.items()}
    s, p, q = make(pkg, oracle, sc, fp64)
    s.set_drains(T.DRAINS_ALL).stage("scene", p)
    assert s.n == len(want["id"]) == len(range(17, T.DRAIN_N, 50))
    assert S.same(s.download(), want)                  # only the obstacles, in their order
    o = oracle.Oracle(fp64, device_pow=True)
    o.set_particles(**want)
    s.step(p)
    S.oracle_frame(oracle, o, q, [], T.DRAINS_ALL)
    assert S.same(s.download(), o.get_particles())


@BOTH
def test_source_and_drain(pkg, oracle, fp64):
    dt = np.float64 if fp64 else np.float32
    sc = scene(fp64)
    want = S.np_drain(S.np_emit(sc, T.SHEET_SOURCES, dt), T.SHEET_DRAINS, dt)
    sheet = int((want["id"] == 900001).sum())
    assert 0 < sheet < T.SHEET_COUNT and len(want["id"]) - sheet < T.DRAIN_N   # part of the sheet and part of the fluid left
    s, p, _ = make(pkg, oracle, sc, fp64, reserve=T.DRAIN_N + T.SHEET_COUNT)
    s.set_sources(T.SHEET_SOURCES).set_drains(T.SHEET_DRAINS).stage("scene", p)
    assert s.n == len(want["id"]) and S.same(s.download(), want)
