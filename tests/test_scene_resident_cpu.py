"""CPU side of sources, drains and cell queries on the device-resident path (pbf_set_sources / pbf_set_drains /
pbf_stage_scene / pbf_query_cells): the entry points are declared and exported, the checker itself (Oracle.emit / drain)
is checked against an independent numpy restatement of ompsph.hpp:93-118, and the scenes the GPU tests run are shown —
on the oracle — to exercise what they claim to exercise.  No compute entry point of the product is called here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scene_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pbf_set_sources", "pbf_set_drains", "pbf_stage_scene", "pbf_query_cells", "pbf_scene_host_syncs"]


def test_new_entry_points_declared_exported_and_bound(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pbf_hip.h")).read(), flags=re.S)
    L = C.CDLL(pkg.LIB_PATH)
    from pbf_sph_amd import capi
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in capi.exported_symbols(), name
    assert "typedef struct pbf_source" in hdr and "typedef struct pbf_drain" in hdr
    assert C.sizeof(capi.Source) == 8 + 11 * 8 and C.sizeof(capi.Drain) == 4 * 8
    assert "#define PBF_ABI_VERSION 1" in hdr
    for m in ("reserve", "set_sources", "set_drains", "query", "scene_host_syncs"):
        assert hasattr(capi.Solver, m), m


def test_product_does_not_name_the_oracle():
    """the existing rule (tests/test_capi_cpu.py), which the new files of the product fall under too"""
    for base, _, files in os.walk(os.path.join(ROOT, "pbf-sph_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h", "Makefile")):
                txt = open(os.path.join(base, f), errors="ignore").read()
                assert "pbf_oracle" not in txt and "oracle_lib" not in txt, os.path.join(base, f)


def boundary_case(dtype):
    """particles at centre + k (3, 4, 0): distance exactly 5 k; width 5 k keeps them (strict <), the next float removes them"""
    ks = np.arange(1, 9)
    centre = np.array([500.0, 500.0, 500.0])
    pos = centre + ks[:, None] * np.array([3.0, 4.0, 0.0])
    n = len(ks)
    return dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n, dtype), pos=pos.astype(dtype),
                vel=np.zeros((n, 3), dtype), colour=np.full((n, 4), 0.5, dtype)), tuple(centre), ks


@pytest.mark.parametrize("fp64", [False, True])
def test_numpy_restatement_equals_the_oracle(pkg, oracle, fp64):
    dt = np.float64 if fp64 else np.float32
    sc = S.cubes_with_obstacle(pkg, fp64)
    odd = [(1, (300, 200, 100), (0, 0, 0), S.RED, 10.0), (2, (310.5, 200, 100), (1, 2, 3), S.GREEN, 2.0),
           (3, (100, 100, 100), (0, 0, 0), S.RED, 0.5), (4, (-0.0, 700, 800), (0, 0, 0), S.GREEN, 17.3)]
    for sources, drains in (S.shim_scene(sc)[:2], S.main_scene(sc), (odd, [((300, 200, 100), 30.0)])):
        o = oracle.Oracle(fp64)
        o.set_particles(**sc)
        want = S.np_emit(sc, sources, dt)
        assert S.same(o.emit(sources).get_particles(), want)
        assert S.same(o.drain(drains).get_particles(), S.np_drain(want, drains, dt))
    counts = [len(S.np_emit(sc, [s], dt)["id"]) - len(sc["id"]) for s in odd]
    assert counts == [12, 2, 0, 20]       # 3 x 4, 1 x 2, 0 x 1, 4 x 5
    b, centre, ks = boundary_case(dt)
    for k in ks:
        for width, gone in ((5.0 * k, False), (float(np.nextafter(dt(5.0 * k), dt(np.inf))), True)):
            o = oracle.Oracle(fp64)
            o.set_particles(**b)
            got = o.drain([(centre, width)]).get_particles()
            assert S.same(got, S.np_drain(b, [(centre, width)], dt))
            assert (k in got["id"] + 1) != gone and all(j in got["id"] + 1 for j in ks if j > k)


def test_main_scene_exercises_what_the_gpu_tests_claim(pkg, oracle):
    sc = S.cubes_with_obstacle(pkg)
    sources, drains = S.main_scene(sc)
    o = oracle.Oracle(False, device_pow=True)
    o.set_particles(**sc)
    q = oracle.make_params(iteration=4, mode=oracle.JACOBI, sort=oracle.SORT_STABLE)
    counts, born_dead = [], 0
    for frame in range(6):
        if frame == 0:
            e = oracle.Oracle(False)
            e.set_particles(**sc)
            n0 = e.n
            e.emit(sources)
            fresh = e.get_particles()
            kept = S.np_drain(fresh, drains, np.float32)
            born_dead = (fresh["id"] >= 100000).sum() - (kept["id"] >= 100000).sum()
        c, _ = S.oracle_frame(oracle, o, q, sources, drains)
        counts.append(c)
    n0, n1, n2 = counts[0]
    assert 0.01 * n1 <= n1 - n2 <= 0.5 * n1, counts[0]
    assert sum(1 for a, b, c in counts if c < b) >= 4, counts
    assert born_dead >= 1
    seq = [v for c in counts for v in c]
    down = any(a // 256 > b // 256 for a, b in zip(seq, seq[1:]))
    assert down, counts
    # Upwards this scene crosses 1664 = 13 x 128 (a wave-pair boundary of the 256-particle blocks), not a multiple of 256;
    # the upward crossing of a 256 boundary is the growth scene's (below), which the GPU capacity test runs.
    assert any(a // 128 < b // 128 for a, b in zip(seq, seq[1:])), counts
    assert (o.get_particles()["type"] == 1).sum() == 1


def test_growth_scene_crosses_a_block_boundary_upwards(pkg, oracle):
    sc = S.cubes_with_obstacle(pkg, True)
    o = oracle.Oracle(True, device_pow=True)
    o.set_particles(**sc)
    q = oracle.make_params(iteration=4, mode=oracle.JACOBI, sort=oracle.SORT_STABLE)
    seq = [o.n]
    for frame in range(S.GROWTH_FRAMES):
        c, _ = S.oracle_frame(oracle, o, q, S.main_scene(sc)[0], [])
        seq += [c[1], c[2]]
    assert any(a // 256 < b // 256 for a, b in zip(seq, seq[1:])), seq
