"""Oracle restatement vs the reference's own headers (oracle/_ref/libref_grid.so).

Wider, randomised version of test_oracle_golden.py.  Where oracle/_ref exists (it is built from the reference
when that is present) the reference side is computed live; elsewhere it comes from golden/ref_live.npz, the same
calls' results stored by golden/make_golden.py (tests/ref_live.py holds the calls and their fixed inputs).
"""
import numpy as np
import pytest

import ref_live


@pytest.fixture(scope="module")
def R(oracle):
    return oracle.ref()


@pytest.fixture(scope="module")
def G():
    return dict(np.load(ref_live.FIXTURE))


def test_morton_exhaustive_slices(oracle, R, G):
    L = oracle.lib()
    want = ref_live.morton(R) if R is not None else G
    xyz, codes = ref_live.morton_inputs()
    for (x, y, z), w in zip(xyz, want["morton_enc"]):
        assert L.pbf_oracle_morton_encode(int(x), int(y), int(z)) == w
    for c, w in zip(codes, want["morton_dec"]):
        for a in range(3):
            assert L.pbf_oracle_morton_decode(int(c), a) == w[a]


def test_neighbour_codes_match_foreach_grid(oracle, R, G):
    """The oracle's 27 codes visit exactly what sph::foreach_grid visits on an identity table."""
    L = oracle.lib()
    want = ref_live.foreach_grid(R) if R is not None else G
    tn = int(want["fg_tn"][0])
    homes = ref_live.foreach_homes(tn)
    assert len(homes) == len(want["fg_counts"])
    ends = np.cumsum(want["fg_counts"].astype(np.int64))
    codes = np.empty(27, np.uint64)
    for h, end, k in zip(homes, ends, want["fg_counts"]):
        L.pbf_oracle_neighbour_codes(int(h), ref_live.vp(codes))
        mine = [int(c) for c in codes if c < tn and c + 1 < tn]  # last entry: empty range
        assert list(want["fg_visits"][end - int(k):end]) == mine


@pytest.mark.parametrize("fp64", [False, True])
def test_oracle_table_equals_reference_table_on_a_real_frame(oracle, R, G, fp64):
    nm = "f64" if fp64 else "f32"
    o = ref_live.real_frame(oracle, fp64)
    want = ref_live.grid_table(R, o, fp64) if R is not None else G
    keys = o.keys()
    # the reference's makeGridTable over these keys (stored: the keys it was given must be these)
    assert np.array_equal(keys, want[f"gt_{nm}_keys"])
    assert np.array_equal(want[f"gt_{nm}_table"], o.table())
    # keys recomputed by the reference's zCurveGridIndexAtCoordAt from the oracle's pStar
    assert np.array_equal(ref_live.grid_index_inputs(o, fp64), want[f"gt_{nm}_d"])
    assert np.array_equal(want[f"gt_{nm}_gia"], keys[::ref_live.GIA_STRIDE])


@pytest.mark.parametrize("fp64", [False, True])
def test_scene_matches_reference_factory(oracle, R, G, fp64):
    nm = "f64" if fp64 else "f32"
    for count in ref_live.SCENE_COUNTS:
        want = ref_live.scene_digest(ref_live.scene(R, count, fp64)) if R is not None else G[f"scene_{count}_{nm}"]
        s = oracle.scene_cubes(count, fp64)
        assert np.array_equal(ref_live.scene_digest(s), want), count
