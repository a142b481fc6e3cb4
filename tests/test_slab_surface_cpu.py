"""What tests/test_slab_surface_gpu.py relies on, proven without a GPU.

  * owned_planes: which node planes of the global lattice a rank owns, restated from k_mc_field's node-cell expression
    (trunc(N(x) / N(res)), pbf_mc.hpp) and NOT from the host's first_node loop; the ranges tile the lattice, are
    contiguous and ascending, and exactly the expected (cuts, resolution) pairs leave an interior rank without a plane.
  * the parameter sets of mc_scenes.SLAB_PARAMS that tests/test_mc_nversion_cpu.py does not already hold: the oracle's
    single-domain surface stays inside nversion_mc's bound on them, with a non-trivial mesh.
  * the check bites: a lattice evaluated with every particle fails nversion_mc.compare against the evaluation that
    lacks the column across a cut (a missing or stale ghost layer), at nodes of the planes next to that cut; and a rank's
    block of planes shifted by one plane (a wrong nodeX0) fails against the full evaluation.
"""
import numpy as np
import pytest

import mc_scenes as M
import nversion_mc as NM
import test_mc_nversion_cpu as T

RESOLUTIONS = (0.4, 0.7, 1.0, 1.5, 2.0, 3.0)
CUTS = sorted({(c["extent_x"], c["columns"]) for c in M.SLAB_PARAMS.values()})


def owned_planes(cuts, res, extent_x, dtype):
    """-> per rank the node indices x of the global lattice with cuts[r] <= trunc(N(x) / N(res)) < cuts[r + 1]."""
    t = np.dtype(dtype).type
    sample_x = int(np.floor(t(extent_x) * t(res))) + 1                   # ompsph.hpp:283-284
    cell = (np.arange(sample_x).astype(dtype) / t(res)).astype(np.int64)  # ompsph.hpp:293-298, as k_mc_field divides
    return [np.nonzero((cell >= cuts[r]) & (cell < cuts[r + 1]))[0] for r in range(len(cuts) - 1)]


def plane_ranges(cuts, res, extent_x, dtype):
    """-> (sample_x, [(x0, count) per rank]); an empty rank's x0 is where its planes would begin."""
    own = owned_planes(cuts, res, extent_x, dtype)
    n = [len(o) for o in own]
    x0 = np.concatenate([[0], np.cumsum(n)])
    for r, o in enumerate(own):
        assert np.array_equal(o, np.arange(x0[r], x0[r] + n[r])), (cuts, res, r, o)
    return int(x0[-1]), [(int(x0[r]), n[r]) for r in range(len(n))]


def refused(cuts, res, extent_x, dtype):
    """A rank with a left neighbour owns no plane while planes remain to its right."""
    sample_x, rng = plane_ranges(cuts, res, extent_x, dtype)
    return any(n == 0 and x0 < sample_x for x0, n in rng[1:])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_owned_planes_tile_the_lattice(dtype):
    empty = set()
    for extent_x, cuts in CUTS:
        for res in RESOLUTIONS:
            t = np.dtype(dtype).type
            own = owned_planes(cuts, res, extent_x, dtype)
            sample_x = int(np.floor(t(extent_x) * t(res))) + 1
            assert np.array_equal(np.concatenate(own), np.arange(sample_x)), "tiles [0, sample_x), ascending across ranks"
            for o in own:
                assert len(o) == 0 or np.array_equal(o, np.arange(o[0], o[0] + len(o))), "contiguous"
            assert plane_ranges(cuts, res, extent_x, dtype)[0] == sample_x
            if refused(cuts, res, extent_x, dtype):
                empty.add((cuts, res))
            # a rank w columns wide owns the integers of [c res, (c + w) res): never empty once w res >= 1
            for r in range(1, len(cuts) - 2):
                if (cuts[r + 1] - cuts[r]) * res >= 1:
                    assert len(own[r]) > 0, (cuts, res, r)
    # the one-column slab [3, 4): [1.2, 1.6) and [2.1, 2.8) hold no integer; everything else does
    assert empty == {((0, 3, 4, 7, 1024), 0.4), ((0, 3, 4, 7, 1024), 0.7)}, empty


def test_the_refused_sets_are_the_marked_ones(pkg):
    from pbf_sph_amd import slab
    for name, case in M.SLAB_PARAMS.items():
        kind, at = case["cuts"].split(":")
        inner = [slab.column_of(float(v)) if kind == "x" else int(v) for v in at.split(",")]
        assert case["columns"] == (0, *inner, 1024), "the columns the worker derives from --cuts"
        ext = case["extent_x"]
        assert ext == M.lattice_of(M.make(case["scene"]), (1.0,), False).extent[0] == \
            M.lattice_of(M.make(case["scene"]), (1.0,), True).extent[0]
        for mc in case["sets"]:
            marked = mc[0] == "!"
            res = mc[1] if marked else mc[0]
            for dtype in (np.float32, np.float64):
                assert refused(case["columns"], res, ext, dtype) == marked, (name, mc)
    _, rng = plane_ranges((0, 3, 7, 1024), 0.7, 10, np.float32)
    assert [n for _, n in rng] == [3, 2, 3], "uneven planes per column at resolution 0.7"


NEW_SETS = sorted({(c["scene"], tuple(mc)) for c in M.SLAB_PARAMS.values() for mc in c["sets"]
                   if mc[0] != "!" and tuple(mc) not in [tuple(x) for x in M.PARAMS[c["scene"]]]})


@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("name,mc", NEW_SETS, ids=[f"{n}-{mc[0]}" for n, mc in NEW_SETS])
def test_oracle_field_within_derived_bound_on_the_new_sets(name, mc, fp64):
    rep = T.held(name, fp64, mc)
    print(name, mc, "f64" if fp64 else "f32", NM.summary(rep))
    assert rep["pattern_bad"] == 0
    assert rep["worst"] <= 1, NM.summary(rep)
    assert rep["left_out"] <= 0.01 * rep["with_hits"], NM.summary(rep)
    if fp64:
        assert rep["rv_bar"] <= 1
    assert rep["with_hits"] > 40 and len(rep["mesh"]["vs"]) >= 3 * 80, "the isolevel must give a non-trivial mesh"


def test_new_sets_are_what_they_should_be():
    assert NEW_SETS == [("faces", M.FACES_07)]
    s, _, _, st, cells = T.oracle_state("faces", False)
    lat = M.lattice_of(s, M.FACES_07, False)
    v = NM.evaluate(st["pos"], st["colour"], st["type"], cells, lat, M.FACES_07[2], M.FACES_07[3])["v"]
    assert v[v > 0].min() < M.FACES_07[1] < v.max(), "isolevel inside the range of v"


# ---- the check bites ---------------------------------------------------------------------------------------------------

def full_lattice(name, fp64, mc):
    """-> (state, cells, lattice geometry, pn, c) with pn / c the float64 evaluation on every particle."""
    s, _, _, st, cells = T.oracle_state(name, fp64)
    lat = M.lattice_of(s, mc, fp64)
    ev = NM.evaluate(st["pos"], st["colour"], st["type"], cells, lat, mc[2], mc[3])
    return st, cells, lat, np.column_stack([ev["v"], ev["nrm"]]), ev["c"], ev


def failing_nodes(rep, pn):
    """Nodes that alone make compare() fail: outside the bound, or carrying a value where the evaluation has no hit."""
    worst = np.maximum(np.maximum(rep["node_rv"], rep["node_rn"]), rep["node_rc"])
    return (rep["plain"] & (worst > 1)) | (rep["empty"] & (pn[:, 0] != 0))


BITE = [(n, d) for n, c in M.SLAB_PARAMS.items() for d in c["fp64"]]


@pytest.mark.parametrize("case,fp64", BITE, ids=[f"{n}-{'f64' if d else 'f32'}" for n, d in BITE])
def test_a_missing_ghost_layer_is_caught(case, fp64):
    c = M.SLAB_PARAMS[case]
    mc = c["sets"][0]
    dtype = np.float64 if fp64 else np.float32
    st, cells, lat, pn, cc, ev = full_lattice(c["scene"], fp64, mc)
    ok = NM.compare(pn, cc, st["pos"], st["colour"], st["type"], cells, lat, mc[2], mc[3], dtype)
    assert ok["worst"] <= 1 and ok["pattern_bad"] == 0, "the full evaluation against itself"
    fluid = st["type"] != NM.OBSTACLE
    plane_cell = np.repeat(lat.node_cell[0], int(lat.sample[1] * lat.sample[2]))   # x-major: the cell of each node's plane
    bitten = 0
    for cut in c["columns"][1:-1]:
        # (the column a rank lacks, the cell of its planes next to the cut): the right rank without the copies of column
        # cut - 1, the left rank without those of column cut
        for lacking, at in ((cut - 1, cut), (cut, cut - 1)):
            keep = cells[:, 0] != lacking
            if not (fluid & ~keep).any():
                continue
            rep = NM.compare(pn, cc, st["pos"][keep], st["colour"][keep], st["type"][keep], cells[keep], lat, mc[2], mc[3],
                             dtype)
            bad = failing_nodes(rep, pn)
            print(case, "column", lacking, "missing:", NM.summary(rep), "failing nodes in the adjacent planes",
                  int((bad & (plane_cell == at)).sum()))
            assert rep["worst"] > 1 or rep["pattern_bad"] > 0
            # (obstacles-3, column 6: obstacles and fluid beyond them, out of the left rank's reach — nothing to miss there)
            if ((rep["ev"]["hits"] != ev["hits"]) & (plane_cell == at)).any():
                assert (bad & (plane_cell == at)).any(), (case, lacking, at)
                bitten += 1
    if case == "blob-empty":   # what the case is for: nothing to copy, and no particle within reach of the empty ranks' planes
        own = np.concatenate(owned_planes(c["columns"], mc[0], int(lat.extent[0]), dtype)[1:])
        nodes = np.isin(np.repeat(np.arange(lat.sample[0]), int(lat.sample[1] * lat.sample[2])), own)
        assert bitten == 0 and len(own) > 0 and (ev["hits"][nodes] == 0).all()
        assert not (cells[:, 0] >= 20).any()
    else:
        assert bitten >= 2, "both sides of a cut"
    if case == "blob-3":
        assert (cells[:, 0] == 12).any() and not np.isin(cells[:, 0], (10, 11)).any()
    if case == "obstacles-3":
        assert (~fluid & np.isin(cells[:, 0], (5, 6))).sum() > 100, "obstacles on both sides of the first cut"
    if case == "faces-4":
        assert (fluid & (cells[:, 0] == 3)).sum() > 50, "the one-column slab holds particles"


@pytest.mark.parametrize("case,fp64", BITE, ids=[f"{n}-{'f64' if d else 'f32'}" for n, d in BITE])
def test_a_shifted_plane_is_caught(case, fp64):
    c = M.SLAB_PARAMS[case]
    mc = c["sets"][0]
    dtype = np.float64 if fp64 else np.float32
    st, cells, lat, pn, cc, ev = full_lattice(c["scene"], fp64, mc)
    sx, per = int(lat.sample[0]), int(lat.sample[1] * lat.sample[2])
    _, rng = plane_ranges(c["columns"], mc[0], int(lat.extent[0]), dtype)
    hits = ev["hits"].reshape(sx, per)
    bitten = 0
    for r, (x0, n) in enumerate(rng):
        if r == 0 or n == 0 or not hits[x0:x0 + n].any():
            continue
        # rank r computed its planes one node plane to the right of where they belong
        src = np.minimum(np.arange(x0, x0 + n) + 1, sx - 1)
        pn2, cc2 = pn.reshape(sx, per, 4).copy(), cc.reshape(sx, per, 4).copy()
        pn2[x0:x0 + n], cc2[x0:x0 + n] = pn2[src], cc2[src]
        rep = NM.compare(pn2.reshape(-1, 4), cc2.reshape(-1, 4), st["pos"], st["colour"], st["type"], cells, lat, mc[2],
                         mc[3], dtype)
        bad = failing_nodes(rep, pn2.reshape(-1, 4)).reshape(sx, per)
        print(case, "rank", r, "shifted:", NM.summary(rep), "failing nodes in its first plane", int(bad[x0].sum()))
        assert rep["worst"] > 1 or rep["pattern_bad"] > 0
        assert bad[x0:x0 + n].any() and not bad[:x0].any()
        bitten += 1
    assert bitten >= (0 if case == "blob-empty" else 1)
