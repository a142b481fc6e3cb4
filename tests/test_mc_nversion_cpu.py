"""The oracle's marching-cubes field against tests/nversion_mc.py: an all-pairs float64 evaluation written from the
reference's text (ompsph.hpp:277-356) alone, with bounds derived from rounding counts, on scenes that reach the clamp
folds, the nodes outside the grid, a particle on a node, the strict threshold and obstacles (tests/mc_scenes.py).

The same comparison runs against the device in tests/test_mc_field_gpu.py.  Here, without a GPU: the oracle in fp32
and fp64 on every scene and parameter set, the proof that each scene exercises its mechanism, six mutations of the
evaluation that the unmutated oracle must violate the bound against (the bound bites), the far-node pattern, and the
closed forms of tests/mc_closed_forms.py on the oracle.
"""
import numpy as np
import pytest

import mc_closed_forms as CF
import mc_scenes as M
import nversion_mc as NM
import oracle_lib as O

_STATE = {}


def oracle_state(name, fp64, scene=None):
    """-> (scene, oracle, params, state after the last step, predict-time cells), cached per scene and precision."""
    key = (name, fp64)
    if scene is not None or key not in _STATE:
        s = scene or M.make(name)
        dt = np.float64 if fp64 else np.float32
        o = O.Oracle(fp64, device_pow=True)
        o.set_particles(**M.cast(s["sc"], dt))
        q = M.oracle_params(s, threads=4)
        for _ in range(s["frames"] - 1):
            o.step(q)
        before = o.get_particles()
        o.step(q)
        st = o.get_particles()
        out = (s, o, q, st, M.predict_time_cells(before, s, st["id"]))
        if scene is not None:
            return out
        _STATE[key] = out
    return _STATE[key]


def oracle_engine(s, fp64):
    _, o, q, st, cells = oracle_state(None, fp64, scene=s)
    return st, (lambda mc: o.surface(q, O.OracleMc(*mc))), cells


lattice_of, exact_nodes = M.lattice_of, M.exact_nodes


def held(name, fp64, mc, mutate=None, device_sqrt=False):
    s, o, q, st, cells = oracle_state(name, fp64)
    lat = lattice_of(s, mc, fp64)
    fluid = st["type"] != NM.OBSTACLE
    assert (cells[fluid] >= 0).all() and (cells[fluid] < lat.extent).all(), "a particle outside the grid"
    o.set_device_sqrt(device_sqrt)
    try:
        w = o.surface(q, O.OracleMc(*mc))
    finally:
        o.set_device_sqrt(False)
    assert list(w["sample"]) == list(lat.sample)
    rep = NM.compare(w["pn"], w["c"], st["pos"], st["colour"], st["type"], cells, lat, mc[2], mc[3], o.dtype,
                     mutate=mutate, exact_nodes=exact_nodes(name, lat, mc))
    rep["mesh"] = w
    return rep


def violates(rep):
    return rep["worst"] > 1 or rep["pattern_bad"] > 0


CASES = [(n, mc, fp64) for n in M.NAMES for mc in M.PARAMS[n] for fp64 in (False, True)]


@pytest.mark.parametrize("name,mc,fp64", CASES, ids=[f"{n}-{mc[0]}-{mc[3]}-{'f64' if d else 'f32'}" for n, mc, d in CASES])
def test_oracle_field_within_derived_bound(name, mc, fp64):
    rep = held(name, fp64, mc)
    print(name, mc, "f64" if fp64 else "f32", NM.summary(rep))
    assert rep["pattern_bad"] == 0
    assert rep["worst"] <= 1, NM.summary(rep)
    assert rep["left_out"] <= 0.01 * rep["with_hits"], NM.summary(rep)
    if fp64:
        assert rep["rv_bar"] <= 1, "fp64 must also meet 1e-12 of the sum of |terms|"
    ev = rep["ev"]
    assert rep["with_hits"] > 40 and len(rep["mesh"]["vs"]) >= 3 * 80, "the isolevel must give a non-trivial mesh"
    # far nodes: everything the evaluation did not visit, and every visited node without a hit, is 0 / NaN / NaN
    far = ~ev["evaluated"]
    if "early" in ev:
        far[ev["early"]] = False
    pn, c = rep["mesh"]["pn"], rep["mesh"]["c"]
    assert (pn[far, 0] == 0).all() and np.isnan(pn[far, 1:]).all() and np.isnan(c[far]).all()
    if name == "on_node":
        lat = lattice_of(M.make(name), mc, fp64)
        k = M.on_node_index(mc)
        # (elsewhere a node may or may not round onto the particle: compare() holds whichever the evaluation finds)
        if k is not None:
            assert rep["infinite"].sum() == 1
            i = int(lat.index(*k))
            assert pn[i, 0] == np.inf and np.isnan(pn[i, 1:]).all() and rep["infinite"][i]
        if mc[0] == 2.0:                                      # the rest of the node block: compared, none left out
            blk = [lat.index(x, y, z) for x in range(*M.BLOCK[0]) for y in range(*M.BLOCK[1]) for z in range(*M.BLOCK[2])]
            rest = [j for j in blk if j != i]
            assert (rep["plain"][rest] | rep["empty"][rest]).all()


HALF = [(n, mc, fp64) for n, mc, fp64 in CASES if mc[3] == 0.5]
OTHER = [(n, mc, fp64) for n, mc, fp64 in CASES if mc[3] != 0.5]
case_id = lambda c: f"{c[0]}-{c[1][0]}-{c[1][3]}-{'f64' if c[2] else 'f32'}"


def surfaces(name, fp64, mc):
    """-> the oracle's surface with std::pow and with the second substitution (sqrt for influence 0.5)."""
    _, o, q, _, _ = oracle_state(name, fp64)
    a = o.surface(q, O.OracleMc(*mc))
    o.set_device_sqrt(True)
    try:
        b = o.surface(q, O.OracleMc(*mc))
    finally:
        o.set_device_sqrt(False)
    return a, b


@pytest.mark.parametrize("name,mc,fp64", HALF, ids=[case_id(c) for c in HALF])
def test_oracle_sqrt_field_within_derived_bound(name, mc, fp64):
    """The second documented substitution — sqrt(len) for pow(len, 0.5) — leaves the oracle's field inside the
    unchanged bounds of tests/nversion_mc.py: every scene x influence-0.5 set x precision."""
    assert len(HALF) == 2 * 2 * len(M.NAMES)
    rep = held(name, fp64, mc, device_sqrt=True)
    print("sqrt", name, mc, "f64" if fp64 else "f32", NM.summary(rep))
    assert rep["pattern_bad"] == 0
    assert rep["worst"] <= 1, NM.summary(rep)
    assert rep["left_out"] <= 0.01 * rep["with_hits"], NM.summary(rep)
    if fp64:
        assert rep["rv_bar"] <= 1, "fp64 must also meet 1e-12 of the sum of |terms|"
    assert rep["with_hits"] > 40 and len(rep["mesh"]["vs"]) >= 3 * 80


@pytest.mark.parametrize("name,mc,fp64", OTHER, ids=[case_id(c) for c in OTHER])
def test_sqrt_switch_changes_no_bit_off_influence_half(name, mc, fp64):
    a, b = surfaces(name, fp64, mc)
    for k in ("sample", "pn", "c", "vs", "ns", "cs"):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name,mc,fp64", HALF, ids=[case_id(c) for c in HALF])
def test_sqrt_and_pow_fields_agree_within_the_old_tolerance(name, mc, fp64):
    """How far the libm pow(len, 0.5) is from the correctly rounded root, seen through the field: printed (information),
    and held to the tolerance tests/test_mc.py::test_surface_gpu_vs_oracle used while it compared across the two."""
    a, b = surfaces(name, fp64, mc)
    va, vb = a["pn"][:, 0], b["pn"][:, 0]
    fin = np.isfinite(va) & np.isfinite(vb)
    it = np.int64 if fp64 else np.int32
    ulps = np.abs(va[fin].view(it).astype(np.int64) - vb[fin].view(it).astype(np.int64))   # (v >= 0: same sign)
    whole = (a["pn"].view(it) != b["pn"].view(it)).any(axis=1) & ~np.isnan(a["pn"]).any(axis=1)
    print(f"POW-VS-SQRT {name} {mc} {'f64' if fp64 else 'f32'}: v differs on {int((ulps > 0).sum())} of {int(fin.sum())} "
          f"finite nodes, by at most {int(ulps.max())} ulp; pn differs on {int(whole.sum())} nodes; triangles "
          f"{len(a['vs']) // 3} vs {len(b['vs']) // 3}")
    assert np.array_equal(np.isfinite(va), np.isfinite(vb))
    tol = 2e-6 if not fp64 else 1e-13
    np.testing.assert_allclose(va, vb, rtol=tol, atol=tol * 100)
    assert np.array_equal(np.isnan(a["c"]), np.isnan(b["c"]))
    np.testing.assert_allclose(np.nan_to_num(a["pn"]), np.nan_to_num(b["pn"]), rtol=1e-4, atol=1e-4)


def test_faces_scene_reaches_the_folds_and_the_nodes_outside_the_grid():
    for fp64 in (False, True):
        s, _, _, st, cells = oracle_state("faces", fp64)
        assert np.array_equal(cells[np.argsort(st["id"])], s["placed_cells"]), "the particles stay in their cells"
        for mc in M.PARAMS["faces"]:
            lat = lattice_of(s, mc, fp64)
            assert tuple(lat.extent) == M.FACES_EXT
            ev = NM.evaluate(st["pos"], st["colour"], st["type"], cells, lat, mc[2], mc[3])
            hit = ev["hits"] > 0
            assert {1, 2, 4, 8} <= set(np.unique(ev["wmax"][hit]).astype(int)), "weights 2, 4 and 8 must all occur"
            whole = [float(e * mc[0]).is_integer() for e in lat.extent]
            assert whole == ([True, False, True] if mc[0] == 1.5 else [True] * 3)
            shape = tuple(int(x) for x in lat.sample)
            H = hit.reshape(shape)
            for ax in range(3):
                last = lat.node_cell[ax] == lat.extent[ax]
                assert last.any() == whole[ax]
                if whole[ax]:
                    assert np.take(H, np.nonzero(last)[0], axis=ax).sum() > 10, "nodes outside the grid must have hits"
            assert ("early" in ev) == all(whole), "the (ext, ext, ext) node exists iff extent * res is whole on all axes"


def test_obstacles_scene_has_obstacles_inside_the_threshold_of_many_nodes():
    s, _, _, st, cells = oracle_state("obstacles", True)
    assert 100 < (st["type"] == 1).sum() < 600
    mc = M.PARAMS["obstacles"][0]
    lat = lattice_of(s, mc, True)
    a = NM.evaluate(st["pos"], st["colour"], st["type"], cells, lat, mc[2], mc[3])
    b = NM.evaluate(st["pos"], st["colour"], st["type"], cells, lat, mc[2], mc[3], mutate="obstacles")
    assert (a["v"] != b["v"]).sum() > 500


@pytest.mark.parametrize("fp64", [False, True])
def test_on_node_scene_is_exact(fp64):
    """The particle's stored position equals the node's coordinate bit for bit, computed the reference's way in the
    precision under test, and the six pairs at one threshold are exact too."""
    t = np.float64 if fp64 else np.float32
    s, _, _, st, _ = oracle_state("on_node", fp64)
    p = st["pos"][st["id"] == 0][0]
    assert p.dtype == t
    h, scale = t(s["h"]), t(s["scale"])
    for res, k in ((t(2), np.array(M.ON_NODE)), (t(1), np.array(M.ON_NODE) // 2)):
        step = h / res
        min_e = np.asarray(s["min_bound"], t) / scale - h * t(2)
        a = (min_e + k.astype(t) * step) * scale
        assert a.dtype == t and np.array_equal(a, p), (a, p)
        assert np.array_equal((p / scale) * scale, p)
        a2 = (min_e + (k + np.array([2, 0, 0]) * int(res) // 2).astype(t) * step) * scale
        l = p - a2
        assert np.sqrt((l * l).sum(dtype=t)) == h * scale
    near = st["pos"][st["id"] == 1][0].astype(np.float64)
    node = -128.0 + 32.0 * np.array(M.NEAR_NODE)
    assert abs(np.linalg.norm(near - node) - 1e-3) < 1e-4


MUTATIONS = [("unit_weight", "faces", 0), ("le", "on_node", 0), ("obstacles", "obstacles", 0),
             ("drop_smallest", "blob", 0), ("flip_sign", "blob", 0), ("clamp_centre", "faces", 1)]


@pytest.mark.parametrize("mutation,name,k", MUTATIONS, ids=[m[0] for m in MUTATIONS])
@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
def test_bound_bites(mutation, name, k, fp64):
    """The unmutated oracle violates the bound against the mutated evaluation: the bound is not loose enough to hide
    the defect the scene was built for."""
    mc = M.PARAMS[name][k]
    assert not violates(held(name, fp64, mc))
    rep = held(name, fp64, mc, mutate=mutation)
    print(mutation, name, "f64" if fp64 else "f32", NM.summary(rep))
    assert violates(rep), NM.summary(rep)


@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
def test_oracle_one_particle_closed_form(fp64):
    print(CF.check_one_particle(oracle_engine, fp64))


@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
def test_oracle_corner_particle_weights(fp64):
    CF.check_corner_particle(oracle_engine, fp64, M.make("faces"))


def test_oracle_blob_mesh_encloses_the_fluid_with_the_reference_winding():
    ok, vol = CF.check_volume_sign(held("blob", False, M.PARAMS["blob"][0])["mesh"])
    assert ok, vol


@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
def test_oracle_one_colour(fp64):
    print(CF.check_one_colour(oracle_engine, fp64, M.make("faces")))


def test_recorded_winding_sign_is_current_and_ours_agrees():
    """tests/golden/ref_mc_winding.npz against the live reference table where oracle/_ref/libref_mc.so was built, and
    against the same row of our generated table everywhere."""
    import ctypes as C
    import importlib.util
    import os

    import test_mc_tables as T
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(T.ROOT, "tests", "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    so = os.path.join(T.ROOT, "oracle", "_ref", "libref_mc.so")
    if os.path.exists(so):
        R = C.CDLL(so)
        R.ref_mc_tri.restype = C.c_uint32
        assert R.ref_mc_tri(1, 3) == 255
        assert mg.mc_winding_sign([R.ref_mc_tri(1, j) for j in range(3)]) == CF.reference_winding()
    _, _, tri = T.load(os.path.join(T.ROOT, "oracle", "mc_tables.h"))
    assert tri[1][3] == 255 and mg.mc_winding_sign(tri[1][:3]) == CF.reference_winding()
