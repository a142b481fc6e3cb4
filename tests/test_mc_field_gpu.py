"""k_mc_mark_near + k_mc_field against tests/nversion_mc.py, the all-pairs float64 evaluation of the reference's field
(ompsph.hpp:277-356), within bounds derived from rounding counts: every scene of tests/mc_scenes.py x parameter set x
precision.  The evaluation gets positions, colours and types from the device's own download and the predict-time cells
from nversion.predict + predict_cells on the state before the last step; the step itself is pinned elsewhere.
tests/test_mc_nversion_cpu.py proves on the CPU that the scenes reach the clamp folds, the nodes outside the grid, a
particle on a node, the strict threshold and obstacles, and that the bound bites.  The closed forms of
tests/mc_closed_forms.py run here against the device.
"""
import numpy as np
import pytest

import mc_closed_forms as CF
import mc_scenes as M
import nversion_mc as NM

pytestmark = pytest.mark.gpu


def device_state(pkg, s, fp64):
    dt = np.float64 if fp64 else np.float32
    sol = pkg.Solver(h=s["h"], fp64=fp64)
    sol.upload(**M.cast(s["sc"], dt))
    p = M.device_params(pkg, s)
    for _ in range(s["frames"] - 1):
        sol.step(p)
    before = sol.download()
    sol.step(p)
    st = sol.download()
    return sol, p, st, M.predict_time_cells(before, s, st["id"])


def device_engine(pkg):
    def engine(s, fp64):
        sol, p, st, cells = device_state(pkg, s, fp64)
        return st, (lambda mc: sol.surface(p, pkg.McParams(*mc))), cells
    return engine


CASES = [(n, fp64) for n in M.NAMES for fp64 in (False, True)]


@pytest.mark.parametrize("name,fp64", CASES, ids=[f"{n}-{'f64' if d else 'f32'}" for n, d in CASES])
def test_device_field_within_derived_bound(pkg, name, fp64):
    s = M.make(name)
    sol, p, st, cells = device_state(pkg, s, fp64)
    try:
        for mc in M.PARAMS[name]:
            lat = M.lattice_of(s, mc, fp64)
            fluid = st["type"] != NM.OBSTACLE
            assert (cells[fluid] >= 0).all() and (cells[fluid] < lat.extent).all(), "a particle outside the grid"
            g = sol.surface(p, pkg.McParams(*mc))
            assert list(g["sample"]) == list(lat.sample)
            rep = NM.compare(g["pn"], g["c"], st["pos"], st["colour"], st["type"], cells, lat, mc[2], mc[3], sol.dtype,
                             exact_nodes=M.exact_nodes(name, lat, mc))
            print("RATIO device", name, mc, "f64" if fp64 else "f32", NM.summary(rep))
            assert rep["pattern_bad"] == 0, (mc, NM.summary(rep))
            assert rep["worst"] <= 1, (mc, NM.summary(rep))
            assert rep["left_out"] <= 0.01 * rep["with_hits"], (mc, NM.summary(rep))
            if fp64:
                assert rep["rv_bar"] <= 1, "fp64 must also meet 1e-12 of the sum of |terms|"
            far = ~rep["ev"]["evaluated"]
            if "early" in rep["ev"]:
                far[rep["ev"]["early"]] = False
            assert (g["pn"][far, 0] == 0).all() and np.isnan(g["pn"][far, 1:]).all() and np.isnan(g["c"][far]).all()
            if name == "on_node":
                k = M.on_node_index(mc)
                # (elsewhere a node may or may not round onto the particle: compare() holds whichever the evaluation finds)
                if k is not None:
                    assert rep["infinite"].sum() == 1
                    i = int(lat.index(*k))
                    assert g["pn"][i, 0] == np.inf and np.isnan(g["pn"][i, 1:]).all()
            if name == "blob" and mc == M.PARAMS[name][0]:
                ok, vol = CF.check_volume_sign(g)
                assert ok, vol
    finally:
        sol.close()


@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
def test_device_one_particle_closed_form(pkg, fp64):
    print(CF.check_one_particle(device_engine(pkg), fp64))


@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
def test_device_corner_particle_weights(pkg, fp64):
    CF.check_corner_particle(device_engine(pkg), fp64, M.make("faces"))


@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
def test_device_one_colour(pkg, fp64):
    print(CF.check_one_colour(device_engine(pkg), fp64, M.make("faces")))
