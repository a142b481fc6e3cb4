"""The opt-in velocity passes (vorticity, XSPH, surface tension) on a ctx that has solids: include/pbf_hip.h promises that they
run after the friction pass and "see the boundary-corrected velocity", and they read the pStar the collider and the scenery
projected.

  1. per particle: the scheme of test_extras_paths_gpu.check_against_reference with the solids installed in every twin.  A pass
     leaves ids, positions, pStar, the reaction records, their sums, the friction sums and the obstacles' velocities alone, byte
     for byte; its increment and its records stay inside tests/extras_ref.py's derived bars, evaluated on the `off` twin's own
     pStar, velocity and mass.  No tolerance is new: the bars, ER.AMBIGUOUS_CAP and ER.fast_allowance are used as they are.
     The test discriminates: against the XSPH reference evaluated on the velocity of a twin whose last step ran WITHOUT the
     friction pass — what a pass ordered before friction would have read — the device's increment is outside the bar;
  2. every launch path gives the default path's bytes, the solids' records included;
  3. sequencing, configuration (d) of tests/test_solids_scene_gpu.py with all three passes: a replayed graph, one pbf_steps(p, 4)
     and the stages called one by one give the bytes of four pbf_step.

The CPU side (the ambiguous share of every scene with its solids): tests/test_solids_composed_cpu.py.
"""
import numpy as np
import pytest

import collider_pose_ref as PR
import extras_ref as ER
import scene_cases as S
import solids_scene_cases as SS
import test_extras_paths_gpu as X
from sample_ref import key_cells
from test_collider_body_gpu import first_step_share
from test_collider_friction_gpu import MU, V, W, friction_bytes, staged_step
from test_collider_gpu import IDS, VARIANTS, dt_of, plane_through
from test_collider_pose_gpu import body_lattice_through, install, wrench_bytes
from test_nversion_cpu import scene
from test_scenery_gpu import set_scenery
from test_solids_scene_gpu import differing, snapshot, solids

pytestmark = pytest.mark.gpu

SCENES = ["cloud", "obstacles_moving", "edges65"]


def case_of(name, fp64):
    return body_lattice_through(scene(name), dt_of(fp64), PR.GENERIC, SS.EXTRAS_SHARE[name])


def rubbed_beside_a_wall(s, name, fp64):
    """run()'s hook: the posed collider through the scene's fluid with friction MU, V, W, and a scenery plane"""
    sc = scene(name)
    install(s, case_of(name, fp64), PR.GENERIC).set_collider_friction(MU, V, W)
    return set_scenery(s, plane_through(sc, dt_of(fp64), SS.WALL_SHARE, SS.WALL_N)[1])


def solid_records(s):
    return dict(push=s.collider_push().tobytes(), wrench=wrench_bytes(s), friction=friction_bytes(s))


# ---- 1. per particle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", SCENES)
def test_passes_within_the_derived_bars_beside_the_solids(pkg, name, fp64, fast):
    dtype = dt_of(fp64)
    sc = scene(name)
    share = first_step_share(sc, dtype, case_of(name, fp64), PR.GENERIC)
    print(f"{name}: {100 * share:.1f} % of the fluid starts inside the solid")
    assert 0.1 <= share <= 0.9, share
    kept = {}

    def also(on, off, passes):
        got, want = solid_records(on), solid_records(off)
        assert not differing(got, want), (passes, differing(got, want))
        if passes == ("xsph",):
            kept["off"], kept["dv"] = off, on.download()["vel"].astype(np.float64) - off.download()["vel"].astype(np.float64)

    seen = X.check_against_reference(pkg, name, fp64, fast, solids=rubbed_beside_a_wall, also=also, iteration=SS.EXTRAS_ITERATION)
    assert set(seen) == {"omega", "confinement", "xsph", "rho", "normal", "tension"}

    # the same reference on the velocity BEFORE the friction pass must not fit
    off = kept["off"]
    fr = off.collider_friction_reaction()
    print(f"{name}: the friction pass slid {fr['hits']} of {fr['particles']} particles in contact")
    assert fr["hits"] >= 1
    p0 = X.params(pkg, name, iteration=SS.EXTRAS_ITERATION)
    early = X.run(pkg, name, fp64, fast, stop_after_sort=True, solids=rubbed_beside_a_wall, iteration=SS.EXTRAS_ITERATION)
    cells = key_cells(early.keys())
    unrubbed = pkg.Solver(h=X.H, fp64=fp64, flags=pkg.FLAG_FAST_MATH if fast else 0).upload(**sc)
    rubbed_beside_a_wall(unrubbed, name, fp64)
    warm = ER.SCENES[name][1]
    if warm:
        unrubbed.steps(p0, warm)
    unrubbed.set_collider_friction(None).step(p0)             # (the reaction stays on: the same step without its pass)
    a, b = off.download(), unrubbed.download()
    assert a["pos"].tobytes() == b["pos"].tobytes() and off.pstar().tobytes() == unrubbed.pstar().tobytes()
    assert a["vel"].tobytes() != b["vel"].tobytes()
    obstacle = a["type"] == 1
    h = ER.kernel_inputs(dtype, X.H, p0.dt)[0]
    P = ER.Pairs(off.pstar()[:, :3].astype(np.float64), h, dtype, cells)
    value, bar, _ = ER.xsph(P, b["vel"].astype(np.float64), obstacle)
    extra = ER.fast_allowance(value) if fast else 0.0
    ratio, err = ER.worst(kept["dv"], value, bar, ~obstacle, extra)
    print(f"{name}: against XSPH of the velocity before friction: worst error / bar {ratio:.3g}")
    assert ratio > 1.0, ratio


# ---- 2. launch paths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", ["obstacles_moving", "edges65"])
def test_every_path_gives_the_default_paths_bytes_beside_the_solids(pkg, name, fp64, fast):
    paths = X.PATHS if name == "obstacles_moving" else [dict(gather=0), dict(list_max=12), dict(list_max=32)]
    X.check_paths(pkg, name, fp64, fast, paths, solids=rubbed_beside_a_wall, more=solid_records, iteration=SS.EXTRAS_ITERATION)


# ---- 3. sequencing -----------------------------------------------------------------------------------------------------------------
def all_passes(pkg):
    p = pkg.default_params(4, 1000.0)
    p.vorticity = p.xsph = 1
    return p


def floating(pkg, fp64, fast, path=None):
    """configuration (d) — body, friction, scenery, body contact — on the scene of tests/test_solids_scene_gpu.py, and surface tension"""
    sc = S.cubes_with_obstacle(pkg, fp64)
    return solids(pkg, sc, fp64, fast, "body", path=path, reserve=0).set_surface_tension(ER.GAMMA, ER.BETA)


def sequenced(s):
    out = snapshot(s, "body")
    out["omega"], out["surface_state"] = s.omega().tobytes(), s.surface_state().tobytes()
    return out


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_graphed_batched_and_staged_steps_give_the_eager_bytes(pkg, fp64, fast):
    p = all_passes(pkg)
    eager = floating(pkg, fp64, fast)
    plain = floating(pkg, fp64, fast)
    q = pkg.default_params(4, 1000.0)
    plain.set_surface_tension(0.0, 0.0)
    for _ in range(4):
        eager.step(p)
        plain.step(q)
    want = sequenced(eager)
    assert want["vel"] != snapshot(plain, "body")["vel"]     # (the passes did something)
    assert eager.collider_friction_reaction()["hits"] > 0 and eager.collider_body_contact_state()["passes"] == 4
    graphed = floating(pkg, fp64, fast, dict(graph=1)).steps(p, 4)
    stats = graphed.graph_stats()
    print(f"graph stats {stats}")
    assert not differing(sequenced(graphed), want), differing(sequenced(graphed), want)
    assert stats[0] > 0 and stats[1] > 0 and stats[2], stats
    batched = floating(pkg, fp64, fast, dict(graph=0)).steps(p, 4)
    assert not differing(sequenced(batched), want), differing(sequenced(batched), want)
    staged = floating(pkg, fp64, fast)
    for _ in range(4):
        staged_step(staged, p, lambda: staged.stage("body", p))
    assert not differing(sequenced(staged), want), differing(sequenced(staged), want)
