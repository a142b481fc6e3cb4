"""What tests/test_solids_scene_gpu.py and tests/test_solids_extras_gpu.py take for granted about their scenes, checked without a
device: the geometry of the moved inlet, the outlet and the two solids through the restated device function
(collider_ref.project, collider_pose_ref.project), the host arithmetic of the counts, and — for the velocity passes — that
every scene, with its solids, keeps the share of ambiguous walkers at or below extras_ref.AMBIGUOUS_CAP on a float64
all-pairs step that includes the projection (the step of tests/test_collider_cpu.py, from tests/nversion.py)."""
import numpy as np
import pytest

import collider_friction_ref as FR
import collider_pose_ref as PR
import collider_ref as CR
import extras_ref as ER
import nversion as NV
import scene_cases as S
import solids_scene_cases as SS
from test_collider_body_gpu import first_step_share
from test_collider_friction_gpu import MU, V, W
from test_collider_gpu import plane_through
from test_collider_pose_gpu import body_lattice_through
from test_nversion_cpu import scene

DTYPES = [np.float32, np.float64]
IDS = ["fp32", "fp64"]


def solver_frame(points, dtype, fr):
    return np.ascontiguousarray((np.asarray(points, np.float64).astype(dtype) / fr[0]).astype(dtype))


# ---- part A: the geometry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_moved_inlets_sheet_is_born_inside_the_margin_shell(pkg, dtype):
    """every particle of the sheet hits at its birth position (phi < margin) and lies less than one margin away from the
    solid's surface; part of the sheet is in the shell proper (0 <= phi); the other inlet stays where main_scene put it"""
    sc = S.cubes_with_obstacle(pkg, dtype == np.float64)
    sources, drains = SS.composed_scene(sc)
    lat, _, _, fr = body_lattice_through(sc, dtype, PR.GENERIC, SS.SHARE)
    pts = S.np_emit({k: v[:0] for k, v in sc.items()}, sources[:1], dtype)["pos"]
    assert len(pts) == 16
    phi, _, hit = PR.project(lat, fr, PR.pose_of(*PR.GENERIC, dtype), solver_frame(pts, dtype, fr))
    print(f"sheet phi {phi.min():.3f} .. {phi.max():.3f}, margin {CR.MARGIN}")
    assert hit.all() and (np.abs(phi) < CR.MARGIN).all() and (phi >= 0).any()
    assert sources[1] == S.main_scene(sc)[0][1] and drains[1] == S.main_scene(sc)[1][1]
    assert 0.1 <= first_step_share(sc, dtype, (lat, None, None, fr), PR.GENERIC) <= 0.9


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_outlet_lies_over_the_surface_the_collider_pushes_onto(pkg, dtype):
    """its centre is 10 world units beyond phi = margin, so its ball cuts a disc out of that surface; fluid starts below the
    disc (what the first projection lifts onto it), and no particle of the moved inlet's sheet is born inside it"""
    sc = S.cubes_with_obstacle(pkg, dtype == np.float64)
    sources, drains = SS.composed_scene(sc)
    centre, width = drains[0]
    lat, _, _, fr = body_lattice_through(sc, dtype, PR.GENERIC, SS.SHARE)
    pose = PR.pose_of(*PR.GENERIC, dtype)
    phi, _, _ = PR.project(lat, fr, pose, solver_frame([centre], dtype, fr))
    assert abs(float(phi[0]) - (CR.MARGIN + 10.0)) < 0.01 and width > 10.0
    w = SS.fluid_positions(sc)
    _, moved, hit = PR.project(lat, fr, pose, solver_frame(w, dtype, fr))
    landed = moved[hit].astype(np.float64) * float(fr[0])
    inside = np.linalg.norm(landed - np.array(centre), axis=1) < width
    print(f"{int(inside.sum())} particles of the start state are projected into the outlet")
    assert inside.sum() >= 3
    sheet = SS.sheet(sources[0])
    assert (np.linalg.norm(sheet - np.array(centre), axis=1) > width + 27.0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_scenery_pushes_some_fluid_too(pkg, dtype):
    sc = S.cubes_with_obstacle(pkg, dtype == np.float64)
    wall, _, _ = plane_through(sc, dtype, SS.WALL_SHARE, SS.WALL_N)
    fr = CR.frame(CR.SCALE, *CR.BOX, dtype)
    hit = CR.project(wall, fr, solver_frame(SS.fluid_positions(sc), dtype, fr))[2]
    assert 0.05 <= hit.mean() <= 0.2, hit.mean()
    # it is not the collider's plane again: the two normals are far from parallel
    assert abs(float(SS.unit(SS.WALL_N) @ SS.unit(CR.PLANE_N))) < 0.5


def test_the_counts_are_what_the_gpu_tests_say(pkg):
    """host arithmetic: 28 particles per frame; without a drain the count passes 2 048 in the third frame, so the drains may
    take up to 120 particles in six frames before no frame sees a third partial record; the capacity case holds two frames"""
    sc = S.cubes_with_obstacle(pkg)
    sources, _ = SS.composed_scene(sc)
    per = SS.emitted_per_frame(sources)
    n = len(sc["id"])
    assert (n, per) == (2000, 28) and per == len(S.np_emit(sc, sources, np.float32)["id"]) - n
    assert [SS.records(n + per * (k + 1)) for k in range(SS.FRAMES)] == [2, 3, 3, 3, 3, 3]
    assert n + per * SS.FRAMES - 2 * SS.TILE == 120
    reserve = n + 2 * per + 10
    assert n + 2 * per <= reserve < n + 3 * per and n + per * SS.FRAMES <= SS.RESERVE


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_shrinking_scene_starts_above_two_tiles_and_its_corner_drain_takes_the_difference(pkg, dtype):
    base = S.cubes_with_obstacle(pkg, dtype == np.float64)
    sc, drains = SS.shrinking_scene(base, dtype)
    n = len(sc["id"])
    assert n == 2060 and SS.records(n) == 3 and len(np.unique(sc["id"])) == n
    left = S.np_drain(sc, drains[:1], dtype)
    assert len(left["id"]) == 2000 and S.same(left, {k: np.asarray(v).astype(left[k].dtype) for k, v in base.items()})
    # with room for what one step moves them by: the extra particles stay 40 world units inside, the scene's 20 outside
    centre, width = drains[0]
    r = np.linalg.norm(sc["pos"].astype(np.float64) - np.array(centre), axis=1)
    assert r[2000:].max() < width - 40.0 and r[:2000].min() > width + 20.0
    assert SS.records(2000) == 2
    # neither solid reaches the extra particles: they are still there, and inside the drain, after the step without a scene
    lat, _, _, fr = body_lattice_through(base, dtype, PR.GENERIC, SS.SHARE)
    wall, _, _ = plane_through(base, dtype, SS.WALL_SHARE, SS.WALL_N)
    q = solver_frame(sc["pos"][2000:], dtype, fr)
    phi = PR.project(lat, fr, PR.pose_of(*PR.GENERIC, dtype), q)[0]
    far = CR.project(wall, fr, q)[0]
    assert phi.min() > CR.MARGIN + 50.0 and far.min() > CR.MARGIN + 50.0, (phi.min(), far.min())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_depletion_scene(dtype):
    """no obstacle; the plane passes through the block; the wide drain holds the whole box; the inlet's sheet hits at birth"""
    sc = SS.depletion_scene(dtype)
    assert not sc["type"].any() and len(sc["id"]) == 729
    case = body_lattice_through(sc, dtype, PR.GENERIC, SS.SHARE)
    assert 0.1 <= first_step_share(sc, dtype, case, PR.GENERIC) <= 0.9
    corners = np.array([[x, y, z] for x in (0.0, 1000.0) for y in (0.0, 1000.0) for z in (0.0, 1000.0)])
    assert np.linalg.norm(corners - 500.0, axis=1).max() < 2000.0
    source = SS.composed_scene(sc)[0][0]
    lat, _, _, fr = case
    pts = S.np_emit({k: v[:0] for k, v in sc.items()}, [source], dtype)["pos"]
    assert PR.project(lat, fr, PR.pose_of(*PR.GENERIC, dtype), solver_frame(pts, dtype, fr))[2].all()


# ---- part B: the ambiguous share on a float64 all-pairs step with the projection ------------------------------------------------
def all_pairs_step_beside_the_solids(name):
    """the scene's warm steps and the step under test under tests/nversion.py's stages (float64, all pairs, cells fixed at predict
    time), the collider and then the scenery applied after delta-p's clamp as DeltaOp::end does, the friction restatement after
    finalise -> (pStar, velocity, mass, obstacle, predict-time cells, particles that slid) of the last step"""
    sc = scene(name)
    _, warm, force = ER.SCENES[name]
    iteration, N = SS.EXTRAS_ITERATION, np.float64
    lat, _, _, fr = body_lattice_through(sc, N, PR.GENERIC, SS.EXTRAS_SHARE[name])
    wall, _, _ = plane_through(sc, N, SS.WALL_SHARE, SS.WALL_N)
    pose = PR.pose_of(*PR.GENERIC, N)
    pos, vel, mass = sc["pos"].astype(N), sc["vel"].astype(N), sc["mass"].astype(N)
    obstacle = sc["type"] == 1
    h, dt, lo, hi = 0.1, float(np.float32(0.0083) * np.float32(1.5)), [0.0] * 3, [1000.0] * 3
    for _ in range(warm + 1):
        v, ps = NV.predict(pos, vel, mass, dt, CR.SCALE, force)
        v[obstacle], ps[obstacle] = vel[obstacle], pos[obstacle] / CR.SCALE
        cells = NV.predict_cells(ps, h, CR.SCALE, lo)
        rec = None
        for _ in range(iteration):
            lam, _ = NV.lambdas(ps, mass, h, obstacle, cells)
            ps, _ = NV.delta(ps, lam, h, CR.SCALE, lo, hi, obstacle, cells)
            _, q, hit = PR.project(lat, fr, pose, ps)
            hit &= ~obstacle
            q = np.where(hit[:, None], q, ps)
            rec = PR.react(fr, pose, ps, q, hit, rec)
            _, q2, hit2 = CR.project(wall, fr, q)
            ps = np.where((hit2 & ~obstacle)[:, None], q2, q)
        new_pos, new_vel = NV.finalise(ps, pos, v, dt, CR.SCALE)
        new_pos[obstacle], new_vel[obstacle] = pos[obstacle], vel[obstacle]
        A = np.zeros((len(pos), 4), N) if rec is None else np.ascontiguousarray(rec[:, :4])
        res = FR.friction(N, N(CR.SCALE), N(dt), MU, V, W, pose[1], new_vel, new_pos, A)
        pos, vel = new_pos, res["vel"]
    return ps, vel, mass, obstacle, cells, res["slide"]


@pytest.mark.parametrize("name", list(SS.EXTRAS_SHARE))
def test_every_part_b_scene_keeps_the_ambiguous_share_under_the_cap(name):
    ps, vel, mass, obstacle, cells, slide = all_pairs_step_beside_the_solids(name)
    fluid = ~obstacle
    assert np.isfinite(ps).all() and np.isfinite(vel).all()
    assert slide.any()
    h, dt, gamma, beta = ER.kernel_inputs(np.float32, 0.1, float(np.float32(0.0083) * np.float32(1.5)), ER.GAMMA, ER.BETA)
    P = ER.Pairs(ps, h, np.float32, cells)
    w, _, amb_w = ER.vorticity(P, vel, obstacle)
    _, _, amb_c = ER.confinement(P, vel, w, dt, obstacle)
    _, amb_s = ER.surface(P, vel, mass, dt, gamma, beta, obstacle)
    for record, amb in (("omega", amb_w), ("confinement", amb_c), ("surface", amb_s)):
        share = amb.sum() / max(int(fluid.sum()), 1)
        print(f"{name} {record}: ambiguous {100 * share:.2f} %")
        assert share <= ER.AMBIGUOUS_CAP, (name, record, share)
