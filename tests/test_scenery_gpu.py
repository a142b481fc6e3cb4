"""Scenery on the device (pbf_set_scenery / pbf_set_scenery_mesh / pbf_scenery_sample, include/pbf_hip.h): one static lattice in
the world frame beside the collider, projected after it.

  1. the window: pbf_scenery_sample equals tests/collider_ref.py bit for bit; a posed collider's own window is not disturbed;
  2. scenery alone is the static collider with the same lattice: eager, pbf_steps and graphs;
  3. delta-p with a posed collider and scenery = tests/scenery_ref.project_both applied to delta-p with neither, bit for bit,
     positions and reaction records, under every pose of collider_pose_ref.POSES and with no pose set;
  4. a scenery nothing touches changes nothing but the mode: state, records, wrench, body state, friction sums;
  5. every path that can run delta-p gives the default path's bytes (coop 2 / 4 / 8 within test_hip_parity's tolerance);
  6. a replayed hipGraph gives the eager bytes across a replaced scenery; a pose update per step recaptures nothing;
  7. the reaction is on whenever both lattices are installed;
  8. it holds the fluid: a block falls onto the tilted plane as scenery past a posed ball;
  9. a body in scenery: the tank's ball in a bowl;
 10. refusals leave the scenery, the collider and the state alone;
 11. pbf_set_scenery_mesh installs the lattice of pbf_sdf_from_mesh;
 12. the C++ shim and the CLI.

The CPU side of the restatement: tests/test_scenery_cpu.py.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import collider_pose_ref as PR
import collider_ref as CR
import mesh_soups as SP
import mesh_shapes as MS
import scenery_ref as SR
from test_collider_body_gpu import BALL, DISPLACED, RADIUS, TANK_SIDE, TANK_TOP, body_bytes, stock_body, tank
from test_collider_friction_gpu import MU, V, W, friction_bytes
from test_collider_gpu import (BOX_LATTICE, ERR_INVALID, ERR_STATE, H, IDS, VARIANTS, assert_sample_equal, dt_of, plane_through,
                               set_lattice, solver, state_bytes)
from test_collider_pose_gpu import body_lattice_through, install, pose_at, wrench_bytes
from test_extras_paths_gpu import PATHS
from test_nversion_cpu import scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pbf-sph_amd", "benchmark")
SPACING = BOX_LATTICE["spacing"]


def set_scenery(s, phi64):
    """the float64 nodes of a lattice over the box (collider_ref.BLOCK_LATTICE) as scenery"""
    return s.set_scenery(phi64, BOX_LATTICE["origin"], SPACING, CR.MARGIN)


def inf_lattice():
    return np.full(BOX_LATTICE["dims"], np.inf)


def everything(s):
    out = state_bytes(s)
    out["push"] = s.collider_push().tobytes()
    out["wrench"] = wrench_bytes(s)
    return out


def differing(got, want):
    return [k for k in want if got[k] != want[k]]


# ---- 1. the window -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("dims", [(2, 2, 2), (3, 5, 4), (23, 19, 27)])
def test_scenery_sample_equals_the_restatement(pkg, dims, fp64, fast):
    dtype = dt_of(fp64)
    lat, fr, pts, names = CR.edge_case(dims, dtype, n_random=4000)
    origin, spacing = CR.EDGE_LATTICES[dims]
    s = solver(pkg, fp64, fast)
    s.set_scenery(lat.phi.astype(np.float64), origin, spacing, CR.MARGIN)
    p = pkg.default_params(4, 1000.0)
    p.scale = CR.EDGE_SCALE
    want = CR.sample(lat, fr, pts)
    assert 0.02 < want[2].mean() < 0.98 and np.isinf(want[0]).any()
    assert_sample_equal(s.scenery_sample(pts, p), want, dims)
    # a posed collider beside it: each window shows its own lattice, the collider's under its pose
    R, t = PR.GENERIC
    clat, cfr, cpts, _ = CR.edge_case((3, 5, 4), dtype, n_random=2000)
    corigin, cspacing = CR.EDGE_LATTICES[(3, 5, 4)]
    with np.errstate(all="ignore"):
        world = cpts @ R.T + t
    s.set_collider(clat.phi.astype(np.float64), corigin, cspacing, CR.MARGIN).set_collider_pose(R, t)
    assert_sample_equal(s.collider_sample(p, world), PR.sample(clat, cfr, PR.pose_of(R, t, dtype), world), (dims, "collider"))
    assert_sample_equal(s.scenery_sample(pts, p), want, (dims, "scenery, again"))
    s.close()


# ---- 2. scenery alone is the static collider ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", ["cloud", "obstacles"])
def test_scenery_alone_is_the_static_collider(pkg, name, fp64, fast):
    sc = scene(name)
    lat, phi64, _ = plane_through(sc, dt_of(fp64))
    p = pkg.default_params(4, 1000.0)
    free = state_bytes(solver(pkg, fp64, fast).upload(**sc).steps(p, 4))
    for what, path, batched in (("eager", None, False), ("steps", None, True), ("graph", dict(graph=1), True)):
        a = set_lattice(solver(pkg, fp64, fast, path).upload(**sc), lat, phi64, SPACING)
        b = set_scenery(solver(pkg, fp64, fast, path).upload(**sc), phi64)
        for s in (a, b):
            if batched:
                s.steps(p, 4)
            else:
                for _ in range(4):
                    s.step(p)
        assert not differing(state_bytes(b), state_bytes(a)), (what, differing(state_bytes(b), state_bytes(a)))
        assert state_bytes(a)["pos"] != free["pos"]           # (it acts on this scene)
        if what == "graph":
            assert b.graph_stats()[1] > 0 and b.graph_stats() == a.graph_stats(), (a.graph_stats(), b.graph_stats())


# ---- 3. the stage against the restatement ------------------------------------------------------------------------------------
def run_to_delta(pkg, sc, fp64, fast, case, pose64, sphi, warm, iteration, clear):
    """upload, `warm` steps with both solids on, then predict -> sort -> diffuse -> `iteration` x (lambda, delta) by stage
    call; clear: BOTH solids are cleared before the LAST delta.  -> (solver, the records before the last launch)"""
    s = set_scenery(install(solver(pkg, fp64, fast).upload(**sc), case, pose64), sphi)
    p = pkg.default_params(4, 1000.0)
    if warm:
        s.steps(p, warm)
    s.stage("predict", p).stage("sort", p).stage("diffuse", p)
    push = None
    for it in range(iteration):
        s.stage("lambda", p)
        if it == iteration - 1:
            push = s.collider_push()
            if clear:
                s.set_collider(None).set_scenery(None)
        s.stage("delta", p)
    return s, push


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("warm", [0, 3])
@pytest.mark.parametrize("name", ["cloud", "obstacles", "edges1", "edges65", "edges257"])
def test_delta_with_both_solids_is_the_restatement_of_delta_with_neither(pkg, name, warm, fp64, fast):
    """Jacobi, as test_collider_pose_gpu's: twin B (a collider under a pose, and scenery) must hold project_both of twin A's
    output (both solids cleared for this one launch); lambda, and obstacles, as A's; PBF_BUF_COLLIDER_PUSH the restated
    records, accumulated onto those B held before the launch (warm = 0: the first launch after the sort, onto zeros; warm =
    3: the second, onto the first launch's).  The collider is test_collider_pose_gpu's plane through the fluid, the scenery
    a second plane with another normal, so at the first launch after the upload some fluid is below both, some below one
    and some below neither: each class is required to be non-empty there (a single particle: it starts inside both).  After
    warm steps the fluid rests on the planes and the classes are printed; what test_collider_pose_gpu requires there is
    required here: cloud, obstacles and edges257 keep hitting."""
    dtype = dt_of(fp64)
    sc = scene(name)
    block = name in ("edges65", "edges257")
    slat, sphi = SR.scenery_plane_through(sc, dtype, 0.2 if block else 0.35)
    iteration = 1 if warm == 0 else 2
    for pose_name, pose64 in list(PR.POSES.items()) + [("none", None)]:
        case = body_lattice_through(sc, dtype, pose64 or PR.IDENTITY, 0.15 if block else 0.5)
        lat, _, _, fr = case
        poseN = PR.pose_of(*(pose64 or PR.IDENTITY), dtype)           # (no pose set: the record holds the identity)
        a, _ = run_to_delta(pkg, sc, fp64, fast, case, pose64, sphi, warm, iteration, clear=True)
        b, before = run_to_delta(pkg, sc, fp64, fast, case, pose64, sphi, warm, iteration, clear=False)
        da, db = a.download(), b.download()
        for k in da:
            assert da[k].tobytes() == db[k].tobytes(), (pose_name, k)
        pa, pb = a.pstar(), b.pstar()
        fluid = da["type"] == 0
        q = np.ascontiguousarray(pa[:, :3])
        want, hit_c, hit_s, rec = SR.project_both(lat, poseN, slat, fr, q, before)
        rec[~fluid] = before[~fluid]                          # (obstacles are never projected)
        both, one, none = (hit_c & hit_s)[fluid].sum(), (hit_c ^ hit_s)[fluid].sum(), (~hit_c & ~hit_s)[fluid].sum()
        print(f"{name} warm {warm} pose {pose_name}: both {both}, one {one}, neither {none}")
        if warm == 0:
            assert (both > 0 and one > 0 and none > 0) if fluid.sum() > 1 else both == 1, (both, one, none)
            assert not before.any()
        elif name in ("cloud", "obstacles", "edges257"):
            assert both + one > 0 and none > 0, (both, one, none)
        assert pb[fluid, :3].tobytes() == want[fluid].tobytes(), (pose_name, int((pb[fluid, :3] != want[fluid]).any(axis=1).sum()))
        assert pb[:, 3].tobytes() == pa[:, 3].tobytes()
        assert pb[~fluid].tobytes() == pa[~fluid].tobytes()
        got = b.collider_push()
        assert got.tobytes() == rec.tobytes(), (pose_name, int((got != rec).any(axis=1).sum()))
        assert not got[~fluid].any()
        for s in (a, b):
            s.close()


# ---- 4. an untouched scenery changes nothing but the mode ---------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("feature", ["reaction", "body", "friction"])
def test_an_untouched_scenery_changes_nothing_but_the_mode(pkg, feature, fp64, fast):
    sc = scene("obstacles")
    case = body_lattice_through(sc, dt_of(fp64), PR.GENERIC)
    p = pkg.default_params(4, 1000.0)

    def run(scenery):
        s = install(solver(pkg, fp64, fast).upload(**sc), case, PR.GENERIC, reaction=True)
        if feature == "body":
            s.set_collider_body(**stock_body().kwargs())
        if feature == "friction":
            s.set_collider_friction(MU, V, W)
        if scenery:
            set_scenery(s, inf_lattice())
        out = []
        for _ in range(4):                                    # every step's bytes, not only the last one's
            s.step(p)
            e = everything(s)
            if feature == "body":
                e["body"] = body_bytes(s)
            if feature == "friction":
                e["friction"] = friction_bytes(s)
            out.append(e)
        return out, s

    want, ref = run(False)
    got, s = run(True)
    assert ref.collider_reaction()["hits"] > 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert not differing(g, w), (k, differing(g, w))
    if feature != "reaction":
        return
    # the scenery set on a ctx whose records were off turned them on, and the state is the same
    t = install(solver(pkg, fp64, fast).upload(**sc), case, PR.GENERIC)
    set_scenery(t, inf_lattice()).steps(p, 4)
    assert t.collider_reaction()["step"] == 4
    assert not differing(state_bytes(t), {k: want[-1][k] for k in state_bytes(t)})


# ---- 5. every path ---------------------------------------------------------------------------------------------------------------
def run_both_steps(pkg, sc, fp64, fast, case, sphi, path=None, steps=4, batched=False):
    """steps x (a new pose, one step) with the scenery beside the collider"""
    s = set_scenery(install(solver(pkg, fp64, fast, path).upload(**sc), case), sphi)
    p = pkg.default_params(4, 1000.0)
    for k in range(steps):
        s.set_collider_pose(*pose_at(k))
        s.steps(p, 1) if batched else s.step(p)
    return s


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_every_path_gives_the_default_paths_bytes(pkg, fp64, fast):
    sc = scene("obstacles")
    case = body_lattice_through(sc, dt_of(fp64), pose_at(0))
    _, sphi = SR.scenery_plane_through(sc, dt_of(fp64))
    ref = run_both_steps(pkg, sc, fp64, fast, case, sphi)
    want = everything(ref)
    assert ref.collider_reaction()["hits"] > 0 and ref.collider_reaction()["step"] == 4
    alone = state_bytes(run_both_steps(pkg, sc, fp64, fast, case, inf_lattice()))
    assert alone["pos"] != want["pos"]                        # the scenery does act on this scene
    for path in PATHS + [dict(pipeline=1), dict(fuse_predict=0), dict(row_major=0, gather=0)]:
        got = everything(run_both_steps(pkg, sc, fp64, fast, case, sphi, path))
        assert not differing(got, want), (path, differing(got, want))
    for what, path in (("graph", dict(graph=1)), ("steps", {}), ("steps, fuse_predict = 0", dict(fuse_predict=0))):
        got = everything(run_both_steps(pkg, sc, fp64, fast, case, sphi, path, batched=True))
        assert not differing(got, want), (what, differing(got, want))


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("coop", [2, 4, 8])
def test_coop_within_the_parity_tolerance(pkg, coop, fp64):
    """coop changes the summation order: one step from a common state, <= 1e-3 world units (fp32) / 1e-9 (fp64), the bar of
    test_collider_pose_gpu.test_coop_within_the_parity_tolerance"""
    sc = scene("obstacles")
    case = body_lattice_through(sc, dt_of(fp64), pose_at(0))
    _, sphi = SR.scenery_plane_through(sc, dt_of(fp64))
    st = run_both_steps(pkg, sc, fp64, False, case, sphi, steps=3).download()
    outs = []
    for c in (0, coop):
        s = set_scenery(install(solver(pkg, fp64, False, dict(coop=c)).upload(**st), case, pose_at(3)), sphi)
        outs.append(s.step(pkg.default_params(4, 1000.0)).download())
    assert np.array_equal(outs[0]["id"], outs[1]["id"])
    d = np.linalg.norm(outs[0]["pos"].astype(np.float64) - outs[1]["pos"].astype(np.float64), axis=1)
    print(f"coop {coop} vs 0: largest distance {d.max():.3e} world units")
    assert d.max() <= (1e-9 if fp64 else 1e-3), d.max()


# ---- 6. graphs ---------------------------------------------------------------------------------------------------------------
def test_graph_replay_sees_a_replaced_scenery(pkg):
    sc = scene("cloud")
    case = body_lattice_through(sc, np.float32, pose_at(0))
    _, phi1 = SR.scenery_plane_through(sc, np.float32, 0.35)
    _, phi2 = SR.scenery_plane_through(sc, np.float32, 0.5, normal=(0.25, -0.9, -0.2))
    p = pkg.default_params(4, 1000.0)
    g = install(solver(pkg, False).set_option("graph", 1).upload(**sc), case, pose_at(0))
    e = install(solver(pkg, False).upload(**sc), case, pose_at(0))
    for phi in (phi1, phi2, None):                            # set, replace, clear: each moves the key
        for s in (g, e):
            s.set_scenery(None) if phi is None else set_scenery(s, phi)
        before = g.graph_stats()
        g.steps(p, 6)
        for _ in range(6):
            e.step(p)
        assert not differing(everything(g), everything(e)), differing(everything(g), everything(e))
        after = g.graph_stats()
        assert after[0] > before[0] and after[1] > before[1] and after[2], (before, after)      # recaptured, then replayed
    assert e.graph_stats()[1] == 0
    # the two planes do give different runs: a stale lattice would have shown
    x = set_scenery(install(solver(pkg, False).upload(**sc), case, pose_at(0)), phi1)
    for _ in range(12):
        x.step(p)
    x.set_scenery(None)
    for _ in range(6):
        x.step(p)
    assert state_bytes(x)["pos"] != state_bytes(e)["pos"]


def test_a_new_pose_per_step_beside_scenery_recaptures_nothing(pkg):
    sc = scene("cloud")
    case = body_lattice_through(sc, np.float32, pose_at(0))
    _, sphi = SR.scenery_plane_through(sc, np.float32)
    p = pkg.default_params(4, 1000.0)

    def run(graph, moving, steps=12):
        s = solver(pkg, False)
        if graph:
            s.set_option("graph", 1)
        set_scenery(install(s.upload(**sc), case, pose_at(0)), sphi)
        for k in range(steps):
            if moving:
                s.set_collider_pose(*pose_at(k))
            s.steps(p, 1)
        return s

    g, e, const = run(True, True), run(False, True), run(True, False)
    assert not differing(everything(g), everything(e))
    assert g.graph_stats()[0] == const.graph_stats()[0] > 0, (g.graph_stats(), const.graph_stats())
    assert g.graph_stats()[1] > 0 and g.graph_stats()[2], g.graph_stats()
    assert state_bytes(const)["pos"] != state_bytes(g)["pos"]  # a stale pose would have shown


# ---- 7. the reaction rule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["collider first", "scenery first", "mesh collider last"])
def test_the_reaction_is_on_whenever_both_are_installed(pkg, order):
    sc = scene("cloud")
    lat, phi64, _ = plane_through(sc, np.float32)
    _, sphi = SR.scenery_plane_through(sc, np.float32)
    p = pkg.default_params(4, 1000.0)
    s = solver(pkg, False).upload(**sc)
    L = s.L
    if order == "collider first":
        set_scenery(set_lattice(s, lat, phi64, SPACING), sphi)
    elif order == "scenery first":
        set_lattice(set_scenery(s, sphi), lat, phi64, SPACING)
    else:
        v, t = MS.icosphere(subdivisions=2, R=120.0, centre=(165.0, 835.0, 165.0))     # test_mesh_sdf_gpu's ball in the cloud
        set_scenery(s, sphi).set_collider_mesh(v, t, margin=CR.MARGIN, **BOX_LATTICE)
    s.step(p)
    w = s.collider_reaction()
    assert w["step"] == 1 and w["hits"] > 0
    assert L.pbf_set_collider_reaction(s.ctx, 0) == ERR_STATE and b"scenery" in L.pbf_last_error(s.ctx)
    s.step(p)
    assert s.collider_reaction()["step"] == 2                 # (the refusal changed nothing)
    # after either is cleared it may be turned off; clearing leaves it on
    if order == "scenery first":
        s.set_collider(None)
        from pbf_sph_amd import capi
        assert L.pbf_collider_reaction(s.ctx, C.byref(capi.ColliderWrench())) == ERR_STATE         # (on, but there is no collider to report on)
        s.step(p)
    else:
        s.set_scenery(None)
        s.step(p)
        assert s.collider_reaction()["step"] == 3
    assert L.pbf_set_collider_reaction(s.ctx, 0) == 0
    s.step(p)
    s.close()


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_scenery_set_and_cleared_is_scenery_never_set(pkg, fp64, fast):
    sc = scene("cloud")
    _, sphi = SR.scenery_plane_through(sc, dt_of(fp64))
    p = pkg.default_params(4, 1000.0)
    never = solver(pkg, fp64, fast).upload(**sc).steps(p, 8)
    s = set_scenery(solver(pkg, fp64, fast).upload(**sc), sphi).set_scenery(None).steps(p, 8)
    assert state_bytes(s) == state_bytes(never)
    assert s.L.pbf_collider_reaction(s.ctx, None) == ERR_INVALID and s.L.pbf_set_collider_reaction(s.ctx, 0) == 0


# ---- 8. it holds the fluid -----------------------------------------------------------------------------------------------------
SPHERE_R, SPHERE_C = 70.0, np.array([345.0, 320.0, 494.0])    # beside collider_ref.block_scene (x from 400): 15 into its side
SPHERE_LATTICE = dict(origin=(-100.0,) * 3, spacing=10.0, dims=(21, 21, 21))


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_block_falls_onto_the_scenery_past_a_posed_ball(pkg, fp64):
    """test_collider_gpu.test_block_falls_onto_the_tilted_plane with the plane as SCENERY, and a ball under a pose (its
    lattice about the body frame's origin, carried to SPHERE_C under the generic rotation) that reaches 15 world units into
    the side of the block's path.  The ball's surface stays more than 3 h scale = 150 world units off the plane (asserted),
    so no particle is near both: no wedge.  The plane's bar and precondition are that test's; the ball's bar is the bowl
    test's, one lattice spacing."""
    dtype = dt_of(fp64)
    sc = CR.block_scene()
    lat, _ = CR.plane_case(dtype, CR.BLOCK_PLANE_D, **BOX_LATTICE)
    fr = CR.frame(CR.SCALE, *CR.BOX, dtype)
    bar = CR.plane_bar_world(dtype)
    p = pkg.default_params(4, 1000.0)
    assert CR.plane_phi(CR.PLANE_N, CR.BLOCK_PLANE_D, SPHERE_C[None])[0] - SPHERE_R > 3 * H * CR.SCALE
    ball = pkg.sdf_lattice(pkg.sdf_sphere((0.0, 0.0, 0.0), SPHERE_R), SPHERE_LATTICE["origin"], SPHERE_LATTICE["spacing"], SPHERE_LATTICE["dims"])

    def depth(ps):                                            # how deep the deepest particle is in the ball, world units
        return float((SPHERE_R - np.linalg.norm(ps.astype(np.float64) * CR.SCALE - SPHERE_C, axis=1)).max())

    def run(collider, scenery):
        s = solver(pkg, fp64).upload(**sc)
        if collider:
            s.set_collider(ball, SPHERE_LATTICE["origin"], SPHERE_LATTICE["spacing"], CR.MARGIN).set_collider_pose(PR.GENERIC[0], SPHERE_C)
        if scenery:
            s.set_scenery(lat.phi.astype(np.float64), BOX_LATTICE["origin"], SPACING, CR.MARGIN)
        lowest, deepest, touched = np.inf, -np.inf, False
        for step in range(CR.BLOCK_STEPS):
            ps = s.step(p).pstar()[:, :3]
            phi = CR.plane_phi(CR.PLANE_N, CR.BLOCK_PLANE_D, ps.astype(np.float64) * CR.SCALE)
            if scenery:
                assert not CR.on_face(fr, ps).any(), step     # the precondition: the second clamp never acted
                assert phi.min() >= CR.MARGIN - bar, (step, phi.min() - CR.MARGIN, bar)
            lowest, deepest = min(lowest, phi.min() - CR.MARGIN), max(deepest, depth(ps))
            touched |= bool((phi < CR.MARGIN + 1.0).any())
        return s, lowest, deepest, touched, phi

    s, lowest, deepest, touched, _ = run(True, True)
    print(f"{np.dtype(dtype).name}: lowest phi - margin over the run {lowest:.3e} world units, bar {bar:.3e}; deepest in the ball {deepest:.2f}")
    assert touched and s.collider_reaction()["step"] == CR.BLOCK_STEPS
    assert deepest <= SPHERE_LATTICE["spacing"], deepest
    _, _, without_ball, _, _ = run(False, True)
    assert without_ball > SPHERE_LATTICE["spacing"], without_ball      # without the collider some are deeper
    _, _, _, _, phi = run(True, False)
    assert phi.min() < -H * CR.SCALE, phi.min()               # without the scenery: below the plane by more than a cell


# ---- 9. a body in scenery ------------------------------------------------------------------------------------------------------
BOWL_R, BOWL_SPACING = 560.0, 27.0                             # clips the tank's four floor corners by about 40 world units
BOWL = dict(origin=(-BOWL_SPACING,) * 3, spacing=BOWL_SPACING, dims=(29, 29, 29))


def test_a_floating_ball_in_a_bowl(pkg):
    """test_collider_body_gpu's tank (a block of fluid that fills the floor of its own box, settled for 40 steps) with a bowl
    as scenery and the ball dropped onto the fluid as the body: 60 steps through one pbf_steps call equal 60 eager steps in
    every byte, the bowl holds the fluid to test_block_falls_into_the_bowl's bar, the body was advanced 60 times"""
    p = pkg.default_params(4, TANK_SIDE)
    st = solver(pkg, False).upload(**tank()).steps(p, 40).download()
    centre = np.full(3, 0.5 * TANK_SIDE)
    bowl = pkg.sdf_lattice(lambda x: -pkg.sdf_sphere(centre, BOWL_R)(x), BOWL["origin"], BOWL["spacing"], BOWL["dims"])
    ballphi = pkg.sdf_lattice(pkg.sdf_sphere((0.0, 0.0, 0.0), RADIUS), BALL["origin"], BALL["spacing"], BALL["dims"])
    body = dict(mass=DISPLACED, inertia=(0.4 * DISPLACED * RADIUS ** 2,) * 3, rot=np.eye(3), gain=0.49, accel=(0.0, 4900.0, 0.0),
                centre=(351.0, TANK_TOP - RADIUS - 30.0, 351.0), velocity=(0.0, 300.0, 0.0), centre_min=(RADIUS,) * 3,
                centre_max=(TANK_SIDE - RADIUS,) * 3)

    def make():
        s = solver(pkg, False).upload(**st)
        s.set_scenery(bowl, BOWL["origin"], BOWL["spacing"], CR.MARGIN)
        s.set_collider(ballphi, BALL["origin"], BALL["spacing"], CR.MARGIN)
        return s.set_collider_body(**body)

    def all_bytes(s):
        e = everything(s)
        e["body"] = body_bytes(s)
        return e

    a, b = make().steps(p, 60), make()
    for _ in range(60):
        b.step(p)
    assert not differing(all_bytes(a), all_bytes(b)), differing(all_bytes(a), all_bytes(b))
    w = a.pstar()[:, :3].astype(np.float64) * float(p.scale)
    beyond = int((np.linalg.norm(w - centre, axis=1) > BOWL_R - CR.MARGIN + BOWL_SPACING).sum())
    start = st["pos"].astype(np.float64)
    print(f"particles beyond r - margin + spacing: {beyond} after 60 steps, {(np.linalg.norm(start - centre, axis=1) > BOWL_R - CR.MARGIN + BOWL_SPACING).sum()} at the start")
    assert beyond == 0
    body_state = a.collider_body_state()
    assert body_state["steps"] == 60 and body_state["rejected"] == 0 and np.isfinite(body_state["centre"]).all()


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_alone(pkg):
    from pbf_sph_amd import capi
    sc = scene("cloud")
    lat, phi64, _ = plane_through(sc, np.float32)
    slat, sphi = SR.scenery_plane_through(sc, np.float32)
    p = pkg.default_params(4, 1000.0)
    s = solver(pkg, False).upload(**sc)
    L = s.L
    pts = np.random.default_rng(2).random((500, 3)) * 1000.0
    X = pts.ctypes.data_as(C.c_void_p)
    assert L.pbf_scenery_sample(s.ctx, C.byref(p), len(pts), X, None, None, None) == ERR_STATE and b"no scenery" in L.pbf_last_error(s.ctx)
    assert L.pbf_scenery_sample(s.ctx, C.byref(p), 0, None, None, None, None) == 0
    set_scenery(set_lattice(s, lat, phi64, SPACING), sphi).steps(p, 2)
    before, ssample, csample = everything(s), s.scenery_sample(pts, p), s.collider_sample(p, pts)
    assert ssample["hit"].any() and not ssample["hit"].all()
    assert not all(ssample[k].tobytes() == csample[k].tobytes() for k in ssample)     # (two different lattices)

    good = slat.phi.copy()

    def sdf(dims=good.shape, origin=BOX_LATTICE["origin"], spacing=SPACING, margin=CR.MARGIN, phi=good):
        d = capi.ColliderSdf()
        d.dims[:], d.origin[:] = list(dims), list(origin)
        d.spacing, d.margin, d.phi = spacing, margin, None if phi is None else phi.ctypes.data
        return d

    nan_phi = good.copy()
    nan_phi[3, 4, 5] = np.nan
    bad = {"a dim < 2": sdf(dims=(1, 23, 23)), "2^31 nodes": sdf(dims=(2048, 1024, 1024)), "dim 0": sdf(dims=(23, 0, 23)),
           "origin nan": sdf(origin=(0.0, np.nan, 0.0)), "origin inf": sdf(origin=(np.inf, 0.0, 0.0)),
           "spacing 0": sdf(spacing=0.0), "spacing < 0": sdf(spacing=-1.0), "spacing nan": sdf(spacing=np.nan), "spacing inf": sdf(spacing=np.inf),
           "margin < 0": sdf(margin=-0.5), "margin nan": sdf(margin=np.nan), "margin inf": sdf(margin=np.inf),
           "phi NULL": sdf(phi=None), "NaN in phi": sdf(phi=nan_phi)}
    for what, d in bad.items():
        assert L.pbf_set_scenery(s.ctx, C.byref(d)) == ERR_INVALID, what
        assert L.pbf_last_error(s.ctx).startswith(b"pbf_set_scenery: "), (what, L.pbf_last_error(s.ctx))
        # the same refusal, in the same order, as the collider's
        scenery_text = L.pbf_last_error(s.ctx)[len(b"pbf_set_scenery: "):]
        assert L.pbf_set_collider(s.ctx, C.byref(d)) == ERR_INVALID and L.pbf_last_error(s.ctx) == b"pbf_set_collider: " + scenery_text, what
    q = pkg.default_params(4, 1000.0)
    q.scale = 0.0
    for what, args in {"NULL params": (None, len(pts), X), "NULL points": (C.byref(p), len(pts), None), "scale 0": (C.byref(q), len(pts), X),
                       "2^31 points": (C.byref(p), 2 ** 31, X)}.items():
        assert L.pbf_scenery_sample(s.ctx, args[0], args[1], args[2], None, None, None) == ERR_INVALID, what
    tetra = MS.shape("tetra")
    m, keep = capi.mesh_struct(tetra[0], tetra[1][:-1])       # an open mesh without the winding flag
    assert L.pbf_set_scenery_mesh(s.ctx, C.byref(m), C.byref(sdf(phi=None)), 0, None) == ERR_INVALID
    assert L.pbf_set_scenery_mesh(s.ctx, C.byref(m), C.byref(sdf(phi=None, margin=-1.0)), capi.MESH_SIGN_WINDING, None) == ERR_INVALID
    # everything refused: both solids, the records and the particles are what they were
    again_s, again_c = s.scenery_sample(pts, p), s.collider_sample(p, pts)
    assert all(again_s[k].tobytes() == ssample[k].tobytes() for k in ssample)
    assert all(again_c[k].tobytes() == csample[k].tobytes() for k in csample)
    assert everything(s) == before
    # infinities are legal nodes
    inf_phi = good.copy()
    inf_phi[:2] = np.inf
    assert L.pbf_set_scenery(s.ctx, C.byref(sdf(phi=inf_phi))) == 0
    only = np.zeros(len(pts), np.uint8)
    assert L.pbf_scenery_sample(s.ctx, C.byref(p), len(pts), X, None, None, only.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(only != 0, CR.sample(CR.Lattice(inf_phi, BOX_LATTICE["origin"], SPACING, CR.MARGIN, np.float32),
                                               CR.frame(CR.SCALE, *CR.BOX, np.float32), pts)[2])

    # slab mode: refused on a configured ctx; scenery set earlier makes delta-p and pbf_slab_step refuse
    t = set_scenery(solver(pkg, False).upload(**sc), sphi).step(p)
    kept, state = t.scenery_sample(pts, p), state_bytes(t)
    cut = capi.SlabCut(0, 12, 0, 0)
    assert L.pbf_slab_configure(t.ctx, C.byref(cut), 0, 0) == 0
    assert L.pbf_set_scenery(t.ctx, C.byref(sdf())) == ERR_STATE and b"slab" in L.pbf_last_error(t.ctx)
    assert L.pbf_set_scenery_mesh(t.ctx, C.byref(capi.mesh_struct(*tetra)[0]), C.byref(sdf(phi=None)), 0, None) == ERR_STATE
    assert L.pbf_slab_step(t.ctx, C.byref(p)) == ERR_STATE
    assert L.pbf_slab_steps(t.ctx, C.byref(p), 2) == ERR_STATE
    assert L.pbf_stage_delta(t.ctx, C.byref(p)) == ERR_STATE
    assert all(t.scenery_sample(pts, p)[k].tobytes() == kept[k].tobytes() for k in kept)       # still the one set before
    assert L.pbf_slab_configure(t.ctx, None, 0, 0) == 0
    assert state_bytes(t) == state
    assert L.pbf_set_scenery(t.ctx, None) == 0                                                  # clearing is always allowed
    assert L.pbf_scenery_sample(t.ctx, C.byref(p), len(pts), X, None, None, None) == ERR_STATE
    # an attached ctx refuses alike
    noop = capi.EXCHANGE_FN(lambda *a: 0)
    comm = C.c_void_p()
    assert L.pbf_comm_create_host_callback(noop, None, 1, 0, C.byref(comm)) == 0
    cuts = np.array([0, 1024], np.uint32)
    u = solver(pkg, False).reserve(8192).upload(**sc)
    assert L.pbf_slab_attach(u.ctx, comm, cuts.ctypes.data_as(C.c_void_p), 256, 256) == 0
    assert L.pbf_set_scenery(u.ctx, C.byref(sdf())) == ERR_STATE
    assert L.pbf_scenery_sample(u.ctx, C.byref(p), len(pts), X, None, None, None) == ERR_STATE
    u.close()
    L.pbf_comm_destroy(comm)
    s.close()                                                 # pbf_destroy with both set
    t.close()


# ---- 11. pbf_set_scenery_mesh ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name,winding", [("tetra", False), ("open1", True)])
def test_set_scenery_mesh_is_set_scenery_of_the_lattice(pkg, name, winding, fp64, fast):
    """a closed mesh (the tetrahedron, four triangles) and a soup under PBF_MESH_SIGN_WINDING (the icosphere with a face
    missing), on mesh_shapes' lattice A"""
    v, t = SP.mesh(name, "A")
    lat = MS.LATTICE_A
    p = pkg.default_params(4, 1000.0)
    lo, hi = np.asarray(lat["origin"]), np.asarray(lat["origin"]) + lat["spacing"] * (np.asarray(lat["dims"]) - 1)
    pts = lo - 20.0 + np.random.default_rng(3).random((4000, 3)) * (hi - lo + 40.0)
    a, b = solver(pkg, fp64, fast), solver(pkg, fp64, fast)
    phi, _ = a.sdf_from_mesh(v, t, lat["origin"], lat["spacing"], lat["dims"], winding=winding)
    assert (phi < 0).any() and (phi > 0).any()
    a.set_scenery(phi, lat["origin"], lat["spacing"], CR.MARGIN)
    stats = b.set_scenery_mesh(v, t, lat["origin"], lat["spacing"], lat["dims"], CR.MARGIN, winding=winding)
    assert stats["pairs_total"] == phi.size * len(t)
    sa, sb = a.scenery_sample(pts, p), b.scenery_sample(pts, p)
    assert sa["hit"].any() and not sa["hit"].all() and np.isinf(sa["phi"]).any()
    assert all(sa[k].tobytes() == sb[k].tobytes() for k in sa)
    assert b.L.pbf_collider_sample(b.ctx, C.byref(p), 1, pts.ctypes.data_as(C.c_void_p), None, None, None) == ERR_STATE     # (no collider came with it)


# ---- 12. the shim and the CLI ---------------------------------------------------------------------------------------------------
def test_shim(pkg):
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_scenery_shim"), "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("ok scenery_shim_") == 6, r.stdout


def test_cli_a_body_in_a_bowl(pkg, tmp_path):
    common = ["--scene", "cubes", "--particles", "2048", "--solver-iter", "4", "-n", "8", "-w", "0", "--resident", "--no-surface"]
    r = subprocess.run([BIN, *common, "--collider=sphere:300,250,300,80", "--collider-body=40", "--collider-body-report",
                        "--scenery=bowl:500,500,500,800,13.5,50", "-o", str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Scenery              : bowl, lattice 23 x 23 x 23, spacing 50, margin 13.5" in r.stdout, r.stdout
    assert "Collider             : sphere" in r.stdout
    lines = [json.loads(l) for l in r.stdout.split("\n") if l.startswith('{"frame"')]
    assert [l["frame"] for l in lines] == list(range(8)) and all("body" in l for l in lines)
    body = lines[-1]["body"]
    assert body["steps"] == 8 and body["rejected"] == 0 and np.isfinite(body["centre"]).all()
    # the scenery alone; refused with slabs; ignored without --resident
    r = subprocess.run([BIN, *common, "--scenery=plane:0,-1,0,-150,13.5,50", "-o", str(tmp_path / "o2")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "Scenery              : plane" in r.stdout and "Collider " not in r.stdout, r.stdout + r.stderr
    r = subprocess.run([BIN, *common, "--scenery=plane:0,-1,0,-150", "--slabs", "2", "-o", str(tmp_path / "o3")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0 and "single-device" in r.stderr
    r = subprocess.run([BIN, *[c for c in common if c != "--resident"], "-n", "1", "--scenery=plane:0,-1,0,-150", "-o", str(tmp_path / "o4")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--scenery takes effect with --resident: ignored" in r.stdout
