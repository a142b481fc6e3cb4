"""Moving colliders on the device (pbf_set_collider_pose, pbf_set_collider_reaction / pbf_collider_reaction, include/pbf_hip.h):

  1. the device function alone, through pbf_collider_sample under a pose, equals tests/collider_pose_ref.py bit for bit;
  2. delta-p with the posed collider = the restatement applied to delta-p without it, bit for bit, at iteration 1 and 2, and
     PBF_BUF_COLLIDER_PUSH = the restated records (one update, then two accumulated);
  3. every path that can run delta-p gives the default path's state, record and wrench bytes with a pose that changes every
     step (coop = 2 within test_hip_parity's tolerance);
  4. a new pose per step recaptures nothing and gives the eager bytes; none -> posed -> none returns to the static bytes;
  5. the identity pose and the reaction without a pose equal the static collider; a pose on an untouched lattice changes nothing;
  6. a moving plane pushes a block: nothing is left on the solid side and the impulse points along the world normal;
  7. the sum against a closed form (n = 1) and against a float64 sum of the records at n = 65, 1025 and 262 145;
  8. refusals leave the pose, the records and the state alone;
  9. the C++ shim's frames and `benchmark --collider-motion --collider-reaction` equal the same frames over the C ABI.

The CPU side of the restatement and of scene 6's preconditions: tests/test_collider_pose_cpu.py.
"""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import collider_pose_ref as PR
import collider_ref as CR
from test_collider_gpu import (BOX_LATTICE, ERR_INVALID, ERR_STATE, H, IDS, VARIANTS, assert_sample_equal, dt_of, plane_through,
                               set_lattice, solver, state_bytes)
from test_extras_paths_gpu import PATHS
from test_nversion_cpu import scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pbf-sph_amd", "benchmark")


def body_lattice_through(sc, dtype, pose64, share=0.5, normal=CR.PLANE_N):
    """the world plane that `share` of the scene's fluid starts below (as test_collider_gpu.plane_through), as a lattice in the
    body frame of pose64 that covers the whole box -> (Lattice, float64 nodes, origin, frame)"""
    w = sc["pos"][sc["type"] == 0].astype(np.float64)
    d = float(np.quantile(CR.plane_phi(normal, 0.0, w), share)) - CR.MARGIN
    if len(w) == 1:
        d += 30.0                                             # a single particle starts inside the solid
    return PR.body_plane_case(pose64, dtype, normal, d)


def install(s, case, pose64=None, reaction=False):
    lat, phi64, origin, _ = case
    s.set_collider(phi64, origin, PR.BODY_SPACING, CR.MARGIN)
    if reaction:
        s.set_collider_reaction(True)
    if pose64 is not None:
        s.set_collider_pose(*pose64)
    return s


def wrench_bytes(s):
    return bytes(s.collider_reaction(raw=True))


# ---- 1. the device function alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("pose", list(PR.POSES))
@pytest.mark.parametrize("dims", [(2, 2, 2), (3, 5, 4), (23, 19, 27)])
def test_device_function_under_a_pose_equals_the_restatement(pkg, dims, pose, fp64, fast):
    """the lattices and edge points of the static test, carried into the world frame by the pose (exactly, for the identity
    and the quarter turn: the edge points stay ON the edges), and 4000 random points"""
    dtype = dt_of(fp64)
    lat, fr, pts, names = CR.edge_case(dims, dtype, n_random=4000)
    origin, spacing = CR.EDGE_LATTICES[dims]
    R, t = PR.POSES[pose]
    with np.errstate(all="ignore"):
        world = pts @ R.T + t
    world[~np.isfinite(pts).all(axis=1)] = pts[~np.isfinite(pts).all(axis=1)]
    poseN = PR.pose_of(R, t, dtype)
    s = solver(pkg, fp64, fast)
    s.set_collider(lat.phi.astype(np.float64), origin, spacing, CR.MARGIN).set_collider_pose(R, t)
    p = pkg.default_params(4, 1000.0)
    p.scale = CR.EDGE_SCALE
    want = PR.sample(lat, fr, poseN, world)
    assert 0.02 < want[2].mean() < 0.98 and np.isinf(want[0]).any()
    if pose != "generic":                                     # exact: the static function's answers on the body points
        static = CR.sample(lat, fr, pts)
        assert np.array_equal(static[2], want[2]) and np.array_equal(static[0], want[0])
    assert_sample_equal(s.collider_sample(p, world), want, (dims, pose))
    s.set_collider_pose(None)                                 # and back: the static function at the same points
    assert_sample_equal(s.collider_sample(p, world), CR.sample(lat, fr, world), (dims, pose, "cleared"))


# ---- 2. integration, bit for bit, every iteration ---------------------------------------------------------------------------
def run_to_delta(pkg, sc, fp64, fast, case, pose64, warm, iteration, clear):
    """upload, `warm` steps with the posed collider and the reaction on, then predict -> sort -> diffuse -> `iteration` x
    (lambda, delta) by stage call; clear: the collider is cleared before the LAST delta"""
    s = install(solver(pkg, fp64, fast).upload(**sc), case, pose64, reaction=True)
    p = pkg.default_params(4, 1000.0)
    if warm:
        s.steps(p, warm)
    s.stage("predict", p).stage("sort", p).stage("diffuse", p)
    push = None
    for it in range(iteration):
        s.stage("lambda", p)
        if it == iteration - 1:
            push = s.collider_push()                          # the records before the last launch
            if clear:
                s.set_collider(None)
        s.stage("delta", p)
    return s, push


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("warm", [0, 3])
@pytest.mark.parametrize("name", ["cloud", "obstacles", "edges1", "edges65", "edges257"])
def test_delta_with_posed_collider_is_the_restatement_of_delta_without(pkg, name, warm, fp64, fast):
    """Jacobi, as test_collider_gpu's: twin B (posed collider on) must hold the restatement of twin A's output (collider
    cleared for this one launch); lambda, and obstacles, as A's.  The records after iteration 1 are the single update; after
    iteration 2 the accumulation of two, the first being the records B held before its last launch (themselves checked as
    iteration 1's).  The hit-share conditions are the static test's, asserted on the restatement."""
    dtype = dt_of(fp64)
    sc = scene(name)
    pose64 = PR.GENERIC
    case = body_lattice_through(sc, dtype, pose64, 0.15 if name in ("edges65", "edges257") else 0.5)
    lat, _, _, fr = case
    poseN = PR.pose_of(*pose64, dtype)
    for iteration in (1, 2):
        a, _ = run_to_delta(pkg, sc, fp64, fast, case, pose64, warm, iteration, clear=True)
        b, before = run_to_delta(pkg, sc, fp64, fast, case, pose64, warm, iteration, clear=False)
        da, db = a.download(), b.download()
        for k in da:
            assert da[k].tobytes() == db[k].tobytes(), (iteration, k)
        pa, pb = a.pstar(), b.pstar()
        fluid = da["type"] == 0
        q = np.ascontiguousarray(pa[:, :3])
        _, want, hit = PR.project(lat, fr, poseN, q)
        share = hit[fluid].mean()
        print(f"{name} warm {warm} iteration {iteration}: {100 * share:.1f} % of the fluid hits")
        if warm == 0 and iteration == 1:
            assert (0.1 <= share <= 0.9) if fluid.sum() > 1 else share == 1.0, share
        elif name in ("cloud", "obstacles", "edges257"):
            assert 0.0 < share < 1.0, share
        assert pb[fluid, :3].tobytes() == want[fluid].tobytes(), (iteration, int((pb[fluid, :3] != want[fluid]).any(axis=1).sum()))
        assert pb[:, 3].tobytes() == pa[:, 3].tobytes()
        assert pb[~fluid].tobytes() == pa[~fluid].tobytes()
        # the records: obstacles never hit; the fluid's follow the contract from the records held before this launch
        if iteration == 1:
            assert not before.any()
        else:
            assert before.tobytes() == first.tobytes()
        rec = PR.react(fr, poseN, q, want, hit & fluid, before)
        got = b.collider_push()
        assert got.tobytes() == rec.tobytes(), (iteration, int((got != rec).any(axis=1).sum()))
        assert not got[~fluid].any()
        if iteration == 1:
            first = got


# ---- 3. every path gives the default path's bytes ---------------------------------------------------------------------------
def pose_at(k):
    """the pose of step k: the generic rotation turned a little further and carried along"""
    return PR.rotation((0.3, -0.5, 0.8), 0.7 + 0.05 * k), PR.GENERIC[1] + np.array([6.0, -4.0, 3.0]) * k


def run_posed_steps(pkg, sc, fp64, fast, case, path=None, steps=4, batched=False, reaction=True):
    """steps x (a new pose, one step); batched: the step goes through pbf_steps (graphs where the path asks for them)"""
    s = install(solver(pkg, fp64, fast, path).upload(**sc), case, None, reaction)
    p = pkg.default_params(4, 1000.0)
    for k in range(steps):
        s.set_collider_pose(*pose_at(k))
        s.steps(p, 1) if batched else s.step(p)
    return s


def everything(s):
    out = state_bytes(s)
    out["push"] = s.collider_push().tobytes()
    out["wrench"] = wrench_bytes(s)
    return out


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_every_path_gives_the_default_paths_bytes(pkg, fp64, fast):
    sc = scene("obstacles")
    case = body_lattice_through(sc, dt_of(fp64), pose_at(0))
    ref = run_posed_steps(pkg, sc, fp64, fast, case)
    want = everything(ref)
    w = ref.collider_reaction()
    assert w["hits"] > 0 and w["step"] == 4 and np.abs(w["impulse"]).max() > 0
    fixed = state_bytes(install(solver(pkg, fp64, fast).upload(**sc), case, pose_at(0)).steps(pkg.default_params(4, 1000.0), 4))
    assert fixed["pos"] != want["pos"]                        # the motion does act on this scene
    for path in PATHS + [dict(pipeline=1), dict(fuse_predict=0), dict(row_major=0, gather=0)]:
        got = everything(run_posed_steps(pkg, sc, fp64, fast, case, path))
        assert not [k for k in want if got[k] != want[k]], (path, [k for k in want if got[k] != want[k]])
    for what, path in (("graph", dict(graph=1)), ("steps", {}), ("steps, fuse_predict = 0", dict(fuse_predict=0))):
        got = everything(run_posed_steps(pkg, sc, fp64, fast, case, path, batched=True))
        assert not [k for k in want if got[k] != want[k]], (what, [k for k in want if got[k] != want[k]])
    # one pbf_steps(4) call under a constant pose = four pbf_step calls
    p = pkg.default_params(4, 1000.0)
    one = everything(install(solver(pkg, fp64, fast).upload(**sc), case, pose_at(0), True).steps(p, 4))
    four = install(solver(pkg, fp64, fast).upload(**sc), case, pose_at(0), True)
    for _ in range(4):
        four.step(p)
    assert one == everything(four)
    # and without the records: the posed kernels give the same state
    plain = state_bytes(run_posed_steps(pkg, sc, fp64, fast, case, reaction=False))
    assert not [k for k in plain if plain[k] != want[k]]


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_coop_within_the_parity_tolerance(pkg, fp64):
    """coop = 2 changes the summation order: one step from a common state, <= 1e-3 world units (fp32) / 1e-9 (fp64) as
    test_hip_parity.test_wave_cooperative_reader_within_tolerance holds it without a collider"""
    sc = scene("obstacles")
    case = body_lattice_through(sc, dt_of(fp64), pose_at(0))
    st = run_posed_steps(pkg, sc, fp64, False, case, steps=3).download()
    outs = []
    for coop in (0, 2):
        s = install(solver(pkg, fp64, False, dict(coop=coop)).upload(**st), case, pose_at(3), True)
        outs.append(s.step(pkg.default_params(4, 1000.0)).download())
    assert np.array_equal(outs[0]["id"], outs[1]["id"])
    d = np.linalg.norm(outs[0]["pos"].astype(np.float64) - outs[1]["pos"].astype(np.float64), axis=1)
    print(f"coop 2 vs 0: largest distance {d.max():.3e} world units")
    assert d.max() <= (1e-9 if fp64 else 1e-3), d.max()


# ---- 4. graphs ---------------------------------------------------------------------------------------------------------
def test_a_new_pose_per_step_recaptures_nothing(pkg):
    sc = scene("cloud")
    case = body_lattice_through(sc, np.float32, pose_at(0))
    p = pkg.default_params(4, 1000.0)

    def run(graph, moving, steps=12):
        s = solver(pkg, False)
        if graph:
            s.set_option("graph", 1)
        install(s.upload(**sc), case, pose_at(0), True)
        for k in range(steps):
            if moving:
                s.set_collider_pose(*pose_at(k))
            s.steps(p, 1)
        return s

    g, e, const = run(True, True), run(False, True), run(True, False)
    assert everything(g) == everything(e)
    assert g.graph_stats()[0] == const.graph_stats()[0] > 0, (g.graph_stats(), const.graph_stats())
    assert g.graph_stats()[1] > 0 and g.graph_stats()[2], g.graph_stats()
    assert e.graph_stats()[1] == 0
    assert state_bytes(const)["pos"] != state_bytes(g)["pos"]  # a stale pose would have shown


@pytest.mark.parametrize("graph", [0, 1], ids=["eager", "graph"])
def test_pose_none_posed_none_returns_to_the_static_bytes(pkg, graph):
    sc = scene("cloud")
    lat, phi64, _ = plane_through(sc, np.float32)
    p = pkg.default_params(4, 1000.0)
    a = solver(pkg, False, dict(graph=graph)).upload(**sc)
    set_lattice(a, lat, phi64, BOX_LATTICE["spacing"]).steps(p, 3)
    b = solver(pkg, False, dict(graph=graph)).upload(**a.download())
    set_lattice(b, lat, phi64, BOX_LATTICE["spacing"])
    b.set_collider_pose(PR.rotation((0, 0, 1), 0.2), (40.0, 0.0, 0.0)).steps(p, 3)
    posed = state_bytes(b)
    b.upload(**a.download()).set_collider_pose(None).steps(p, 3)
    c = solver(pkg, False, dict(graph=graph)).upload(**a.download())
    set_lattice(c, lat, phi64, BOX_LATTICE["spacing"]).steps(p, 3)
    assert state_bytes(b) == state_bytes(c) and posed != state_bytes(c)
    # a new lattice resets the pose
    b.set_collider_pose(PR.rotation((0, 0, 1), 0.2), (40.0, 0.0, 0.0))
    set_lattice(b, lat, phi64, BOX_LATTICE["spacing"]).upload(**a.download()).steps(p, 3)
    assert state_bytes(b) == state_bytes(c)


# ---- 5. off means off ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", ["cloud", "obstacles"])
def test_identity_pose_and_reaction_without_a_pose_equal_the_static_collider(pkg, name, fp64, fast):
    sc = scene(name)
    lat, phi64, _ = plane_through(sc, dt_of(fp64))
    p = pkg.default_params(4, 1000.0)

    def run(pose=False, reaction=False):
        s = solver(pkg, fp64, fast).upload(**sc)
        set_lattice(s, lat, phi64, BOX_LATTICE["spacing"])
        if reaction:
            s.set_collider_reaction(True)
        if pose:
            s.set_collider_pose(*PR.IDENTITY)
        return s.steps(p, 6)

    static = run()
    want, ps = static.download(), static.pstar()
    free = state_bytes(solver(pkg, fp64, fast).upload(**sc).steps(p, 6))
    assert free["pos"] != want["pos"].tobytes()               # (the collider acts)
    for kw in (dict(pose=True), dict(reaction=True), dict(pose=True, reaction=True)):
        s = run(**kw)
        got = s.download()
        for k in want:                                        # ==, not bytes: a zero may change its sign
            assert np.array_equal(got[k], want[k]), (kw, k)
        assert np.array_equal(s.pstar(), ps), kw
        if kw.get("reaction"):
            assert s.collider_reaction()["step"] == 6


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_a_pose_on_an_untouched_lattice_changes_nothing(pkg, fp64, fast):
    sc = scene("cloud")
    p = pkg.default_params(4, 1000.0)
    never = solver(pkg, fp64, fast).upload(**sc).steps(p, 8)
    # the plane of test_collider_gpu 1000 world units below the floor, seen from a body frame: phi >= 950 in the whole box
    case = PR.body_plane_case(PR.GENERIC, dt_of(fp64), (0.0, -1.0, 0.0), -2000.0)
    corners = np.array([[x, y, z] for x in (0.0, 1000.0) for y in (0.0, 1000.0) for z in (0.0, 1000.0)])
    assert CR.plane_phi((0.0, -1.0, 0.0), -2000.0, corners).min() >= 950.0
    s = install(solver(pkg, fp64, fast).upload(**sc), case, PR.GENERIC, True).steps(p, 8)
    assert state_bytes(s) == state_bytes(never)
    w = s.collider_reaction()
    assert w["hits"] == 0 and w["particles"] == 0 and w["step"] == 8 and not s.collider_push().any()
    assert not np.abs(w["impulse"]).any() and not np.abs(w["abs_angular"]).any()


# ---- 6. it pushes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_a_moving_plane_pushes_the_block(pkg, fp64):
    """tests/test_collider_pose_cpu.py checks this scene's preconditions on a float64 all-pairs step: no particle reaches a
    box face, and the plane does reach the block"""
    dtype = dt_of(fp64)
    sc = CR.block_scene()
    lat, phi64, origin, fr = PR.push_case(dtype)
    bar = PR.pose_bar_world(dtype)
    p = pkg.default_params(4, 1000.0)
    s = solver(pkg, fp64).upload(**sc)
    s.set_collider(phi64, origin, PR.BODY_SPACING, CR.MARGIN).set_collider_reaction(True)
    n_w = PR.PUSH_R @ np.array([1.0, 0.0, 0.0])
    mass = float(sc["mass"][0])
    worst, pushed = np.inf, 0
    for step in range(PR.PUSH_STEPS):
        R, t = PR.push_pose(step)
        ps = s.set_collider_pose(R, t).step(p).pstar()[:, :3]
        assert not CR.on_face(fr, ps).any(), step             # the precondition: the second clamp never acted
        w = ps.astype(np.float64) * CR.SCALE
        seen = s.collider_sample(p, w)["phi"]                 # the posed function itself, at the stored positions
        inside = np.isfinite(seen)
        assert inside.all(), step                             # (the lattice covers the block all along)
        assert seen.min() >= CR.MARGIN - bar, (step, seen.min() - CR.MARGIN, bar)
        true = w @ n_w - PR.push_plane_d(step)                # and the closed form of the plane where it stands now
        assert true.min() >= CR.MARGIN - bar, (step, true.min() - CR.MARGIN, bar)
        worst = min(worst, true.min() - CR.MARGIN)
        wr = s.collider_reaction()
        assert wr["step"] == step + 1
        if wr["hits"]:
            pushed += 1
            P = wr["impulse"]
            along = float(P @ n_w)
            across = np.abs(P - along * n_w).max()
            # every hit's displacement is along the normal up to the roundings the CPU-validated bar bounds; the sum's own
            # rounding scales with abs_impulse
            tol = wr["hits"] * mass * bar + (wr["hits"] + 16) * 2.0 ** -53 * np.abs(wr["abs_impulse"]).max()
            assert along > 0 and across <= tol, (step, P, across, tol)
    print(f"{np.dtype(dtype).name}: lowest phi - margin over the run {worst:.3e} world units, bar {bar:.3e}; pushed in {pushed} steps")
    assert pushed >= PR.PUSH_STEPS // 2


# ---- 7. the sum -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_one_particle_against_the_closed_form(pkg, fp64):
    """a particle a known depth inside a plane: delta = (margin + depth) n, P = m delta, L = m (w' - t) x delta, in float64
    from the position delta-p would have stored without the collider.  Rounding of the contract: w' lands on phi = margin
    within the CPU-validated bar (normal part) and the displacement's other components carry the same roundings, so each
    component of delta is within 2 bars; L adds |r| <= 2600 times that and one rounding of each product"""
    dtype = dt_of(fp64)
    mass = 1.75
    sc = dict(id=np.zeros(1, np.uint64), type=np.zeros(1, np.uint8), mass=np.full(1, mass), pos=np.array([[510.0, 430.0, 470.0]]),
              vel=np.zeros((1, 3)), colour=np.full((1, 4), 0.5))
    R, t = PR.GENERIC
    n_w = np.asarray(CR.PLANE_N) / np.linalg.norm(CR.PLANE_N)
    d = float(n_w @ sc["pos"][0]) + 40.0                      # the particle starts 40 inside the solid
    case = PR.body_plane_case(PR.GENERIC, dtype, CR.PLANE_N, d)
    p = pkg.default_params(1, 1000.0)
    twins = []
    for clear in (True, False):
        s = install(solver(pkg, fp64).upload(**sc), case, PR.GENERIC, True)
        s.stage("predict", p).stage("sort", p).stage("diffuse", p).stage("lambda", p)
        if clear:
            s.set_collider(None)
        twins.append(s.stage("delta", p))
    w0 = twins[0].pstar()[0, :3].astype(np.float64) * CR.SCALE
    depth = -(float(n_w @ w0) - d)
    assert 30.0 < depth < 50.0
    delta = (CR.MARGIN + depth) * n_w
    wr = twins[1].collider_reaction()
    bar = PR.pose_bar_world(dtype)
    assert wr["hits"] == 1 and wr["particles"] == 1 and wr["step"] == 1
    assert np.abs(wr["impulse"] - mass * delta).max() <= mass * 2 * bar, (wr["impulse"], mass * delta)
    L = mass * np.cross(w0 + delta - t, delta)
    tol = mass * (2600.0 * 2 * bar + 4 * float(np.finfo(dtype).eps) * 2600.0 * np.abs(delta).max())
    assert np.abs(wr["angular"] - L).max() <= tol, (wr["angular"], L, tol)
    assert np.array_equal(wr["abs_impulse"], np.abs(wr["impulse"])) and np.array_equal(wr["abs_angular"], np.abs(wr["angular"]))


def dense_block(n):
    """n particles on a cubic grid 12 world units apart in mid-box, their mass scaled to the rest density"""
    k = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    pos = g * 12.0 + (500.0 - 6.0 * (k - 1))
    return dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.full(n, (12.0 / 27.0) ** 3), pos=pos,
                vel=np.zeros((n, 3)), colour=np.full((n, 4), 0.5))


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", [65, 1025, 262145])
def test_the_sum_equals_a_float64_sum_of_the_records(pkg, n, fp64):
    """every particle inside the solid, so every particle hits in both iterations: a second wave round (65), a second
    workgroup (1025) and the second 256-record round of the final fold (262 145 = 256 x 1024 + 1)"""
    dtype = dt_of(fp64)
    sc = dense_block(n)
    # body plane b_x = c with the solid on the -x side, far beyond the box on the fluid side: the whole box is inside the solid
    n_w = PR.GENERIC[0] @ np.array([1.0, 0.0, 0.0])
    case = PR.body_plane_case(PR.GENERIC, dtype, n_w, 5000.0, dims=(41, 41, 41))
    assert case[1].max() < 0
    p = pkg.default_params(2, 1000.0)
    outs = []
    for _ in range(2):
        s = install(solver(pkg, fp64).upload(**sc), case, PR.GENERIC, True).step(p)
        outs.append((wrench_bytes(s), s.collider_push().tobytes()))
    assert outs[0] == outs[1]                                 # bit-identical over two runs
    wr, rec, mass = s.collider_reaction(), s.collider_push().astype(np.float64), s.download()["mass"].astype(np.float64)
    assert np.isfinite(rec).all()
    assert wr["hits"] == 2 * n and wr["particles"] == n and wr["step"] == 1 and (rec[:, 3] == 2).all()
    for key, cols in (("impulse", slice(0, 3)), ("angular", slice(4, 7))):
        terms = mass[:, None] * rec[:, cols]
        tol = (n + 16) * 2.0 ** -53 * wr["abs_" + key]
        assert (np.abs(wr[key] - terms.sum(axis=0)) <= tol).all(), (key, wr[key], terms.sum(axis=0), tol)
        assert (np.abs(wr["abs_" + key] - np.abs(terms).sum(axis=0)) <= tol).all(), key
    # a further step in which nothing touches: the solid carried far away along its own normal
    s.set_collider_pose(PR.GENERIC[0], PR.GENERIC[1] + 1e5 * n_w).step(p)
    wr = s.collider_reaction()
    assert wr["step"] == 2 and wr["hits"] == 0 and wr["particles"] == 0 and not s.collider_push().any()
    assert not any(np.abs(wr[k]).any() for k in ("impulse", "angular", "abs_impulse", "abs_angular"))


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_alone(pkg):
    from pbf_sph_amd import capi
    sc = scene("cloud")
    case = body_lattice_through(sc, np.float32, PR.GENERIC)
    p = pkg.default_params(4, 1000.0)
    pts = np.random.default_rng(2).random((500, 3)) * 1000.0

    def pose(rot=PR.GENERIC[0], trans=PR.GENERIC[1]):
        d = capi.ColliderPose()
        d.rot[:], d.trans[:] = [float(v) for v in np.asarray(rot).reshape(9)], [float(v) for v in trans]
        return d

    s = solver(pkg, False).upload(**sc)
    L = s.L
    wr = capi.ColliderWrench()
    assert L.pbf_set_collider_pose(s.ctx, C.byref(pose())) == ERR_STATE and b"no collider" in L.pbf_last_error(s.ctx)
    assert L.pbf_set_collider_pose(s.ctx, None) == ERR_STATE
    assert L.pbf_collider_reaction(s.ctx, C.byref(wr)) == ERR_STATE and b"not enabled" in L.pbf_last_error(s.ctx)
    install(s, case, PR.GENERIC)
    assert L.pbf_collider_reaction(s.ctx, C.byref(wr)) == ERR_STATE
    s.set_collider_reaction(True)
    assert L.pbf_collider_reaction(s.ctx, C.byref(wr)) == ERR_STATE and b"no step" in L.pbf_last_error(s.ctx)
    buf = np.zeros((s.n, 8), np.float32)
    assert L.pbf_read_buffer(s.ctx, pkg.BUF_COLLIDER_PUSH, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == ERR_STATE
    s.steps(p, 2)
    before, sample, push, wrench = state_bytes(s), s.collider_sample(p, pts), s.collider_push().tobytes(), wrench_bytes(s)
    assert sample["hit"].any() and not sample["hit"].all() and np.frombuffer(push, np.float32).any()

    R, t = PR.GENERIC
    sheared = R.copy()
    sheared[0, 1] += 1e-4
    bad = {"nan in rot": pose(rot=np.where(np.arange(9).reshape(3, 3) == 4, np.nan, R)), "inf in rot": pose(rot=np.where(np.eye(3) > 0, np.inf, R)),
           "nan in trans": pose(trans=(0.0, np.nan, 0.0)), "inf in trans": pose(trans=(np.inf, 0.0, 0.0)),
           "scaled": pose(rot=R * 1.00001), "sheared": pose(rot=sheared), "zero": pose(rot=np.zeros((3, 3))),
           "reflection": pose(rot=np.diag([1.0, 1.0, -1.0])), "rotated reflection": pose(rot=R @ np.diag([-1.0, 1.0, 1.0]))}
    for what, d in bad.items():
        assert L.pbf_set_collider_pose(s.ctx, C.byref(d)) == ERR_INVALID, what
        assert not PR.pose_ok(list(d.rot), list(d.trans)), what
    assert L.pbf_collider_reaction(s.ctx, None) == ERR_INVALID
    # a rotation composed in float32 passes (and is then put back)
    r32 = (PR.rotation((1, 0, 0), 0.4).astype(np.float32) @ PR.rotation((0, 1, 0), -1.1).astype(np.float32)).astype(np.float64)
    assert L.pbf_set_collider_pose(s.ctx, C.byref(pose(rot=r32))) == 0
    assert s.collider_sample(p, pts)["phi"].tobytes() != sample["phi"].tobytes()
    assert L.pbf_set_collider_pose(s.ctx, C.byref(pose())) == 0
    # everything refused: the pose (seen through the sample), the records, the wrench and the particles are what they were
    again = s.collider_sample(p, pts)
    assert all(again[k].tobytes() == sample[k].tobytes() for k in sample)
    assert state_bytes(s) == before and s.collider_push().tobytes() == push and wrench_bytes(s) == wrench
    # an upload makes the records stale until the next step
    s.upload(**sc)
    assert L.pbf_collider_reaction(s.ctx, C.byref(wr)) == ERR_STATE
    s.step(p)
    assert s.collider_reaction()["step"] == 3
    # disabling and enabling again starts a new count
    s.set_collider_reaction(False)
    assert L.pbf_collider_reaction(s.ctx, C.byref(wr)) == ERR_STATE
    s.set_collider_reaction(True).step(p)
    assert s.collider_reaction()["step"] == 1

    # slab mode: a pose or reaction call on a configured ctx is refused; the collider set before stays what it was
    u = install(solver(pkg, False).upload(**sc), case, PR.GENERIC).step(p)
    kept = u.collider_sample(p, pts)
    cut = capi.SlabCut(0, 12, 0, 0)
    assert L.pbf_slab_configure(u.ctx, C.byref(cut), 0, 0) == 0
    assert L.pbf_set_collider_pose(u.ctx, C.byref(pose(rot=np.eye(3)))) == ERR_STATE and b"slab" in L.pbf_last_error(u.ctx)
    assert L.pbf_set_collider_pose(u.ctx, None) == ERR_STATE
    assert L.pbf_set_collider_reaction(u.ctx, 1) == ERR_STATE and b"slab" in L.pbf_last_error(u.ctx)
    assert L.pbf_collider_reaction(u.ctx, C.byref(wr)) == ERR_STATE
    assert all(u.collider_sample(p, pts)[k].tobytes() == kept[k].tobytes() for k in kept)
    s.close()
    u.close()


# ---- 9. the shim and the CLI ---------------------------------------------------------------------------------------------
def test_shim(pkg, tmp_path):
    from pbf_sph_amd import capi
    frames = 4
    sc = pkg.scene_cubes(2048)
    lat, phi64, _ = plane_through(sc, np.float32, 0.4)
    with open(tmp_path / "lattice.bin", "wb") as f:
        f.write(np.array(lat.dims, np.uint32).tobytes() + np.array(BOX_LATTICE["origin"], np.float64).tobytes() +
                np.array([BOX_LATTICE["spacing"], CR.MARGIN], np.float64).tobytes() + lat.phi.tobytes())
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_collider_pose_shim"), str(tmp_path / "lattice.bin"),
                        str(tmp_path / "dump.bin"), str(frames)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    raw = open(tmp_path / "dump.bin", "rb").read()
    n = int(np.frombuffer(raw, np.uint64, 1)[0])
    at = 8

    def take(dtype, shape):
        nonlocal at
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at).reshape(shape)
        at += a.nbytes
        return a

    def particles():
        return dict(id=take(np.uint64, (n,)), type=take(np.uint8, (n,)), mass=take(np.float32, (n,)), pos=take(np.float32, (n, 3)),
                    vel=take(np.float32, (n, 3)), colour=take(np.float32, (n, 4)))

    first, last = particles(), particles()
    # the same frames over the C ABI with the poses the program used: advance() is upload -> step -> download
    s = solver(pkg, False)
    set_lattice(s, lat, phi64, BOX_LATTICE["spacing"]).set_collider_reaction(True)
    p = pkg.default_params(4, 1000.0)
    st = first
    for k in range(frames):
        rot, trans = take(np.float64, (3, 3)), take(np.float64, (3,))
        wrench = raw[at:at + C.sizeof(capi.ColliderWrench)]
        at += len(wrench)
        st = s.upload(**st).set_collider_pose(rot, trans).step(p).download()
        assert wrench_bytes(s) == wrench, k
    assert at == len(raw)
    for k in last:
        assert st[k].tobytes() == last[k].tobytes(), k


def cli_pose(motion, frame, dt):
    """benchmark.cpp's colliderPoseOf, operation for operation in float64 (math.sin / math.cos: the C library's)"""
    m, tau = motion, float(frame) * dt
    wl = math.sqrt((m[3] * m[3] + m[4] * m[4]) + m[5] * m[5])
    angle = wl * tau
    k = [m[3] / wl if wl > 0 else 0.0, m[4] / wl if wl > 0 else 0.0, m[5] / wl if wl > 0 else 0.0]
    K = [0.0, -k[2], k[1], k[2], 0.0, -k[0], -k[1], k[0], 0.0]
    s, c1 = math.sin(angle), 1.0 - math.cos(angle)
    rot = [0.0] * 9
    for a in range(3):
        for b in range(3):
            kk = (K[3 * a] * K[b] + K[3 * a + 1] * K[3 + b]) + K[3 * a + 2] * K[6 + b]
            rot[3 * a + b] = ((1.0 if a == b else 0.0) + s * K[3 * a + b]) + c1 * kk
    trans = [(m[6 + a] - ((rot[3 * a] * m[6] + rot[3 * a + 1] * m[7]) + rot[3 * a + 2] * m[8])) + m[a] * tau for a in range(3)]
    return rot, trans


def test_cli_collider_motion_and_reaction(pkg, tmp_path):
    # the cubes lie in y <= 198 (gravity is +y): the solid y > 150 starts inside them, rises and tilts
    motion = [0.0, -200.0, 0.0, 0.0, 0.0, 0.5, 500.0, 150.0, 500.0]
    common = ["--scene", "cubes", "--particles", "2048", "--solver-iter", "4", "-n", "5", "-w", "0", "--resident", "--no-surface",
              "--collider=plane:0,-1,0,-150,13.5,50"]
    r = subprocess.run([BIN, *common, "--collider-motion=" + ",".join(str(v) for v in motion), "--collider-reaction", "-o",
                        str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.split("\n") if l.startswith('{"frame"')]
    assert [l["frame"] for l in lines] == [0, 1, 2, 3, 4]
    # the same frames from Python: the CLI's lattice is the analytic plane on the box plus one spacing, in double, rounded to N
    ax = -50.0 + np.arange(23, dtype=np.float64) * 50.0
    y = np.broadcast_to(ax[None, :, None], (23, 23, 23))
    phi = ((0.0 * ax[:, None, None] + -1.0 * y) + 0.0 * ax[None, None, :]) / 1.0 - -150.0
    s = solver(pkg, False).upload(**pkg.scene_cubes(2048))
    s.set_collider(phi, (-50.0,) * 3, 50.0, 13.5).set_collider_reaction(True)
    base = pkg.default_params(4, 1000.0)
    hits = 0
    for frame, l in enumerate(lines):
        s.set_collider_pose(*cli_pose(motion, frame, float(np.float32(base.dt)))).step(pkg.apply_motion(base, frame, False))
        w = s.collider_reaction()
        got = l["wrench"]
        for k in ("impulse", "angular", "abs_impulse", "abs_angular"):
            assert list(w[k]) == got[k], (frame, k, w[k], got[k])
        assert (w["hits"], w["particles"], w["step"]) == (got["hits"], got["particles"], got["step"]) and w["step"] == frame + 1
        hits += w["hits"]
    assert hits > 0
    # every second frame; refused with slabs, as --collider is; ignored without a collider
    r = subprocess.run([BIN, *common, "--collider-reaction=2", "-o", str(tmp_path / "o2")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and [json.loads(l)["frame"] for l in r.stdout.split("\n") if l.startswith('{"frame"')] == [1, 3]
    r = subprocess.run([BIN, *common, "--collider-motion=1,0,0", "--slabs", "2", "-o", str(tmp_path / "o3")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0 and "single-device" in r.stderr
    r = subprocess.run([BIN, *common[:-1], "--collider-motion=1,0,0", "-o", str(tmp_path / "o4")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ignored" in r.stdout
    r = subprocess.run([BIN, *common, "--collider-motion=1,0", "-o", str(tmp_path / "o5")], capture_output=True, text=True, timeout=300)
    # (a parse error prints the reason and the usage and exits 0, as the reference's driver does: nothing may have run)
    assert "--collider-motion: expected vx,vy,vz" in r.stderr and "Benchmark completed" not in r.stdout and '{"frame"' not in r.stdout
    r = subprocess.run([BIN, *common, "--collider-reaction=0", "-o", str(tmp_path / "o6")], capture_output=True, text=True, timeout=300)
    assert "--collider-reaction: every must be >= 1" in r.stderr and "Benchmark completed" not in r.stdout
    h = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--collider-motion=" in h and "--collider-reaction" in h
