"""Floating bodies on the device (pbf_set_collider_body, pbf_collider_body_state, pbf_stage_body, include/pbf_hip.h):

  1. the device body equals the host loop — step, pbf_collider_reaction, tests/collider_body_ref.py's advance,
     pbf_set_collider_pose — bit for bit: particles, records, body state and the consumed sums, every step;
  2. the in-step sum equals pbf_collider_reaction beyond one workgroup and beyond one fold trip (65, 1 025, 262 145);
  3. pbf_steps, fused and graphed, gives the eager bytes; no more captures than a constant pose; re-placing captures nothing;
  4. every launch path gives the default path's bytes (coop = 2 within test_hip_parity's tolerance);
  5. stage by stage = one pbf_step; pbf_stage_body before any sort is refused;
  6. off means off: set and cleared = never set; all factors 0 and no accel = the constant-pose run;
  7. physics without a fitted number: free fall above the fluid, slowed by the fluid, a light body ends above a heavy one;
  8. refusals leave everything unchanged.

The CPU side of the restatement: tests/test_collider_body_cpu.py.
"""
import ctypes as C

import numpy as np
import pytest

import collider_body_ref as BR
import collider_pose_ref as PR
import collider_ref as CR
from test_collider_gpu import ERR_INVALID, ERR_STATE, IDS, VARIANTS, dt_of, solver, state_bytes
from test_collider_pose_gpu import body_lattice_through, dense_block, install, wrench_bytes
from test_extras_paths_gpu import PATHS
from test_nversion_cpu import scene

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)


def stock_body(**kw):
    """a start pose that is not the identity, start velocities that are not zero, both dampings, a little gravity; heavy
    against the scenes' fluid (about a thousand unit masses), so that the first impulse does not throw it out of reach"""
    d = dict(mass=2e4, inertia=(2e8, 2.5e8, 3e8), rot=PR.GENERIC[0], centre=PR.GENERIC[1], velocity=(20.0, -10.0, 5.0),
             angular_velocity=(0.3, -0.2, 0.1), gain=0.49, accel=(0.0, 300.0, 0.0), linear_damping=0.2, angular_damping=0.5)
    d.update(kw)
    return BR.Body(**d)


def with_body(pkg, sc, fp64, fast, case, ref, path=None):
    """a ctx with the scene, the lattice and a device body placed where the restated body `ref` stands"""
    s = install(solver(pkg, fp64, fast, path).upload(**sc), case)
    return s.set_collider_body(**ref.kwargs())


def body_bytes(s):
    return bytes(s.collider_body_state(raw=True))


def everything(s):
    out = state_bytes(s)
    out["push"] = s.collider_push().tobytes()
    out["body"] = body_bytes(s)
    return out


def differing(got, want):
    return [k for k in want if got[k] != want[k]]


def first_step_share(sc, dtype, case, pose64):
    """the share of the fluid the restated device function projects at the scene's start positions"""
    lat, _, _, fr = case
    q = (sc["pos"].astype(dtype) / fr[0]).astype(dtype)
    hit = PR.project(lat, fr, PR.pose_of(*pose64, dtype), np.ascontiguousarray(q))[2]
    return float(hit[sc["type"] == 0].mean())


def host_loop(pkg, sc, fp64, fast, case, ref, p, steps, check=None):
    """twin B: no body, the reaction on and a pose set; per step pbf_step, pbf_collider_reaction, the restatement's advance,
    pbf_set_collider_pose.  check(k, twin, ref, wrench) runs after every step.  -> the twin"""
    b = install(solver(pkg, fp64, fast).upload(**sc), case, ref.pose(), reaction=True)
    for k in range(steps):
        b.step(p)
        wr = b.collider_reaction(raw=True)
        ref.advance(float(p.dt), list(wr.impulse), list(wr.angular), int(wr.hits))
        b.set_collider_pose(*ref.pose())
        if check:
            check(k, b, ref, wr)
    return b


# ---- 1. the device body equals the host loop ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", ["cloud", "obstacles", "edges65"])
def test_device_body_equals_the_host_loop(pkg, name, fp64, fast):
    dtype = dt_of(fp64)
    sc = scene(name)
    ref = stock_body()
    case = body_lattice_through(sc, dtype, ref.pose(), 0.15 if name == "edges65" else 0.5)
    share = first_step_share(sc, dtype, case, ref.pose())
    print(f"{name}: {100 * share:.1f} % of the fluid starts inside the solid")
    assert 0.1 <= share <= 0.9, share
    p = pkg.default_params(4, 1000.0)
    a = with_body(pkg, sc, fp64, fast, case, ref)
    assert body_bytes(a) == ref.state_words()                 # the start: the pose as given, q = q(R), the counters at zero
    moved = []

    def check(k, b, ref, wr):
        a.step(p)
        got, want = state_bytes(a), state_bytes(b)
        assert not differing(got, want), (k, differing(got, want))
        assert a.collider_push().tobytes() == b.collider_push().tobytes(), k
        st = a.collider_body_state(raw=True)
        assert bytes(st) == ref.state_words(), (k, a.collider_body_state(), ref.x, ref.q, ref.v, ref.w)
        assert (bytes(st.impulse), bytes(st.angular), int(st.hits)) == (bytes(wr.impulse), bytes(wr.angular), int(wr.hits)), k
        assert st.steps == k + 1 and st.rejected == 0
        if k == 0:
            assert wr.hits > 0 and 0.1 <= wr.particles / float((sc["type"] == 0).sum()) <= 0.9, (wr.hits, wr.particles)
        moved.append(np.abs(np.array(wr.impulse)).max() > 0)

    start = ref.pose()
    host_loop(pkg, sc, fp64, fast, case, ref, p, 12, check)
    assert sum(moved[1:]) >= 3, moved                         # the fluid still acts on the body once it has moved
    assert not np.array_equal(ref.pose()[0], start[0]) and not np.array_equal(ref.pose()[1], start[1])
    # and an untouched body would have gone elsewhere: the same start under accel alone
    free = stock_body()
    for _ in range(12):
        free.advance(float(p.dt), np.zeros(3), np.zeros(3))
    assert free.state_words() != ref.state_words()


# ---- 2. the in-step sum -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", [65, 1025, 262145])
def test_in_step_sum_equals_the_observers(pkg, n, fp64):
    """every particle inside the solid (test_collider_pose_gpu's item 7): a second wave round (65), a second workgroup (1 025)
    and the second 256-record round of the fold (262 145).  The body is frozen so that the solid stays where it is."""
    dtype = dt_of(fp64)
    sc = dense_block(n)
    n_w = PR.GENERIC[0] @ np.array([1.0, 0.0, 0.0])
    case = PR.body_plane_case(PR.GENERIC, dtype, n_w, 5000.0, dims=(41, 41, 41))
    assert case[1].max() < 0
    p = pkg.default_params(2, 1000.0)
    ref = stock_body(linear_factor=(0.0,) * 3, angular_factor=(0.0,) * 3)
    s = with_body(pkg, sc, fp64, False, case, ref).step(p)
    st, wr = s.collider_body_state(raw=True), s.collider_reaction(raw=True)
    assert wr.hits == 2 * n and wr.particles == n and st.steps == 1
    assert (bytes(st.impulse), bytes(st.angular), int(st.hits)) == (bytes(wr.impulse), bytes(wr.angular), int(wr.hits))
    assert np.abs(np.array(st.impulse)).max() > 0 and np.abs(np.array(st.angular)).max() > 0
    ref.advance(float(p.dt), list(wr.impulse), list(wr.angular), int(wr.hits))
    assert bytes(st) == ref.state_words()


# ---- 3. batched and replayed steps --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_batched_and_graphed_steps_give_the_eager_bytes(pkg, fp64, fast):
    dtype = dt_of(fp64)
    sc = scene("cloud")
    case = body_lattice_through(sc, dtype, stock_body().pose())
    p = pkg.default_params(4, 1000.0)
    eager = with_body(pkg, sc, fp64, fast, case, stock_body())
    hits = 0
    for _ in range(12):
        hits += eager.step(p).collider_body_state()["hits"]
    want = everything(eager)
    assert eager.collider_body_state()["steps"] == 12 and hits > 0
    fused = with_body(pkg, sc, fp64, fast, case, stock_body(), dict(graph=0)).steps(p, 12)
    assert not differing(everything(fused), want), differing(everything(fused), want)
    assert fused.graph_stats()[1] == 0
    graphed = with_body(pkg, sc, fp64, fast, case, stock_body(), dict(graph=1)).steps(p, 12)
    assert not differing(everything(graphed), want), differing(everything(graphed), want)
    const = install(solver(pkg, fp64, fast, dict(graph=1)).upload(**sc), case, stock_body().pose(), reaction=True).steps(p, 12)
    g, c = graphed.graph_stats(), const.graph_stats()
    print(f"graphs: body {g}, constant pose {c}")
    assert 0 < g[0] <= c[0] and g[1] > 0 and g[2], (g, c)
    assert state_bytes(const)["pos"] != want["pos"]           # (a body that stood still would have shown)
    # re-placing the body between two batches captures nothing new, and the second batch starts from the new place
    moved = stock_body(centre=PR.GENERIC[1] + np.array([4.0, -3.0, 2.0]), velocity=(0.0, 0.0, 0.0))
    graphed.set_collider_body(**moved.kwargs())
    assert body_bytes(graphed) == moved.state_words()
    graphed.steps(p, 12)
    g2 = graphed.graph_stats()
    assert g2[0] == g[0] and g2[1] > g[1], (g, g2)
    again = eager.set_collider_body(**moved.kwargs())
    for _ in range(12):
        again.step(p)
    assert not differing(everything(graphed), everything(again))


# ---- 4. every launch path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_every_path_gives_the_default_paths_bytes(pkg, fp64, fast):
    sc = scene("obstacles")
    case = body_lattice_through(sc, dt_of(fp64), stock_body().pose())
    p = pkg.default_params(4, 1000.0)

    def run(path=None):
        s = with_body(pkg, sc, fp64, fast, case, stock_body(), path)
        for _ in range(6):
            s.step(p)
        return s

    ref = run()
    want = everything(ref)
    st = ref.collider_body_state()
    assert st["hits"] > 0 and st["steps"] == 6 and np.abs(st["impulse"]).max() > 0
    for path in PATHS + [dict(pipeline=1), dict(fuse_predict=0), dict(row_major=0, gather=0)]:
        got = everything(run(path))
        assert not differing(got, want), (path, differing(got, want))


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_coop_within_the_parity_tolerance(pkg, fp64):
    """coop = 2 changes the summation order: one step from a common state, <= 1e-3 world units (fp32) / 1e-9 (fp64), as
    test_hip_parity.test_wave_cooperative_reader_within_tolerance holds it without a collider"""
    sc = scene("obstacles")
    case = body_lattice_through(sc, dt_of(fp64), stock_body().pose())
    p = pkg.default_params(4, 1000.0)
    warm = with_body(pkg, sc, fp64, False, case, stock_body())
    for _ in range(3):
        warm.step(p)
    st, body = warm.download(), warm.collider_body_state()
    outs = []
    for coop in (0, 2):
        s = install(solver(pkg, fp64, False, dict(coop=coop)).upload(**st), case)
        s.set_collider_body(**stock_body(rot=body["rot"], centre=body["centre"], velocity=body["velocity"],
                                         angular_velocity=body["angular_velocity"]).kwargs())
        outs.append((s.step(p).download(), s.collider_body_state()))
    assert np.array_equal(outs[0][0]["id"], outs[1][0]["id"])
    d = np.linalg.norm(outs[0][0]["pos"].astype(np.float64) - outs[1][0]["pos"].astype(np.float64), axis=1)
    print(f"coop 2 vs 0: largest distance {d.max():.3e} world units")
    assert d.max() <= (1e-9 if fp64 else 1e-3), d.max()
    assert outs[0][1]["hits"] > 0 and outs[1][1]["steps"] == 1


# ---- 5. stage by stage -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_stage_by_stage_equals_one_step(pkg, fp64, fast):
    sc = scene("obstacles")
    case = body_lattice_through(sc, dt_of(fp64), stock_body().pose())
    p = pkg.default_params(4, 1000.0)
    whole = with_body(pkg, sc, fp64, fast, case, stock_body())
    staged = with_body(pkg, sc, fp64, fast, case, stock_body())
    assert staged.L.pbf_stage_body(staged.ctx, C.byref(p)) == ERR_STATE and b"sort" in staged.L.pbf_last_error(staged.ctx)
    assert body_bytes(staged) == stock_body().state_words()
    for _ in range(2):
        whole.step(p)
        staged.stage("predict", p).stage("sort", p).stage("diffuse", p)
        for _ in range(4):
            staged.stage("lambda", p).stage("delta", p)
        staged.stage("body", p).stage("finalise", p)
        assert not differing(everything(staged), everything(whole))
    assert whole.collider_body_state()["hits"] > 0
    plain = install(solver(pkg, fp64, fast).upload(**sc), case)
    assert plain.L.pbf_stage_body(plain.ctx, C.byref(p)) == ERR_STATE and b"no body" in plain.L.pbf_last_error(plain.ctx)


# ---- 6. off means off -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_a_body_set_and_cleared_is_a_body_never_set(pkg, fp64, fast):
    sc = scene("cloud")
    pose = stock_body().pose()
    case = body_lattice_through(sc, dt_of(fp64), pose)
    p = pkg.default_params(4, 1000.0)
    never = install(solver(pkg, fp64, fast).upload(**sc), case, pose, reaction=True).steps(p, 6)
    s = with_body(pkg, sc, fp64, fast, case, stock_body(centre=(300.0, 200.0, 100.0)))
    s.set_collider_body(None).set_collider_body(None)
    from pbf_sph_amd import capi
    assert s.L.pbf_collider_body_state(s.ctx, C.byref(capi.ColliderBodyState())) == ERR_STATE
    s.set_collider_pose(*pose).steps(p, 6)
    want, got = state_bytes(never), state_bytes(s)
    assert not differing(got, want) and s.collider_push().tobytes() == never.collider_push().tobytes()
    assert wrench_bytes(s) == wrench_bytes(never)
    assert s.collider_reaction()["hits"] > 0
    # turned off after some steps, the solid stays where the body left it, as an ordinary pose
    b = with_body(pkg, sc, fp64, fast, case, stock_body()).steps(p, 3)
    st = b.collider_body_state()
    b.set_collider_body(None).steps(p, 3)
    c = install(solver(pkg, fp64, fast).upload(**sc), case)
    c.set_collider_body(**stock_body().kwargs()).steps(p, 3)
    c.set_collider_body(None).set_collider_pose(st["rot"], st["centre"]).steps(p, 3)
    assert not differing(state_bytes(b), state_bytes(c))


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_a_frozen_body_is_the_constant_pose(pkg, fp64, fast):
    """all factors 0 and accel = 0.  The start rotation is the identity: its quaternion (1, 0, 0, 0) has norm exactly 1, so the
    normalisation of every advance returns it and R(q) is the identity for ever; under a generic rotation |q| rounds and the
    pose record may move by an ulp of double in the first advances, which is the contract and not what this test is about."""
    sc = scene("cloud")
    pose = (np.eye(3), np.array([35.0, -60.0, 20.0]))
    case = body_lattice_through(sc, dt_of(fp64), pose)
    p = pkg.default_params(4, 1000.0)
    const = install(solver(pkg, fp64, fast).upload(**sc), case, pose, reaction=True).steps(p, 6)
    ref = stock_body(rot=pose[0], centre=pose[1], linear_factor=(0.0,) * 3, angular_factor=(0.0,) * 3, accel=(0.0,) * 3)
    s = with_body(pkg, sc, fp64, fast, case, ref).steps(p, 6)
    assert not differing(state_bytes(s), state_bytes(const))
    assert s.collider_push().tobytes() == const.collider_push().tobytes() and wrench_bytes(s) == wrench_bytes(const)
    st = s.collider_body_state()
    assert st["steps"] == 6 and st["hits"] > 0 and np.array_equal(st["rot"], np.eye(3)) and np.array_equal(st["centre"], pose[1])
    assert not st["velocity"].any() and not st["angular_velocity"].any()
    free = state_bytes(with_body(pkg, sc, fp64, fast, case, stock_body(rot=pose[0], centre=pose[1])).steps(p, 6))
    assert free["pos"] != state_bytes(const)["pos"]           # (a body that is free to move does move here)


# ---- 7. physics without a fitted number ---------------------------------------------------------------------------------------
TANK_K, TANK_LAYERS, RADIUS = 26, 15, 60.0
TANK_SIDE = TANK_K * 27.0                                     # 702: the block fills the box's floor (gravity is +y)
TANK_TOP = TANK_SIDE - TANK_LAYERS * 27.0                     # the fluid's surface, about y = 297
BALL = dict(origin=(-100.0,) * 3, spacing=20.0, dims=(11, 11, 11))
DISPLACED = 4.0 / 3.0 * np.pi * RADIUS ** 3 / 27.0 ** 3      # the mass of the fluid a submerged ball displaces: 46 particles


def tank():
    g = np.stack(np.meshgrid(np.arange(TANK_K), np.arange(TANK_LAYERS), np.arange(TANK_K), indexing="ij"), -1).reshape(-1, 3)
    n = len(g)
    pos = g * 27.0 + np.array([13.5, TANK_TOP + 13.5, 13.5])
    return dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n), pos=pos, vel=np.zeros((n, 3)),
                colour=np.full((n, 4), 0.5))


@pytest.fixture(scope="module")
def settled(pkg):
    """the block after 40 steps in its own box, computed once"""
    p = pkg.default_params(4, TANK_SIDE)
    return solver(pkg, False).upload(**tank()).steps(p, 40).download()


def ball(pkg, st, **kw):
    """the settled tank with a ball lattice in the body frame (centre at the frame's origin) and a body on"""
    s = solver(pkg, False).upload(**st)
    phi = pkg.sdf_lattice(pkg.sdf_sphere((0.0, 0.0, 0.0), RADIUS), BALL["origin"], BALL["spacing"], BALL["dims"])
    s.set_collider(phi, BALL["origin"], BALL["spacing"], CR.MARGIN)
    d = dict(inertia=(0.4 * kw.get("mass", 1.0) * RADIUS ** 2,) * 3, rot=np.eye(3), gain=0.49, accel=(0.0, 4900.0, 0.0),
             centre_min=(RADIUS,) * 3, centre_max=(TANK_SIDE - RADIUS,) * 3)
    d.update(kw)
    return s.set_collider_body(**d), BR.Body(**d)


def test_tank_free_fall_above_the_fluid(pkg, settled):
    """(a) the ball starts well above the fluid and does not reach it: its path is the closed form of the CPU test's item 1,
    x_k = x_0 + dt^2 a k (k + 1) / 2 within 4 k eps max|x|"""
    assert len(settled["id"]) > 10000
    p = pkg.default_params(4, TANK_SIDE)
    x0, accel = np.array([351.0, 100.0, 351.0]), np.array([0.0, 500.0, 0.0])
    s, ref = ball(pkg, settled, mass=DISPLACED, centre=x0, accel=accel)
    dt = float(p.dt)
    for k in range(1, 13):
        st = s.step(p).collider_body_state()
        ref.advance(dt, np.zeros(3), np.zeros(3))
        assert st["hits"] == 0 and st["steps"] == k
        want = x0 + dt * dt * accel * (k * (k + 1) / 2.0)
        assert np.abs(st["centre"] - want).max() <= 4 * k * EPS * np.abs(want).max(), (k, st["centre"] - want)
        assert body_bytes(s) == ref.state_words()
    assert st["centre"][1] + RADIUS + CR.MARGIN < TANK_TOP - 27.0


def test_tank_the_fluid_slows_the_ball(pkg, settled):
    """(b) dropped onto the fluid: from the first contact on, the ball falls more slowly than the restated free fall at the
    same step; its centre stays finite and inside its bounds"""
    p = pkg.default_params(4, TANK_SIDE)
    x0 = np.array([351.0, TANK_TOP - RADIUS - 30.0, 351.0])
    s, ref = ball(pkg, settled, mass=DISPLACED, centre=x0, velocity=(0.0, 300.0, 0.0))
    ref.centre_min[:], ref.centre_max[:] = -np.inf, np.inf     # (the free fall is not stopped by the floor either)
    touched = 0
    for k in range(30):
        st = s.step(p).collider_body_state()
        ref.advance(float(p.dt), np.zeros(3), np.zeros(3))
        touched += st["hits"] > 0
        assert np.isfinite(st["centre"]).all() and (st["centre"] >= RADIUS).all() and (st["centre"] <= TANK_SIDE - RADIUS).all()
        if touched:
            assert st["velocity"][1] < ref.v[1], (k, st["velocity"], ref.v)
    print(f"the ball touched the fluid in {touched} of 30 steps; it ends at y = {st['centre'][1]:.1f} with v_y = {st['velocity'][1]:.1f}, "
          f"free fall: y = {ref.x[1]:.1f}, v_y = {ref.v[1]:.1f}")
    assert touched > 0 and st["rejected"] == 0


def test_tank_a_light_ball_ends_above_a_heavy_one(pkg, settled):
    """(c) two runs that differ in mass and inertia alone, a tenth and ten times the displaced fluid's mass"""
    p = pkg.default_params(4, TANK_SIDE)
    x0 = np.array([351.0, TANK_TOP - RADIUS - 30.0, 351.0])
    ends = []
    for mass in (0.1 * DISPLACED, 10.0 * DISPLACED):
        s, _ = ball(pkg, settled, mass=mass, centre=x0, velocity=(0.0, 300.0, 0.0))
        hits = 0
        for _ in range(4):
            hits += s.steps(p, 10).collider_body_state()["hits"] > 0
        st = s.collider_body_state()
        assert hits > 0 and st["steps"] == 40 and np.isfinite(st["centre"]).all()
        ends.append(st["centre"][1])
    print(f"light ball ends at y = {ends[0]:.1f}, heavy ball at y = {ends[1]:.1f} (gravity is +y; the floor is at {TANK_SIDE})")
    assert ends[0] < ends[1], ends


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_unchanged(pkg):
    from pbf_sph_amd import capi
    from test_collider_body_cpu import REFUSALS
    sc = scene("cloud")
    ref = stock_body()
    case = body_lattice_through(sc, np.float32, ref.pose())
    p = pkg.default_params(4, 1000.0)

    s = solver(pkg, False).upload(**sc)
    L = s.L
    good = capi.collider_body(**ref.kwargs())
    assert L.pbf_set_collider_body(s.ctx, C.byref(good)) == ERR_STATE and b"no collider" in L.pbf_last_error(s.ctx)
    assert L.pbf_set_collider_body(s.ctx, None) == ERR_STATE
    assert L.pbf_collider_body_state(s.ctx, C.byref(capi.ColliderBodyState())) == ERR_STATE
    install(s, case).set_collider_body(**ref.kwargs()).steps(p, 2)
    before, push, body = state_bytes(s), s.collider_push().tobytes(), body_bytes(s)
    assert np.frombuffer(push, np.float32).any() and s.collider_body_state()["steps"] == 2

    for what, (kw, reason) in REFUSALS.items():
        d = ref.kwargs()
        d.update(kw)
        assert L.pbf_set_collider_body(s.ctx, C.byref(capi.collider_body(**d))) == ERR_INVALID, what
        assert reason.encode() in L.pbf_last_error(s.ctx), (what, L.pbf_last_error(s.ctx))
    assert L.pbf_collider_body_state(s.ctx, None) == ERR_INVALID
    # while a body is on the pose and the records are its own
    pose = capi.ColliderPose()
    pose.rot[:], pose.trans[:] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], [0.0, 0.0, 0.0]
    assert L.pbf_set_collider_pose(s.ctx, C.byref(pose)) == ERR_STATE and b"body" in L.pbf_last_error(s.ctx)
    assert L.pbf_set_collider_pose(s.ctx, None) == ERR_STATE
    assert L.pbf_set_collider_reaction(s.ctx, 0) == ERR_STATE and b"body" in L.pbf_last_error(s.ctx)
    assert L.pbf_set_collider_reaction(s.ctx, 1) == 0
    assert state_bytes(s) == before and s.collider_push().tobytes() == push and body_bytes(s) == body
    # and the next step is the one an undisturbed twin takes
    twin = install(solver(pkg, False).upload(**sc), case).set_collider_body(**stock_body().kwargs()).steps(p, 3)
    assert not differing(everything(s.step(p)), everything(twin))

    # a new collider, clearing included, turns the body off
    lat, phi64, origin, _ = case
    s.set_collider(phi64, origin, PR.BODY_SPACING, CR.MARGIN)
    assert L.pbf_collider_body_state(s.ctx, C.byref(capi.ColliderBodyState())) == ERR_STATE
    assert L.pbf_set_collider_pose(s.ctx, C.byref(pose)) == 0
    s.set_collider_body(**ref.kwargs()).set_collider(None)
    assert L.pbf_collider_body_state(s.ctx, C.byref(capi.ColliderBodyState())) == ERR_STATE
    free = solver(pkg, False).upload(**s.download()).step(p)
    assert state_bytes(s.step(p)) == state_bytes(free)        # (and the step is the one without a collider)

    # slab mode: refused on a configured ctx; the collider set before stays what it was
    u = install(solver(pkg, False).upload(**sc), case, ref.pose()).step(p)
    pts = np.random.default_rng(2).random((500, 3)) * 1000.0
    kept = u.collider_sample(p, pts)
    cut = capi.SlabCut(0, 12, 0, 0)
    assert L.pbf_slab_configure(u.ctx, C.byref(cut), 0, 0) == 0
    assert L.pbf_set_collider_body(u.ctx, C.byref(good)) == ERR_STATE and b"slab" in L.pbf_last_error(u.ctx)
    assert L.pbf_set_collider_body(u.ctx, None) == ERR_STATE
    assert all(u.collider_sample(p, pts)[k].tobytes() == kept[k].tobytes() for k in kept)
    s.close()
    u.close()
