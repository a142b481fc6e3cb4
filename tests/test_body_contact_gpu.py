"""The body's contact with the scenery on the device (pbf_set_collider_body_contact, pbf_collider_body_contact_points,
pbf_collider_body_contact_state, include/pbf_hip.h):

  1. the surface points equal the restatement (tests/body_contact_ref.py) bit for bit, count and order, up to a lattice whose
     scan takes k_scan_sums beyond its first trip; a lattice without a crossing is refused;
  2. the raw sums of a pass against math.fsum of the NumPy per-point terms within gamma_(p-1) sum|t|, depth_max and the counts
     exactly, for 1, 65, 1 025 points and beyond one trip of the fold of the partial records;
  3. the chain: 12 steps whose every body state and contact state is the NumPy resolve() fed the device's own raw sums, behind
     collider_body_ref's advance(), bit for bit — in contact, separating and out of contact, friction off and on;
  4. eager steps, pbf_steps and replayed graphs give the same bytes; a rewritten record captures nothing, off -> on does, and
     a replay sees a replaced scenery;
  5. off is off: configured and cleared = never configured, bytes and captures;
  6. physics: a ball comes to rest on a floor it otherwise falls through; a second pass per step leaves less depth; a box
     dropped flat does not turn, dropped on a corner it turns the way of r x n; a floating ball stops at a wall; friction slows
     a sliding box;
  7. refusals leave everything unchanged; a cleared body, a replaced collider and cleared scenery turn contact off; a
     re-placed body keeps it;
  8. the C++ shim and the benchmark CLI give the C ABI's bytes.

The CPU side: tests/test_body_contact_cpu.py.
"""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import body_contact_ref as BC
import collider_body_ref as BR
import collider_pose_ref as PR
import collider_ref as CR
from test_collider_body_gpu import DISPLACED, RADIUS, TANK_SIDE, TANK_TOP, settled, tank  # noqa: F401  (settled: a fixture)
from test_collider_gpu import ERR_INVALID, ERR_STATE, IDS, VARIANTS, dt_of, solver, state_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pbf-sph_amd")
EPS = float(np.finfo(np.float64).eps)
U = EPS / 2                                                   # the unit roundoff of a double

# the ball of test_collider_body_gpu: radius 60 on an 11^3 lattice of spacing 20 in the body frame
BALL = dict(origin=(-100.0,) * 3, spacing=20.0, dims=(11, 11, 11))
# a box with half extents (60, 40, 50) on a 21^3 lattice of spacing 10
BOX_HALF = (60.0, 40.0, 50.0)
BOX = dict(origin=(-100.0,) * 3, spacing=10.0, dims=(21, 21, 21))
FLOOR_Y = 800.0                                               # the scenery's floor: solid where y > 800 (gravity is +y)
SCENE = CR.BLOCK_LATTICE                                      # the box plus one spacing of 50


def ball_phi():
    return CR.lattice_of(lambda x: CR.sphere_phi((0.0, 0.0, 0.0), RADIUS, x), BALL["origin"], BALL["spacing"], BALL["dims"])


def box_phi():
    def f(x):
        q = np.abs(x) - np.array(BOX_HALF)
        return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)
    return CR.lattice_of(f, BOX["origin"], BOX["spacing"], BOX["dims"])


def floor_phi(y=FLOOR_Y):
    return CR.lattice_of(lambda x: CR.plane_phi((0.0, -1.0, 0.0), -y, x), SCENE["origin"], SCENE["spacing"], SCENE["dims"])


def far_particles():
    """65 particles in a corner of the box, 300 world units from every body here: steps run, nothing touches the solid"""
    g = np.stack(np.meshgrid(np.arange(5), np.arange(13), indexing="ij"), -1).reshape(-1, 2)
    n = len(g)
    pos = np.stack([40.0 + 27.0 * g[:, 0], np.full(n, 700.0), 40.0 + 27.0 * g[:, 1]], axis=1)
    return dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n), pos=pos, vel=np.zeros((n, 3)),
                colour=np.full((n, 4), 0.5))


def free_body(**kw):
    """a body no bound holds: what stops it is the scenery or nothing"""
    d = dict(mass=46.0, inertia=(0.4 * 46.0 * RADIUS ** 2,) * 3, rot=np.eye(3), centre=(500.0, 700.0, 500.0), gain=0.49,
             accel=(0.0, 4900.0, 0.0))
    d.update(kw)
    return BR.Body(**d)


def rig(pkg, fp64, body, collider, scenery, fast=False, path=None, sc=None):
    """particles, the collider's lattice (phi, geometry) in the body frame, a body placed where `body` stands, the scenery"""
    s = solver(pkg, fp64, fast, path).upload(**(sc or far_particles()))
    s.set_collider(collider[0], collider[1]["origin"], collider[1]["spacing"], 0.0)
    s.set_scenery(scenery[0], scenery[1], scenery[2], 0.0)
    return s.set_collider_body(**body.kwargs())


def contact_bytes(s):
    return bytes(s.collider_body_contact_state(raw=True))


def body_bytes(s):
    return bytes(s.collider_body_state(raw=True))


def everything(s):
    out = state_bytes(s)
    out["body"], out["contact"] = body_bytes(s), contact_bytes(s)
    return out


def differing(got, want):
    return [k for k in want if got[k] != want[k]]


FLOOR = (floor_phi(), SCENE["origin"], SCENE["spacing"])


# ---- 1. the points -------------------------------------------------------------------------------------------------------------
def scan_trip():
    """entries one trip of k_scan_sums covers, read off the kernels: BLOCK block sums of BLOCK * SCAN_ITEMS entries each"""
    src = open(os.path.join(PKG, "csrc", "pbf_kernels.hpp")).read()
    block = int(re.search(r"constexpr int BLOCK = (\d+);", src).group(1))
    items = int(re.search(r"constexpr int SCAN_ITEMS = (\d+);", src).group(1))
    assert re.search(r"for \(uint32_t base = 0; base < nb; base \+= BLOCK\)", src) and "SCAN_TILE = BLOCK * SCAN_ITEMS" in src
    return block * block * items


def alternating(dims):
    """phi(i, j, k) = 0.25 (-1)^i: every cell is crossed and gives one point, its centre"""
    return np.broadcast_to((0.25 * (-1.0) ** np.arange(dims[0]))[:, None, None], dims).copy()


def big_alternating_side():
    """66^3 nodes, enlarged until the scan of its cells (one entry per cell and the closing one) passes one trip of k_scan_sums"""
    side = 66
    while (side - 1) ** 3 + 1 <= scan_trip():
        side += 1
    return side


def point_lattices():
    sphere = CR.lattice_of(lambda x: CR.sphere_phi((85.0, 80.0, 78.0), 52.0, x), (0.0, 0.0, 0.0), 10.0, (17, 17, 17))
    holed = sphere.copy()
    holed[3:6, 8, 8] = np.inf
    holed[8, 12:14, 9] = np.inf
    tilted = lambda dims, o, h: CR.lattice_of(lambda x: CR.plane_phi((0.3, 0.5, -0.4), 1.0 + o[1], x), o, h, dims)
    return {
        "single-cell": (tilted((2, 2, 2), (-8.0, -6.0, -7.0), 16.0), (-8.0, -6.0, -7.0), 16.0, 0.0, 1),
        "3x2x5": (tilted((3, 2, 5), (-9.0, -2.0, -11.0), 6.0), (-9.0, -2.0, -11.0), 6.0, 0.0, 1),
        "sphere": (sphere, (0.0, 0.0, 0.0), 10.0, 1.5, 1),
        "sphere-stride2": (sphere, (0.0, 0.0, 0.0), 10.0, 1.5, 2),
        "inf-nodes": (holed, (0.0, 0.0, 0.0), 10.0, 0.0, 1),
    }


def configure_points(pkg, fp64, fast, phi, origin, spacing, level, stride):
    s = rig(pkg, fp64, free_body(), (phi, dict(origin=origin, spacing=spacing)), FLOOR, fast)
    return s.set_collider_body_contact(level=level, stride=stride)


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", list(point_lattices()))
def test_points_equal_the_restatement(pkg, name, fp64, fast):
    phi, origin, spacing, level, stride = point_lattices()[name]
    want = BC.points(phi, origin, spacing, level, stride, dt_of(fp64))
    s = configure_points(pkg, fp64, fast, phi, origin, spacing, level, stride)
    got = s.collider_body_contact_points()
    print(f"{name}: {len(want)} points")
    assert len(want) > 0 and got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert s.collider_body_contact_state()["points"] == len(want)
    if name == "single-cell":
        assert len(want) == 1
    if name == "inf-nodes":                                    # (the cells around an infinite node give no point)
        assert len(want) < len(BC.points(point_lattices()["sphere"][0], origin, spacing, level, stride, dt_of(fp64)))


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_points_beyond_one_trip_of_the_scan(pkg, fp64):
    side = big_alternating_side()
    cells = (side - 1) ** 3
    assert cells + 1 > scan_trip() and side >= 66
    phi = alternating((side,) * 3)
    origin, spacing = (-float(side - 1),) * 3, 2.0
    want = BC.points(phi, origin, spacing, 0.0, 1, dt_of(fp64))
    assert len(want) == cells
    got = configure_points(pkg, fp64, False, phi, origin, spacing, 0.0, 1).collider_body_contact_points()
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


def test_a_lattice_without_a_crossing_is_refused(pkg):
    from pbf_sph_amd import capi
    s = rig(pkg, False, free_body(), (ball_phi(), BALL), FLOOR)
    c = capi.BodyContact(500.0, 1, 0.0, 0.0, 0.0, 0.8, 0.0, 1)     # (no node of the ball's lattice reaches 500)
    before = everything_but_contact(s)
    assert s.L.pbf_set_collider_body_contact(s.ctx, C.byref(c)) == ERR_INVALID and b"no point" in s.L.pbf_last_error(s.ctx)
    assert s.L.pbf_collider_body_contact_state(s.ctx, C.byref(capi.BodyContactState())) == ERR_STATE
    assert everything_but_contact(s) == before


def everything_but_contact(s):
    out = state_bytes(s)
    out["body"] = body_bytes(s)
    return out


# ---- 2. the sums ------------------------------------------------------------------------------------------------------------------
def sum_cases():
    return {1: (2, 2, 2), 65: (6, 14, 2), 1025: (6, 6, 42), "big": (big_alternating_side(),) * 3}


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", [1, 65, 1025, "big"])
def test_raw_sums_against_fsum(pkg, n, fp64):
    """Every point of a frozen body lies inside a scenery plane.  A sum of p terms in any order is within gamma_(p-1) sum|t| of
    the exact sum, gamma_k = k u / (1 - k u) (the fold here is a tree, whose depth is far below p - 1, and math.fsum's own
    rounding fits into that slack; with one term both sides are the term itself).  The terms are the same operations on both
    sides and carry no error of their own."""
    dims = sum_cases()[n]
    p = int(np.prod([d - 1 for d in dims]))
    if n == "big":
        block = int(re.search(r"constexpr int BLOCK = (\d+);", open(os.path.join(PKG, "csrc", "pbf_kernels.hpp")).read()).group(1))
        partials = (p + 1024 - 1) // 1024                         # (DIAG_TILE points per record)
        assert partials > block and p >= 274625, (partials, block)
    else:
        assert p == n
    origin, spacing = tuple(-(d - 1) * 1.0 for d in dims), 2.0
    body = free_body(rot=PR.GENERIC[0], centre=(500.0, 520.0, 480.0), accel=(0.0, 0.0, 0.0), linear_factor=(0.0,) * 3,
                     angular_factor=(0.0,) * 3)
    scenery = (floor_phi(300.0), SCENE["origin"], SCENE["spacing"])    # solid where y > 300: the whole body is inside
    s = rig(pkg, fp64, body, (alternating(dims), dict(origin=origin, spacing=spacing)), scenery)
    s.set_collider_body_contact(skin=1.5, restitution=0.5, friction=0.3).step(pkg.default_params(4, 1000.0))
    pts, st, cs = s.collider_body_contact_points(), s.collider_body_state(), s.collider_body_contact_state()
    assert len(pts) == p and cs["points"] == p and cs["passes"] == 1
    r, contact, m, d = BC.terms(pts, st["rot"], st["centre"], scenery, 1.5)
    assert contact.all()
    S, M, A, D, count, absum = BC.fold(r, contact, m, d)
    gamma = (p - 1) * U / (1 - (p - 1) * U)
    got = np.concatenate([[cs["depth_sum"]], cs["push"], cs["arm"]])
    want = np.concatenate([[S], M, A])
    err = np.abs(got - want)
    print(f"{p} points: worst error / bar {np.max(err / np.maximum(gamma * absum, 1e-300)):.3g}")
    assert (err <= gamma * absum).all(), (err, gamma * absum)
    assert cs["depth_max"] == D and (cs["contacts"], cs["rejected"]) == (1, 0)


# ---- 3. the chain ---------------------------------------------------------------------------------------------------------------
def bouncing(**kw):
    """above the floor on its way down and sideways, turning: it reaches the floor in its third step, bounces, leaves the skin
    and comes back (the NumPy loop: none, none, hit, separating, none, none, then hits that slide and hits that stick)"""
    d = dict(centre=(500.0, 728.0, 500.0), velocity=(200.0, 300.0, -50.0), angular_velocity=(0.5, -0.3, 0.2), rot=PR.GENERIC[0])
    d.update(kw)
    return free_body(**d)


CHAIN = dict(skin=6.0, restitution=0.3, friction=0.0, correction=0.3, slop=0.5)


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_chain_equals_the_numpy_resolve(pkg, fp64, fast):
    p = pkg.default_params(4, 1000.0)
    ref = bouncing()
    s = rig(pkg, fp64, ref, (ball_phi(), BALL), FLOOR, fast).set_collider_body_contact(**CHAIN)
    n = len(s.collider_body_contact_points())
    c = BC.Contact(CHAIN["skin"], CHAIN["restitution"], CHAIN["friction"], CHAIN["correction"], CHAIN["slop"], points=n)
    assert contact_bytes(s) == c.state_words() and body_bytes(s) == ref.state_words()
    kinds, branches = [], set()
    for k in range(12):
        if k == 6:                                            # friction on: the record is rewritten, the counters start again
            s.set_collider_body_contact(**dict(CHAIN, friction=0.4))
            c = BC.Contact(CHAIN["skin"], CHAIN["restitution"], 0.4, CHAIN["correction"], CHAIN["slop"], points=n)
            assert contact_bytes(s) == c.state_words()
        s.step(p)
        st, cs = s.collider_body_state(raw=True), s.collider_body_contact_state(raw=True)
        ref.advance(float(p.dt), list(st.impulse), list(st.angular), int(st.hits))
        # (a point in contact has d > 0, so the pass found one iff its largest depth is positive)
        c.resolve(ref, cs.depth_sum, list(cs.push), list(cs.arm), cs.depth_max, 1 if cs.depth_max > 0 else 0)
        assert bytes(st) == ref.state_words(), (k, s.collider_body_state(), ref.x, ref.v, ref.w)
        assert bytes(cs) == c.state_words(), (k, s.collider_body_contact_state(), c.impulse, c.shift)
        kinds.append("none" if cs.depth_max == 0 else "hit" if np.abs(c.impulse).max() > 0 else "separating")
        branches.add((k >= 6, c.branch))
    print(kinds, branches)
    assert {"none", "hit", "separating"} <= set(kinds), kinds
    assert "hit" in kinds[:6] and "hit" in kinds[6:] and any(b for on, b in branches if on) and not any(b for on, b in branches if not on)


# ---- 4. the same bytes on every path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_batched_and_graphed_steps_give_the_eager_bytes(pkg, fp64, fast):
    p = pkg.default_params(4, 1000.0)
    higher = (floor_phi(790.0), SCENE["origin"], SCENE["spacing"])

    def run(path, batched):
        s = rig(pkg, fp64, bouncing(), (ball_phi(), BALL), FLOOR, fast, path).set_collider_body_contact(**CHAIN)
        stats = []
        for stage in range(3):
            if stage == 1:                                    # a rewritten record: another restitution, friction on
                s.set_collider_body_contact(**dict(CHAIN, restitution=0.2, friction=0.4))
            if stage == 2:                                    # a replaced scenery: the floor comes up by 10
                s.set_scenery(*higher, 0.0)
            if batched:
                s.steps(p, 12)
            else:
                for _ in range(12):
                    s.step(p)
            stats.append(s.graph_stats())
        return s, stats

    eager, _ = run(None, False)
    want = everything(eager)
    assert eager.collider_body_contact_state()["contacts"] > 0
    fused, st = run(dict(graph=0), True)
    assert not differing(everything(fused), want) and st[-1][1] == 0
    graphed, st = run(dict(graph=1), True)
    assert not differing(everything(graphed), want), differing(everything(graphed), want)
    print("graph stats per stage:", st)
    assert st[0][0] > 0 and st[0][1] > 0 and st[0][2]
    assert st[1][0] == st[0][0] and st[1][1] > st[0][1]       # one capture across the rewrite
    assert st[2][0] > st[1][0]                                # the replaced scenery is captured anew, and the replay saw it:
    unreplaced = rig(pkg, fp64, bouncing(), (ball_phi(), BALL), FLOOR, fast).set_collider_body_contact(**CHAIN)
    for _ in range(12):
        unreplaced.step(p)
    unreplaced.set_collider_body_contact(**dict(CHAIN, restitution=0.2, friction=0.4))
    for _ in range(24):
        unreplaced.step(p)
    assert body_bytes(unreplaced) != want["body"]
    # off -> on is a new capture; on -> off as well
    g = rig(pkg, fp64, bouncing(), (ball_phi(), BALL), FLOOR, fast, dict(graph=1)).steps(p, 8)
    a = g.graph_stats()
    g.set_collider_body_contact(**CHAIN).steps(p, 8)
    b = g.graph_stats()
    g.set_collider_body_contact(on=False).steps(p, 8)
    c = g.graph_stats()
    assert a[0] > 0 and b[0] > a[0] and c[0] > b[0], (a, b, c)
    # another number of passes is another launch sequence
    g.set_collider_body_contact(**CHAIN).steps(p, 8)
    d = g.graph_stats()
    g.set_collider_body_contact(**dict(CHAIN, iterations=3)).steps(p, 8)
    e = g.graph_stats()
    assert e[0] > d[0] and g.collider_body_contact_state()["passes"] == 24


# ---- 5. off is off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_configured_and_cleared_equals_never_configured(pkg, fp64, fast):
    p = pkg.default_params(4, 1000.0)
    sc = tank()                                               # (a body the fluid does touch, scenery the fluid does touch)
    scenery = (floor_phi(650.0), SCENE["origin"], SCENE["spacing"])
    body = lambda: free_body(centre=(351.0, TANK_TOP - 20.0, 351.0), velocity=(0.0, 300.0, 0.0), mass=DISPLACED,
                             centre_max=(np.inf, 640.0, np.inf))
    outs = []
    for touch in (False, True, "on"):
        s = rig(pkg, fp64, body(), (ball_phi(), BALL), scenery, fast, dict(graph=1), sc)
        if touch:
            s.set_collider_body_contact(**CHAIN)
        if touch is True:
            s.set_collider_body_contact(on=False)
        s.steps(p, 6)
        out = everything_but_contact(s)
        out["stats"] = s.graph_stats()
        outs.append(out)
        if touch is True:
            assert s.L.pbf_collider_body_contact_state(s.ctx, None) == ERR_INVALID
    never, cleared, on = outs
    assert not differing(cleared, never), differing(cleared, never)
    assert on["stats"][0] >= never["stats"][0]
    hits = np.frombuffer(never["body"], np.uint64)[-3]
    assert hits > 0                                           # (the fluid pushed the body: the reaction path ran in all three)


# ---- 6. physics ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_a_ball_comes_to_rest_on_the_floor_it_otherwise_falls_through(pkg, fp64):
    """THE test that fails without the feature.  Gravity, no fluid near: without contact the centre ends below the floor; with
    it (e = 0) the ball rests with its lowest point within one spacing of the ball's lattice of the floor."""
    p = pkg.default_params(4, 1000.0)
    through = rig(pkg, fp64, free_body(), (ball_phi(), BALL), FLOOR).steps(p, 60).collider_body_state()
    assert through["centre"][1] > FLOOR_Y + RADIUS
    s = rig(pkg, fp64, free_body(), (ball_phi(), BALL), FLOOR).set_collider_body_contact(restitution=0.0).steps(p, 60)
    st, cs = s.collider_body_state(), s.collider_body_contact_state()
    print(f"the ball rests at y = {st['centre'][1]:.3f} with v_y = {st['velocity'][1]:.3g}; {cs['contacts']} of {cs['passes']} passes responded")
    assert st["centre"][1] < FLOOR_Y and abs(st["centre"][1] + RADIUS - FLOOR_Y) <= BALL["spacing"]
    assert abs(st["velocity"][1]) <= 4900.0 * float(p.dt) and cs["contacts"] > 20 and cs["rejected"] == 0


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_a_second_pass_leaves_less_depth(pkg, fp64):
    """iterations = 2: the depth the second pass of a step finds stays below what the NumPy loop of the same run shows for
    that pass, plus the rounding of N on the world coordinate (8 ulps of 1 000).  Measured: the NumPy loop's largest
    second-pass depth over the 60 steps is 1.195526 world units in fp32 (1.195535 in fp64; the first pass: 5.977631) and the
    device's 1.195526 (fp32).  In the NumPy loop itself every second pass finds the share 1 - correction of what the first pass of its step found, within the same rounding: the
    floor's push is straight up (n = (0, -1, 0) exactly), and the first pass shifts the centre by correction x depth along it."""
    p = pkg.default_params(4, 1000.0)
    s = rig(pkg, fp64, free_body(), (ball_phi(), BALL), FLOOR).set_collider_body_contact(restitution=0.0, iterations=2)
    pts = s.collider_body_contact_points()
    ulps = 8 * float(np.finfo(dt_of(fp64)).eps) * 1000.0
    depth = {}
    ref, c = free_body(), BC.Contact(points=len(pts))
    BC.simulate(ref, c, pts, FLOOR, float(p.dt), 60, 2, each=lambda k, it, D, n: depth.__setitem__((k, it), D))
    first, second = [depth[k, 0] for k in range(60)], [depth[k, 1] for k in range(60)]
    assert max(first) > 0 and all(abs(d2 - (1.0 - 0.8) * d1) <= ulps for d1, d2 in zip(first, second))
    bar = max(second) + ulps
    worst = 0.0
    for k in range(60):
        cs = s.step(p).collider_body_contact_state()
        assert cs["passes"] == 2 * (k + 1)
        worst = max(worst, cs["depth_max"])                   # (the state holds the LAST pass of the step)
    print(f"second pass: device {worst:.6f}, NumPy loop {max(second):.6f} (its first pass: {max(first):.6f})")
    assert 0 < worst <= bar


def dropped_box(pkg, fp64, rot, steps, **kw):
    p = pkg.default_params(4, 1000.0)
    d = dict(mass=100.0, inertia=(1e5, 1.5e5, 1.2e5), rot=rot, centre=(500.0, 720.0, 500.0), velocity=(0.0, 300.0, 0.0))
    mu = kw.pop("mu", 0.0)
    d.update(kw)
    s = rig(pkg, fp64, free_body(**d), (box_phi(), BOX), FLOOR).set_collider_body_contact(restitution=0.0, friction=mu)
    return s, p, free_body(**d)


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_a_box_dropped_flat_does_not_turn(pkg, fp64):
    """By symmetry the arm is along the normal and the impulse has no torque; the NumPy loop gives |w| = 0 exactly.  The device
    folds the same terms in another order: the arm may be off by gamma_p sum|d r| / S <= 4 p eps a (a the largest half extent),
    which an impulse of at most m |v| turns into a change of w of at most m |v| 4 p eps a / I_min per pass."""
    s, p, ref = dropped_box(pkg, fp64, np.eye(3), 20)
    pts = s.collider_body_contact_points()
    c = BC.Contact(points=len(pts))
    BC.simulate(ref, c, pts, FLOOR, float(p.dt), 20)
    st = s.steps(p, 20).collider_body_state()
    cs = s.collider_body_contact_state()
    vmax = 300.0 + 20 * 4900.0 * float(p.dt)
    tol = cs["passes"] * 100.0 * vmax * 4 * len(pts) * EPS * max(BOX_HALF) / 1e5
    print(f"flat box: |w| = {np.linalg.norm(st['angular_velocity']):.3g} (NumPy loop {np.linalg.norm(ref.w):.3g}, bar {tol:.3g}), y = {st['centre'][1]:.3f}")
    assert cs["contacts"] > 5 and np.linalg.norm(st["angular_velocity"]) <= np.linalg.norm(ref.w) + tol
    assert abs(st["centre"][1] + BOX_HALF[1] - FLOOR_Y) <= BOX["spacing"]


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_a_box_dropped_on_a_corner_turns_the_way_of_r_cross_n(pkg, fp64):
    s, p, _ = dropped_box(pkg, fp64, PR.rotation((1.0, 0.2, 0.7), 0.6), 20)
    for k in range(20):
        cs = s.step(p).collider_body_contact_state()
        if cs["contacts"]:
            break
    st = s.collider_body_state()
    r, n = cs["arm"] / cs["depth_sum"], cs["push"] / np.linalg.norm(cs["push"])
    axis = np.cross(r, n)
    print(f"first contact in step {k}: r x n = {axis}, w = {st['angular_velocity']}")
    assert cs["contacts"] == 1 and np.linalg.norm(axis) > 1.0 and float(st["angular_velocity"] @ axis) > 0
    assert n[1] < -0.9                                        # (the floor pushes up)


def test_friction_slows_a_sliding_box(pkg):
    speeds = {}
    for mu in (0.0, 0.5):
        s, p, _ = dropped_box(pkg, False, np.eye(3), 20, centre=(500.0, 757.0, 500.0), velocity=(400.0, 0.0, 0.0), mu=mu)
        st = s.steps(p, 20).collider_body_state()
        assert s.collider_body_contact_state()["contacts"] > 10
        speeds[mu] = float(st["velocity"][0])
    print(f"v_x after 20 steps: {speeds}")
    assert speeds[0.0] == 400.0 and 0 <= speeds[0.5] < 200.0  # (the floor's normal has no x component: without friction v_x is untouched)


WALL_X, WALL_H = 690.0, 20.0


def test_a_floating_ball_stops_at_the_wall(pkg, settled):
    """the settled tank of test_collider_body_gpu; the scenery is a wall just inside the box's (the resting fluid does not
    reach it), on a lattice of spacing 20.  A ball afloat, given a velocity towards the wall, ends with its centre on the near
    side of wall - radius + one spacing; without contact it ends beyond."""
    p = pkg.default_params(4, TANK_SIDE)
    dims = (41, 41, 41)
    wall = (CR.lattice_of(lambda x: CR.plane_phi((-1.0, 0.0, 0.0), -WALL_X, x), (-40.0,) * 3, WALL_H, dims), (-40.0,) * 3, WALL_H)
    ends = {}
    for on in (False, True):
        body = free_body(mass=3.0 * DISPLACED, inertia=(0.4 * 3.0 * DISPLACED * RADIUS ** 2,) * 3, centre=(520.0, TANK_TOP, 351.0),
                         velocity=(1200.0, 0.0, 0.0), centre_min=(-np.inf, RADIUS, RADIUS), centre_max=(np.inf, TANK_SIDE - RADIUS, TANK_SIDE - RADIUS))
        s = rig(pkg, False, body, (ball_phi(), BALL), wall, sc=settled)
        if on:
            s.set_collider_body_contact(restitution=0.0, iterations=2)
        worst = 0.0
        for _ in range(30):
            worst = max(worst, s.step(p).collider_body_state()["centre"][0])
        ends[on] = (s.collider_body_state()["centre"][0], worst)
        if on:
            assert s.collider_body_contact_state()["contacts"] > 0
    print(f"centre x (end, largest): without contact {ends[False]}, with {ends[True]}; the wall is at {WALL_X}")
    assert ends[False][0] > WALL_X - RADIUS + WALL_H
    assert ends[True][0] <= WALL_X - RADIUS + WALL_H and ends[True][1] <= WALL_X - RADIUS + WALL_H


# ---- 7. refusals and lifetimes ---------------------------------------------------------------------------------------------------------
def test_refusals_and_lifetimes(pkg):
    from pbf_sph_amd import capi
    p = pkg.default_params(4, 1000.0)
    good = capi.BodyContact(0.0, 1, 6.0, 0.3, 0.0, 0.3, 0.5, 1)
    state = lambda s: s.L.pbf_collider_body_contact_state(s.ctx, C.byref(capi.BodyContactState()))
    n64 = C.c_uint64(0)
    # needs a body and scenery
    s = solver(pkg, False).upload(**far_particles())
    L = s.L
    assert L.pbf_set_collider_body_contact(s.ctx, C.byref(good)) == ERR_STATE and b"no body" in L.pbf_last_error(s.ctx)
    s.set_collider(ball_phi(), BALL["origin"], BALL["spacing"], 0.0)
    assert L.pbf_set_collider_body_contact(s.ctx, C.byref(good)) == ERR_STATE and b"no body" in L.pbf_last_error(s.ctx)
    s.set_collider_body(**bouncing().kwargs())
    assert L.pbf_set_collider_body_contact(s.ctx, C.byref(good)) == ERR_STATE and b"no scenery" in L.pbf_last_error(s.ctx)
    assert state(s) == ERR_STATE and L.pbf_collider_body_contact_points(s.ctx, C.byref(n64), None) == ERR_STATE
    assert L.pbf_set_collider_body_contact(s.ctx, None) == 0                  # (off while off)
    s.set_scenery(*FLOOR, 0.0)
    assert L.pbf_set_collider_body_contact(s.ctx, C.byref(good)) == 0
    s.steps(p, 4)
    before, pts = everything(s), s.collider_body_contact_points().tobytes()
    assert s.collider_body_contact_state()["passes"] == 4
    # every PBF_ERR_INVALID leaves bytes and state unchanged
    bad = dict(level=np.nan, skin=np.inf, restitution=np.nan, friction=np.inf, correction=np.nan, slop=np.inf)
    bad_range = dict(stride=0, skin=-1.0, restitution=1.5, friction=-0.1, correction=-0.5, slop=-1.0, iterations=0)
    for k, v in list(bad.items()) + list(bad_range.items()) + [("restitution", -0.1), ("correction", 1.5), ("iterations", 9), ("level", 500.0)]:
        c = capi.BodyContact(0.0, 1, 6.0, 0.3, 0.0, 0.3, 0.5, 1)
        setattr(c, k, v)
        assert L.pbf_set_collider_body_contact(s.ctx, C.byref(c)) == ERR_INVALID, (k, v)
        assert b"pbf_set_collider_body_contact" in L.pbf_last_error(s.ctx)
    assert L.pbf_collider_body_contact_state(s.ctx, None) == ERR_INVALID and L.pbf_collider_body_contact_points(s.ctx, None, None) == ERR_INVALID
    assert not differing(everything(s), before) and s.collider_body_contact_points().tobytes() == pts
    twin = rig(pkg, False, bouncing(), (ball_phi(), BALL), FLOOR).set_collider_body_contact(**CHAIN).steps(p, 5)
    assert not differing(everything(s.step(p)), everything(twin))
    # a re-placed body keeps contact and its points and zeroes the counters
    s.set_collider_body(**bouncing().kwargs())
    cs = s.collider_body_contact_state()
    assert (cs["passes"], cs["contacts"], cs["rejected"]) == (0, 0, 0) and cs["points"] == len(pts) // 12
    assert s.collider_body_contact_points().tobytes() == pts
    s.steps(p, 5)
    assert body_bytes(s) == body_bytes(twin) and contact_bytes(s) == contact_bytes(twin)
    # a replaced scenery keeps it on
    s.set_scenery(floor_phi(790.0), SCENE["origin"], SCENE["spacing"], 0.0)
    assert state(s) == 0 and s.collider_body_contact_points().tobytes() == pts
    # cleared scenery, a cleared body and a replaced collider each turn it off
    s.set_scenery(None)
    assert state(s) == ERR_STATE and L.pbf_collider_body_contact_points(s.ctx, C.byref(n64), None) == ERR_STATE
    s.set_scenery(*FLOOR, 0.0).set_collider_body_contact(**CHAIN)
    assert state(s) == 0
    s.set_collider_body(None)
    assert state(s) == ERR_STATE
    s.set_collider_body(**bouncing().kwargs()).set_collider_body_contact(**CHAIN)
    s.set_collider(ball_phi(), BALL["origin"], BALL["spacing"], 0.0)
    assert state(s) == ERR_STATE
    s.set_collider_body(**bouncing().kwargs()).set_collider_body_contact(**CHAIN)
    s.set_collider(None)
    assert state(s) == ERR_STATE
    s.step(p)                                                 # (and the ctx still steps)
    # slab mode
    u = rig(pkg, False, bouncing(), (ball_phi(), BALL), FLOOR)
    u.set_collider(None).set_scenery(None)
    cut = capi.SlabCut(0, 12, 0, 0)
    assert L.pbf_slab_configure(u.ctx, C.byref(cut), 0, 0) == 0
    assert L.pbf_set_collider_body_contact(u.ctx, C.byref(good)) == ERR_STATE and b"slab" in L.pbf_last_error(u.ctx)
    assert L.pbf_set_collider_body_contact(u.ctx, None) == ERR_STATE
    s.close()
    u.close()


# ---- 8. the shim and the CLI --------------------------------------------------------------------------------------------------------------
def write_lattice(path, phi, origin, spacing, margin):
    with open(path, "wb") as f:
        f.write(np.array(phi.shape, np.uint32).tobytes() + np.array(origin, np.float64).tobytes() +
                np.array([spacing, margin], np.float64).tobytes() + np.ascontiguousarray(phi, np.float32).tobytes())


def test_shim(pkg, tmp_path):
    """host/test_body_contact_shim.cpp: Solver::setColliderBodyContact / colliderBodyContact / colliderBodyContactPoints through
    advance() — the same frames over the C ABI, bit for bit"""
    from pbf_sph_amd import capi
    frames = 6
    write_lattice(tmp_path / "ball.bin", ball_phi(), BALL["origin"], BALL["spacing"], 0.0)
    write_lattice(tmp_path / "floor.bin", FLOOR[0], FLOOR[1], FLOOR[2], 0.0)
    r = subprocess.run([os.path.join(PKG, "test_body_contact_shim"), str(tmp_path / "ball.bin"), str(tmp_path / "floor.bin"),
                        str(tmp_path / "dump.bin"), str(frames)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    raw = open(tmp_path / "dump.bin", "rb").read()
    n, npts = (int(v) for v in np.frombuffer(raw, np.uint64, 2))
    at = 16

    def take(dtype, shape):
        nonlocal at
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at).reshape(shape)
        at += a.nbytes
        return a

    def particles():
        return dict(id=take(np.uint64, (n,)), type=take(np.uint8, (n,)), mass=take(np.float32, (n,)), pos=take(np.float32, (n, 3)),
                    vel=take(np.float32, (n, 3)), colour=take(np.float32, (n, 4)))

    first, last = particles(), particles()
    pts = take(np.float32, (npts, 3))
    s = solver(pkg, False)
    s.set_collider(ball_phi(), BALL["origin"], BALL["spacing"], 0.0).set_scenery(*FLOOR, 0.0)
    # the body and the contact of the shim program
    s.set_collider_body(mass=46.0, inertia=(66240.0,) * 3, gain=0.49, accel=(0.0, 4900.0, 0.0), rot=np.eye(3), centre=(500.0, 728.0, 500.0),
                        velocity=(200.0, 300.0, -50.0), angular_velocity=(0.5, -0.3, 0.2))
    s.set_collider_body_contact(skin=6.0, restitution=0.3, friction=0.4, correction=0.3, slop=0.5, iterations=2)
    assert s.collider_body_contact_points().tobytes() == pts.tobytes()
    p = pkg.default_params(4, 1000.0)
    p.dt = float(np.float32(p.dt))
    st, bsize, csize = first, C.sizeof(capi.ColliderBodyState), C.sizeof(capi.BodyContactState)
    contacts = 0
    for k in range(frames):
        st = s.upload(**st).step(p).download()
        assert bytes(s.collider_body_state(raw=True)) == raw[at:at + bsize], k
        at += bsize
        assert contact_bytes(s) == raw[at:at + csize], k
        at += csize
        contacts = s.collider_body_contact_state()["contacts"]
    assert at == len(raw) and contacts > 0
    for k in last:
        assert st[k].tobytes() == last[k].tobytes(), k


def test_cli(pkg, tmp_path):
    """--collider-body-contact adds contact_points, contact_depth and contacts to the report line; without it the line has the
    keys it always had, and the flag without --collider-body or --scenery says what it needs"""
    exe = os.path.join(PKG, "benchmark")
    common = ["--scene", "cubes", "--particles", "2048", "--solver-iter", "4", "-n", "6", "-w", "0", "--resident", "--no-surface",
              "--collider=sphere:500,700,500,60", "--collider-body=40", "--collider-body-report"]
    scenery = "--scenery=plane:0,-1,0,-800,0,50"
    r = subprocess.run([exe, *common, scenery, "--collider-body-contact=0,0.3", "-o", str(tmp_path / "a")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l)["body"] for l in r.stdout.split("\n") if l.startswith('{"frame"')]
    assert len(lines) == 6 and all({"contact_points", "contact_depth", "contacts"} <= set(l) for l in lines)
    assert lines[0]["contact_points"] > 50 and "Collider body contact" in r.stdout and "mu 0.3" in r.stdout
    r = subprocess.run([exe, *common, scenery, "-o", str(tmp_path / "b")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = [l for l in r.stdout.split("\n") if l.startswith('{"frame"')]
    assert len(plain) == 6 and "Collider body contact" not in r.stdout
    for l in plain:                                           # byte for byte the format it always had: these keys in this order
        assert re.fullmatch(r'\{"frame":\d+,"body":\{"rot":\[[^\]]*\],"centre":\[[^\]]*\],"quat":\[[^\]]*\],"velocity":\[[^\]]*\],'
                            r'"angular_velocity":\[[^\]]*\],"impulse":\[[^\]]*\],"angular":\[[^\]]*\],"hits":\d+,"steps":\d+,"rejected":\d+\}\}', l), l
    r = subprocess.run([exe, *common, "--collider-body-contact", "-o", str(tmp_path / "c")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "needs --collider-body and --scenery" in r.stderr
    r = subprocess.run([exe, *common[:-2], scenery, "--collider-body-contact", "-o", str(tmp_path / "d")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "needs --collider-body and --scenery" in r.stderr
    r = subprocess.run([exe, *common, scenery, "--collider-body-contact=2", "-o", str(tmp_path / "e")], capture_output=True, text=True, timeout=300)
    assert "--collider-body-contact: restitution in [0, 1]" in r.stderr and "Benchmark completed" not in r.stdout
    h = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--collider-body-contact" in h
