"""The posed collider on the CPU: tests/collider_pose_ref.py — the NumPy restatement the device is held to bit for bit
(tests/test_collider_pose_gpu.py) — against the static restatement (identity pose), a float64 closed form (a generic pose),
three mutations it must be told from, the pose check, and the stand-alone host program of csrc/pbf_collider_pose.hpp."""
import os
import subprocess

import numpy as np
import pytest

import collider_pose_ref as PR
import collider_ref as CR
import nversion as NV

DTYPES = [np.float32, np.float64]
IDS = ["fp32", "fp64"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    return a.tobytes() == b.tobytes()


# ---- identity pose == the static function --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_identity_pose_is_the_static_function_on_the_plane(dtype):
    lat, fr = CR.plane_case(dtype)
    q = (np.random.default_rng(1).random((200_000, 3)) * 1000.0).astype(dtype) / fr[0]
    want = CR.project(lat, fr, q)
    got = PR.project(lat, fr, PR.pose_of(*PR.IDENTITY, dtype), q)
    assert 0.03 < want[2].mean() < 0.3
    assert np.array_equal(got[2], want[2]) and same_bits(got[0], want[0]) and same_bits(got[1], want[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dims", [(2, 2, 2), (3, 5, 4), (23, 19, 27)])
def test_identity_pose_is_the_static_function_on_the_edge_points(dtype, dims):
    """first / last / before / beyond on every axis, the corner, NaN, +-inf and a mixed point, and random ones"""
    lat, fr, pts, names = CR.edge_case(dims, dtype, n_random=4000)
    want = CR.sample(lat, fr, pts)
    got = PR.sample(lat, fr, PR.pose_of(*PR.IDENTITY, dtype), pts)
    assert want[2].any() and np.isinf(want[0]).any()
    assert np.array_equal(got[2], want[2]) and same_bits(got[0], want[0]) and same_bits(got[1], want[1])


# ---- a generic pose against the closed form ------------------------------------------------------------------------------
def pose_errors(dtype, seed, pose64=PR.GENERIC, mutation=None, n=200_000):
    """-> (|n.w' - d - margin| of the hit particles that end on no box face in units of eps_N * POSE_UNIT, hit share)"""
    lat, _, _, fr = PR.body_plane_case(pose64, dtype)
    q = (np.random.default_rng(seed).random((n, 3)) * 1000.0).astype(dtype) / fr[0]
    phi, moved, hit = PR.project(lat, fr, PR.pose_of(*pose64, dtype), q, mutation)
    assert mutation or np.isfinite(phi).all()                         # the lattice covers the whole box under this pose
    assert same_bits(moved[~hit], q[~hit])                            # a select: bit for bit
    free = hit & ~CR.on_face(fr, moved)
    w = moved[free].astype(np.float64) * CR.SCALE
    err = np.abs(CR.plane_phi(PR.WORLD_N, PR.WORLD_D, w) - CR.MARGIN)
    if mutation is None:
        # the displacement is along the WORLD normal: its part across it carries the same roundings and stays below the
        # same bar (tests/test_collider_pose_gpu.py holds the summed impulse's direction to it)
        n = np.asarray(PR.WORLD_N) / np.linalg.norm(PR.WORLD_N)
        A = w - q[free].astype(np.float64) * CR.SCALE
        across = np.abs(A - np.outer(A @ n, n)).max() / (np.finfo(dtype).eps * PR.POSE_UNIT)
        assert across <= PR.pose_bar_units(dtype), across
    return err / (np.finfo(dtype).eps * PR.POSE_UNIT), hit.mean()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_generic_pose_lands_on_the_world_plane(dtype):
    """The lattice is the world plane n.w = -400 seen from the body frame, so a projected particle lands on phi = margin of
    the WORLD plane up to rounding.  The bar is 8 x the worst measured with this restatement on seed 1
    (collider_pose_ref.POSE_WORST); other seeds and another pose must stay below it."""
    worst = {}
    other = (PR.rotation((-0.6, 0.2, 0.5), 2.1), np.array([-75.0, 210.0, 33.0]))
    for seed, pose64 in ((1, PR.GENERIC), (2, PR.GENERIC), (3, PR.GENERIC), (4, other)):
        units, share = pose_errors(dtype, seed, pose64)
        assert 0.1 <= share <= 0.9, share                             # (of the restatement, before anything else)
        worst[seed] = units.max()
        print(f"{np.dtype(dtype).name} seed {seed}: worst {units.max():.3f} eps * {PR.POSE_UNIT:.0f}, hit {100 * share:.1f} %")
        assert len(units) > 1000 and units.max() <= PR.pose_bar_units(dtype)
    name = np.dtype(dtype).name
    assert abs(worst[1] - PR.POSE_WORST[name]) <= 0.01 * PR.POSE_WORST[name], worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mutation", ["transposed", "gradient", "t_first"])
def test_mutations_miss_the_plane_by_100_bars(dtype, mutation):
    units, share = pose_errors(dtype, 1, mutation=mutation, n=20_000)
    print(f"{np.dtype(dtype).name} {mutation}: worst {units.max():.3e} units, bar {PR.pose_bar_units(dtype):.2f}")
    assert len(units) > 100 and units.max() >= 100.0 * PR.pose_bar_units(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_phi_under_a_pose_follows_the_closed_form(dtype):
    lat, _, _, fr = PR.body_plane_case(PR.GENERIC, dtype)
    pts = np.random.default_rng(5).random((50_000, 3)) * 1000.0
    phi, _, hit = PR.sample(lat, fr, PR.pose_of(*PR.GENERIC, dtype), pts)
    true = CR.plane_phi(PR.WORLD_N, PR.WORLD_D, pts)
    tol = 64 * np.finfo(dtype).eps * PR.POSE_UNIT
    assert np.abs(phi - true).max() <= tol
    clear = np.abs(true - CR.MARGIN) > tol
    assert np.array_equal(hit[clear], (true < CR.MARGIN)[clear])


# ---- the reaction records -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_record_update_follows_the_closed_form(dtype):
    """a hit's record against float64: A = w' - w, B = (w' - t) x A; twice the same update is twice the record (+ 1 hit each);
    a particle that does not hit keeps a record of zeros"""
    lat, _, _, fr = PR.body_plane_case(PR.GENERIC, dtype)
    pose = PR.pose_of(*PR.GENERIC, dtype)
    q = (np.random.default_rng(9).random((20_000, 3)) * 1000.0).astype(dtype) / fr[0]
    _, moved, hit = PR.project(lat, fr, pose, q)
    rec = PR.react(fr, pose, q, moved, hit)
    assert not rec[~hit].any() and (rec[hit, 3] == 1).all() and not rec[:, 7].any()
    w, wp = q.astype(np.float64) * CR.SCALE, moved.astype(np.float64) * CR.SCALE
    A = wp - w
    B = np.cross(wp - PR.GENERIC[1], A)
    eps = float(np.finfo(dtype).eps)
    # delta: one subtraction of values <= 2 (q) and one product; B: two products of |r| <= 2600 by |delta| and their difference
    assert np.abs(rec[hit, :3] - A[hit]).max() <= 4 * eps * 1000.0
    assert np.abs(rec[hit, 4:7] - B[hit]).max() <= 8 * eps * 2600.0 * max(np.abs(A[hit]).max(), 1.0)
    twice = PR.react(fr, pose, q, moved, hit, rec)
    assert (twice[hit, 3] == 2).all() and np.array_equal(twice[hit, :3], rec[hit, :3] + rec[hit, :3]) and not twice[~hit].any()


# ---- the pose check ----------------------------------------------------------------------------------------------------
def float32_rotation():
    """three elementary rotations composed in float32: what a caller with a float pipeline hands over"""
    def rot(axis, a):
        c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
        m = np.eye(3, dtype=np.float32)
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
        return m
    return (rot(0, 0.4) @ rot(1, -1.1) @ rot(2, 2.3)).astype(np.float32)


def test_pose_check():
    assert PR.pose_ok(*PR.IDENTITY) and PR.pose_ok(*PR.QUARTER_Z) and PR.pose_ok(*PR.GENERIC)
    r32 = float32_rotation()
    err = np.abs(r32.astype(np.float64).T @ r32.astype(np.float64) - np.eye(3)).max()
    assert 0 < err < 1e-6 and PR.pose_ok(r32, (1.0, 2.0, 3.0))          # composed in float: passes with room to spare
    R, t = PR.GENERIC
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(9):
            m = R.copy().reshape(9)
            m[k] = bad
            assert not PR.pose_ok(m, t)
        for k in range(3):
            u = t.copy()
            u[k] = bad
            assert not PR.pose_ok(R, u)
    assert not PR.pose_ok(R * 1.00001, t)                             # R^T R - I = 2e-5
    assert PR.pose_ok(R * 1.000004, t)                                # 8e-6: inside the stated bound
    sheared = R.copy()
    sheared[0, 1] += 1e-4
    assert not PR.pose_ok(sheared, t)
    assert not PR.pose_ok(np.diag([1.0, 1.0, -1.0]), t)               # a reflection: orthogonal, det = -1
    assert not PR.pose_ok(R @ np.diag([-1.0, 1.0, 1.0]), t)
    assert not PR.pose_ok(np.zeros((3, 3)), t)
    assert not PR.pose_ok(np.full((3, 3), 1e200), t)


def test_pose_check_host_program():
    """csrc/pbf_collider_pose.hpp alone, as the program it is: plain, and built with the address and undefined-behaviour
    sanitizers (host code only; never loaded into Python)"""
    for name in ("test_collider_pose", "test_collider_pose_san"):
        exe = os.path.join(ROOT, "pbf-sph_amd", name)
        assert os.path.exists(exe), "build() makes it"
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        out = r.stdout + r.stderr
        assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, out
        assert "AddressSanitizer" not in out and "runtime error" not in out, out


# ---- the GPU pushing scene's preconditions, on a float64 all-pairs step --------------------------------------------------------
def test_pushing_scene_meets_its_preconditions():
    """the scene of test_collider_pose_gpu's pushing test under tests/nversion.py's stages (float64, all pairs), the posed
    collider applied after delta-p's clamp as DeltaOp::end does: no particle ever lies on a box face, the lattice covers the
    block all along, every particle ends each step on the fluid side within the bar, and the plane does push (most steps hit)"""
    sc = CR.block_scene()
    pos, vel, mass = sc["pos"].astype(np.float64), sc["vel"].astype(np.float64), sc["mass"].astype(np.float64)
    lat, _, _, fr = PR.push_case(np.float64)
    n_w = PR.PUSH_R[:, 0]
    bar = PR.pose_bar_world(np.float64)
    h, dt, lo, hi = 0.1, 0.0083 * np.float32(1.5), [0.0] * 3, [1000.0] * 3
    pushed = 0
    for step in range(PR.PUSH_STEPS):
        pose = PR.pose_of(*PR.push_pose(step), np.float64)
        vel, ps = NV.predict(pos, vel, mass, dt, CR.SCALE, (0.0, 9.8, 0.0))
        cells = NV.predict_cells(ps, h, CR.SCALE, lo)
        any_hit = False
        for _ in range(4):
            lam, _ = NV.lambdas(ps, mass, h, None, cells)
            ps, _ = NV.delta(ps, lam, h, CR.SCALE, lo, hi, None, cells)
            phi, ps, hit = PR.project(lat, fr, pose, ps)
            assert np.isfinite(phi).all()
            any_hit |= bool(hit.any())
        pos, vel = NV.finalise(ps, pos, vel, dt, CR.SCALE)
        pushed += any_hit
        assert not CR.on_face(fr, ps).any(), step
        true = (ps * CR.SCALE) @ n_w - PR.push_plane_d(step)
        assert true.min() >= CR.MARGIN - bar, (step, true.min() - CR.MARGIN)
    print(f"the plane pushed in {pushed} of {PR.PUSH_STEPS} steps; the block now spans {pos.min(axis=0)} - {pos.max(axis=0)}")
    assert pushed >= PR.PUSH_STEPS // 2
