"""NumPy restatement of the posed collider's device function (collider_project_posed, csrc/pbf_collider.hpp; the contract in
include/pbf_hip.h), operation for operation in arrays of dtype N, on top of tests/collider_ref.py: the static contract from u
to b' is collider_ref.project itself, run in the body frame with scale 1 and an unbounded box (x * 1, x / 1 and a clamp to
+-inf are exact).  Beside it: the pose check of csrc/pbf_collider_pose.hpp restated, the poses and the body-frame plane the
CPU and GPU tests share, and the mutations the CPU test must be able to tell from the contract."""
import numpy as np

import collider_ref as CR


def rotation(axis, angle):
    """Rodrigues, float64"""
    k = np.asarray(axis, np.float64)
    k = k / np.sqrt((k * k).sum())
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def pose_of(rot, trans, dtype):
    """(N(R), N(t)): what pbf_set_collider_pose keeps"""
    N = np.dtype(dtype).type
    return np.asarray(rot, np.float64).reshape(3, 3).astype(N), np.asarray(trans, np.float64).reshape(3).astype(N)


def _body_frame(N):
    inf = np.full(3, np.inf).astype(N)
    return N(1), -inf, inf


def project(lat, fr, pose, q, mutation=None):
    """q (n,3) of dtype N -> (phi (n,), q' (n,3), hit (n,) bool), as collider_ref.project.  mutation: None = the contract;
    "transposed" (R and R^T swapped), "gradient" (the push applied in the world frame without rotating it back) or
    "t_first" (t added before the rotation) = what the tests must tell from it."""
    N = lat.N
    scale, minB, maxB = fr
    R, t = pose
    q = np.asarray(q)
    assert q.dtype == N and R.dtype == N and t.dtype == N
    if mutation == "transposed":
        R = np.ascontiguousarray(R.T)
    with np.errstate(all="ignore"):
        w = [q[:, a] * scale for a in range(3)]
        d = [w[a] - t[a] for a in range(3)]
        b = np.stack([(R[0][a] * d[0] + R[1][a] * d[1]) + R[2][a] * d[2] for a in range(3)], axis=1)
        phi, bp, hit = CR.project(lat, _body_frame(N), b)          # b' = b + s * g where hit, b elsewhere
        if mutation == "gradient":
            wp = [w[a] + (bp[:, a] - b[:, a]) for a in range(3)]
        elif mutation == "t_first":
            c = [bp[:, a] + t[a] for a in range(3)]
            wp = [(R[a][0] * c[0] + R[a][1] * c[1]) + R[a][2] * c[2] for a in range(3)]
        else:
            wp = [((R[a][0] * bp[:, 0] + R[a][1] * bp[:, 1]) + R[a][2] * bp[:, 2]) + t[a] for a in range(3)]
        out = np.empty_like(q)
        for a in range(3):
            moved = np.fmin(maxB[a] / scale, np.fmax(minB[a] / scale, wp[a] / scale))
            out[:, a] = np.where(hit, moved, q[:, a])
    assert phi.dtype == N and out.dtype == N
    return phi, out, hit


def sample(lat, fr, pose, points):
    """pbf_collider_sample under a pose: world points (float64) -> round to N, q = point / scale in N, then project()"""
    with np.errstate(all="ignore"):
        q = np.asarray(points, np.float64).reshape(-1, 3).astype(lat.N) / fr[0]
    return project(lat, fr, pose, q)


# ---- the reaction records (DeltaOp<.., COLLIDE_REACT>::end, csrc/pbf_kernels.hpp) -------------------------------------------
def react(fr, pose, q, moved, hit, rec=None):
    """one delta-p launch's update of the records rec (n,8) of dtype N = {A.xyz, hits, B.xyz, 0} (None: the cleared records),
    in N in the order of the contract: delta_a = (q'_a - q_a) * scale, r_a = q'_a * scale - t_a, A_a += delta_a, hits += 1,
    B_x += r_y * delta_z - r_z * delta_y (y, z cyclic).  A particle that does not hit keeps its record's bits.  -> new rec"""
    N = q.dtype.type
    scale, t = fr[0], pose[1]
    rec = np.zeros((len(q), 8), N) if rec is None else rec.copy()
    with np.errstate(all="ignore"):
        d = [(moved[:, a] - q[:, a]) * scale for a in range(3)]
        r = [moved[:, a] * scale - t[a] for a in range(3)]
        new = rec.copy()
        for a in range(3):
            new[:, a] = rec[:, a] + d[a]
        new[:, 3] = rec[:, 3] + N(1)
        for a in range(3):
            y, z = (a + 1) % 3, (a + 2) % 3
            new[:, 4 + a] = rec[:, 4 + a] + (r[y] * d[z] - r[z] * d[y])
    rec[hit] = new[hit]
    assert rec.dtype == N
    return rec


# ---- the pose check (csrc/pbf_collider_pose.hpp), float64 in the order written -------------------------------------------
ORTHO_BOUND = 1e-5


def pose_ok(rot, trans):
    r = np.asarray(rot, np.float64).reshape(9)
    if not (np.isfinite(r).all() and np.isfinite(np.asarray(trans, np.float64)).all()):
        return False
    with np.errstate(all="ignore"):
        worst = 0.0
        for a in range(3):
            for b in range(3):
                v = (r[a] * r[b] + r[3 + a] * r[3 + b]) + r[6 + a] * r[6 + b]
                worst = max(worst, abs(v - (1.0 if a == b else 0.0)))
        det = (r[0] * (r[4] * r[8] - r[5] * r[7]) - r[1] * (r[3] * r[8] - r[5] * r[6])) + r[2] * (r[3] * r[7] - r[4] * r[6])
    return bool(worst <= ORTHO_BOUND and not det < 0)


# ---- the cases the CPU and GPU tests share --------------------------------------------------------------------------------
IDENTITY = (np.eye(3), np.zeros(3))
# (no translation: R b is then exact for every b, so a lattice's edge points stay ON its edges in the world frame)
QUARTER_Z = (np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), np.zeros(3))
GENERIC = (rotation((0.3, -0.5, 0.8), 0.7), np.array([120.0, -40.0, 65.0]))
POSES = {"identity": IDENTITY, "quarter-z": QUARTER_Z, "generic": GENERIC}

# the world plane n.w = d, sampled in the body frame of a pose on a lattice that covers the whole box under that pose:
# 37^3 nodes at spacing 50 (1800 a side; the box's diagonal is 1733) centred on the body image of the box's centre
WORLD_N, WORLD_D = CR.PLANE_N, -400.0
BODY_DIMS, BODY_SPACING = (37, 37, 37), 50.0
POSE_UNIT = 1600.0                              # as collider_ref.PLANE_UNIT: largest |coordinate| + |d|
# worst |n.w' - d - margin| / (eps_N * POSE_UNIT) over the hit particles that end on no face, measured with project() under
# GENERIC on 2e5 random points of the box (seed 1, tests/test_collider_pose_cpu.py).  The bar is 8 x that: the factor covers
# other seeds and poses, not the code under test.
POSE_WORST = {"float32": 1.391, "float64": 1.44}


def pose_bar_units(dtype):
    return 8.0 * POSE_WORST[np.dtype(dtype).name]


def pose_bar_world(dtype):
    return pose_bar_units(dtype) * float(np.finfo(dtype).eps) * POSE_UNIT


def body_plane(pose64, normal=WORLD_N, d=WORLD_D):
    """the world plane n.w = d in the body frame of the float64 pose (R, t): n_b = R^T n, d_b = d - n.t -> (n_b, d_b)"""
    R, t = pose64
    n = np.asarray(normal, np.float64)
    n = n / np.sqrt((n * n).sum())
    return R.T @ n, float(d) - float(n @ t)


def body_plane_case(pose64, dtype, normal=WORLD_N, d=WORLD_D, margin=CR.MARGIN, dims=BODY_DIMS, spacing=BODY_SPACING):
    """-> (Lattice of that plane in the body frame, float64 nodes, origin, frame of the stock box at scale 500)"""
    R, t = pose64
    nb, db = body_plane(pose64, normal, d)
    centre = R.T @ (np.array([500.0, 500.0, 500.0]) - t)
    origin = np.round(centre - 0.5 * spacing * (np.asarray(dims) - 1))
    phi = CR.lattice_of(lambda x: x @ nb - db, origin, spacing, dims)
    return CR.Lattice(phi, origin, spacing, margin, dtype), phi, origin, CR.frame(CR.SCALE, CR.BOX[0], CR.BOX[1], dtype)


# the pushing scene: collider_ref.block_scene (an 8^3 block at rest in mid-box) and a plane lattice with BODY normal +x (solid
# on the -x side) under a fixed rotation, carried along its world normal R e_x by a third of the particle spacing per step.
# The normal points against gravity (+y), so the block also settles onto the plane.  It starts 5 world units short of the block.
PUSH_R = rotation((0.5, 0.1, 1.0), -1.3)
PUSH_T0 = np.array([35.0, -60.0, 20.0])
PUSH_STEPS, PUSH_ADVANCE = 20, 27.0 / 3.0


def push_plane_d(step):
    """the plane stands at n_w . w = d in the step numbered `step` (from 0), n_w = PUSH_R e_x"""
    n_w = PUSH_R[:, 0]
    lo = float((CR.block_scene()["pos"] @ n_w).min())
    return lo - CR.MARGIN - 5.0 + PUSH_ADVANCE * step


def push_pose(step):
    return PUSH_R, PUSH_T0 + PUSH_ADVANCE * step * PUSH_R[:, 0]


def push_case(dtype):
    """-> (Lattice of the body plane b_x = c, float64 nodes, origin, frame): 37^3 nodes at spacing 50 centred on the body image
    of the block's centre at step 0"""
    n_w = PUSH_R[:, 0]
    c = push_plane_d(0) - float(n_w @ PUSH_T0)
    centre = PUSH_R.T @ (CR.block_scene()["pos"].mean(axis=0) - PUSH_T0)
    origin = np.round(centre - 0.5 * BODY_SPACING * (np.asarray(BODY_DIMS) - 1))
    phi = CR.lattice_of(lambda x: x[..., 0] - c, origin, BODY_SPACING, BODY_DIMS)
    return CR.Lattice(phi, origin, BODY_SPACING, CR.MARGIN, dtype), phi, origin, CR.frame(CR.SCALE, CR.BOX[0], CR.BOX[1], dtype)
