"""NumPy restatement of a delta-p epilogue with a collider AND scenery (DeltaOp<.., COLLIDE_REACT_SCENERY>::end,
csrc/pbf_kernels.hpp; the contract in include/pbf_hip.h): the posed contract on q with the collider's lattice, the reaction
record from (q, q1), then the static contract on q1 with the scenery's lattice — three calls into the restatements the collider
is already held to (tests/collider_ref.py, tests/collider_pose_ref.py) and nothing else.  Beside it: the cases the CPU and GPU
tests share."""
import numpy as np

import collider_pose_ref as PR
import collider_ref as CR


def project_both(lat_c, pose, lat_s, fr, q, rec=None):
    """q (n,3) of dtype N, the solver-frame position after the box clamp -> (q2 (n,3), hit_c (n,), hit_s (n,), rec (n,8)).
    The records describe the collider's push alone, with r taken at q1; the scenery writes none."""
    _, q1, hit_c = PR.project(lat_c, fr, pose, q)
    rec = PR.react(fr, pose, q, q1, hit_c, rec)
    _, q2, hit_s = CR.project(lat_s, fr, q1)
    return q2, hit_c, hit_s, rec


def never_hit(dims, origin, spacing, dtype, margin=CR.MARGIN):
    """a lattice of +inf everywhere: legal ("no solid anywhere near"), inside it phi is inf or NaN and nothing ever hits"""
    return CR.Lattice(np.full(dims, np.inf), origin, spacing, margin, dtype)


# ---- the wedge: the tilted plane of collider_ref as scenery, and a ball above it that presses particles towards it -----------
# The ball's centre stands 150 world units on the fluid side of the plane and its radius is 170, so the cap of the ball below
# phi_plane = margin is where both solids claim a particle: the ball pushes it out radially, which near the cap's rim is
# TOWARDS the plane, and the plane, coming last, has the final word.
WEDGE_DIMS, WEDGE_SPACING, WEDGE_ORIGIN = (45, 45, 45), 25.0, (-50.0, -50.0, -50.0)    # the box plus two spacings
WEDGE_PLANE_D = -600.0
WEDGE_BALL_R = 170.0


def wedge_centre():
    n = np.asarray(CR.PLANE_N, np.float64)
    n = n / np.sqrt((n * n).sum())
    foot = np.array([500.0, 0.0, 500.0])
    foot[1] = (WEDGE_PLANE_D - n[0] * foot[0] - n[2] * foot[2]) / n[1]          # on the plane, mid-box in x and z
    return foot + 150.0 * n


def wedge_case(dtype):
    """-> (Lattice of the plane, Lattice of the ball, identity pose in N, frame)"""
    c = wedge_centre()
    plane = CR.lattice_of(lambda x: CR.plane_phi(CR.PLANE_N, WEDGE_PLANE_D, x), WEDGE_ORIGIN, WEDGE_SPACING, WEDGE_DIMS)
    ball = CR.lattice_of(lambda x: CR.sphere_phi(c, WEDGE_BALL_R, x), WEDGE_ORIGIN, WEDGE_SPACING, WEDGE_DIMS)
    return (CR.Lattice(plane, WEDGE_ORIGIN, WEDGE_SPACING, CR.MARGIN, dtype), CR.Lattice(ball, WEDGE_ORIGIN, WEDGE_SPACING, CR.MARGIN, dtype),
            PR.pose_of(*PR.IDENTITY, dtype), CR.frame(CR.SCALE, CR.BOX[0], CR.BOX[1], dtype))


def wedge_points(dtype, n=200_000, seed=4):
    """q of dtype N: random points of the cube of side 2.4 r about the ball's centre (it holds the whole ball and the cap)"""
    rng = np.random.default_rng(seed)
    w = wedge_centre() + (rng.random((n, 3)) - 0.5) * 2.4 * WEDGE_BALL_R
    return w.astype(dtype) / np.dtype(dtype).type(CR.SCALE)


# ---- the GPU stage test: two lattices that overlap, so that some particles hit both, some one and some none ------------------
def scenery_plane_through(sc, dtype, share=0.35, normal=(-0.3, -0.9, 0.2)):
    """a second tilted plane (another normal than the collider's) that `share` of the scene's fluid starts below, on the
    lattice over the box (collider_ref.BLOCK_LATTICE) -> (Lattice, float64 nodes)"""
    w = sc["pos"][sc["type"] == 0].astype(np.float64)
    d = float(np.quantile(CR.plane_phi(normal, 0.0, w), share)) - CR.MARGIN
    if len(w) == 1:
        d += 30.0                                             # a single particle starts inside the solid
    L = CR.BLOCK_LATTICE
    phi = CR.lattice_of(lambda x: CR.plane_phi(normal, d, x), L["origin"], L["spacing"], L["dims"])
    return CR.Lattice(phi, L["origin"], L["spacing"], CR.MARGIN, dtype), phi
