"""NumPy restatement of the collider friction (pbf_set_collider_friction, include/pbf_hip.h; k_collider_friction,
csrc/pbf_collider_friction.hpp), operation for operation in arrays of dtype N and in the order of the contract, on top of
tests/collider_pose_ref.py (the records it reads are collider_pose_ref.react's); the pass's sums in float64; and
colliderbody::kick (csrc/pbf_collider_body.hpp) on a tests/collider_body_ref.Body.  Beside them the mutations the CPU test
must be able to tell from the contract."""
import numpy as np

import collider_body_ref as BR

VD32 = np.float32(0.49)                       # csrc/pbf_common.hpp: a float constant, widened exactly for N = double
MUTATIONS = ("no_vb", "vb_unscaled", "len_unscaled", "not_normalised", "wxr_sign")


def friction(dtype, scale, dt, mu, V, W, t, vel, pos, A, mutation=None):
    """One pass.  scale, dt, mu: scalars; V, W, t: (3,) world; vel (n,3) solver frame, pos (n,3) world, A (n,4) = the records'
    {A.xyz, hits} — all rounded to N here as the kernel does (arrays must already be of dtype N).
    -> dict(vel (n,3) N: v', dv (n,3) N (0 where the particle did not slide), act, slide (n,) bool, r (n,3) N,
            un, s, jn (n,) N: the normal and tangential relative speed BEFORE the pass and the Coulomb bound)"""
    N = np.dtype(dtype).type
    vel, pos, A = np.asarray(vel), np.asarray(pos), np.asarray(A)
    assert vel.dtype == N and pos.dtype == N and A.dtype == N
    scale, dt, mu = N(scale), N(dt), N(mu)
    V, W, t = (np.asarray(x, np.float64).reshape(3).astype(N) for x in (V, W, t))
    one = N(1)
    with np.errstate(all="ignore"):
        len_ = np.sqrt((A[:, 0] * A[:, 0] + A[:, 1] * A[:, 1]) + A[:, 2] * A[:, 2])
        act = (A[:, 3] > 0) & (len_ > 0)
        n = [A[:, a] / len_ for a in range(3)]
        if mutation == "not_normalised":
            n = [A[:, a] for a in range(3)]
        r = [pos[:, a] - t[a] for a in range(3)]
        c = [W[(a + 1) % 3] * r[(a + 2) % 3] - W[(a + 2) % 3] * r[(a + 1) % 3] for a in range(3)]
        if mutation == "wxr_sign":
            c = [-x for x in c]
        vb = [(V[a] + c[a]) / scale for a in range(3)]
        if mutation == "vb_unscaled":
            vb = [V[a] + c[a] for a in range(3)]
        if mutation == "no_vb":
            vb = [np.zeros(len(vel), N) for a in range(3)]
        u = [vel[:, a] - vb[a] for a in range(3)]
        un = (u[0] * n[0] + u[1] * n[1]) + u[2] * n[2]
        ut = [u[a] - un * n[a] for a in range(3)]
        s = np.sqrt((ut[0] * ut[0] + ut[1] * ut[1]) + ut[2] * ut[2])
        slide = act & (s > 0)
        jn = (N(VD32) * (len_ / scale)) / dt
        if mutation == "len_unscaled":
            jn = (N(VD32) * len_) / dt
        g = (mu * jn) / s
        f = np.where(g < one, g, one)
        dv = np.stack([-(f * ut[a]) for a in range(3)], axis=1)
        out = np.where(slide[:, None], vel + dv, vel)
        dv = np.where(slide[:, None], dv, N(0))
    assert out.dtype == N and dv.dtype == N
    return dict(vel=out, dv=dv, act=act, slide=slide, r=np.stack(r, axis=1), un=un, s=s, jn=jn, vb=np.stack(vb, axis=1), n=np.stack(n, axis=1))


def terms(mass, scale, res):
    """the per-particle terms of the sum in float64, (n, 6): p = m * (double(dv) * double(scale)), r x p — zero rows where the
    particle did not slide"""
    dtype = res["dv"].dtype.type
    m = np.asarray(mass).astype(np.float64)
    sc = np.float64(dtype(scale))
    p = m[:, None] * (res["dv"].astype(np.float64) * sc)
    r = res["r"].astype(np.float64)
    L = np.stack([r[:, 1] * p[:, 2] - r[:, 2] * p[:, 1], r[:, 2] * p[:, 0] - r[:, 0] * p[:, 2], r[:, 0] * p[:, 1] - r[:, 1] * p[:, 0]], axis=1)
    out = np.concatenate([p, L], axis=1)
    out[~res["slide"]] = 0.0
    return out


def kick(body, P, L):
    """colliderbody::kick on a collider_body_ref.Body, float64 in the order written -> body"""
    F = np.float64
    P, L = [F(v) for v in P], [F(v) for v in L]
    if not np.isfinite(P + L).all():
        body.rejected += 1
        return body
    R = BR.rotation_of(body.q)
    v, w = body.v, body.w
    with np.errstate(all="ignore"):
        for a in range(3):
            v[a] = v[a] + (-P[a] / body.mass) * body.linear_factor[a]
        k = [((R[b] * (-L[0]) + R[3 + b] * (-L[1])) + R[6 + b] * (-L[2])) / body.inertia[b] for b in range(3)]
        for a in range(3):
            w[a] = w[a] + ((R[3 * a] * k[0] + R[3 * a + 1] * k[1]) + R[3 * a + 2] * k[2]) * body.angular_factor[a]
    return body


# ---- the random contacts the CPU test measures on --------------------------------------------------------------------------
SCALE, DT = 500.0, float(np.float32(0.0083))
V, W, T = np.array([60.0, -35.0, 80.0]), np.array([0.3, -0.8, 0.5]), np.array([420.0, 310.0, 555.0])
SPEED_UNIT = 8.0                              # above every |relative velocity| of contacts(): |v| <= 3, |vb| <= 1.5 per axis
# worst of |un' - un|, |s' - max(0, s - mu jn)| and max(0, s' - s) in eps_N * SPEED_UNIT over the acting contacts, measured
# with friction() against its own float64 evaluation on contacts(seed 1), mu = 1 (tests/test_collider_friction_cpu.py).
# The bar is 8 x that: the factor covers other seeds, not the code under test.
FRICTION_WORST = {"float32": 1.299, "float64": 1.264}


def bar_units(dtype):
    return 8.0 * FRICTION_WORST[np.dtype(dtype).name]


def bar_speed(dtype):
    """the bar as a solver-frame speed"""
    return bar_units(dtype) * float(np.finfo(dtype).eps) * SPEED_UNIT


def contacts(dtype, seed, n=200000):
    """n random contacts in the stock box at scale 500: positions in the box, solver-frame velocities in [-3, 3], records with a
    random normal, a summed push of 0.05 to 40 world units (jn up to 4.7: both branches of the min occur) and 1 to 4 hits"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 1000.0, (n, 3)).astype(dtype)
    vel = rng.uniform(-3.0, 3.0, (n, 3)).astype(dtype)
    d = rng.normal(size=(n, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    A = np.concatenate([d * np.exp(rng.uniform(np.log(0.05), np.log(40.0), n))[:, None], rng.integers(1, 5, n)[:, None]], axis=1).astype(dtype)
    return dict(pos=pos, vel=vel, A=A)


def args_ok(mu=0.5, velocity=(0.0,) * 3, angular_velocity=(0.0,) * 3):
    """the check of pbf_set_collider_friction restated -> None when accepted, else the reason's key words"""
    if not mu > 0:
        return "mu <= 0 or NaN"
    if not np.isfinite(np.concatenate([np.asarray(velocity, np.float64), np.asarray(angular_velocity, np.float64)])).all():
        return "non-finite velocity"
    return None
