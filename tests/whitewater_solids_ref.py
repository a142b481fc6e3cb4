"""NumPy restatement of pbf_set_whitewater_solids' contract (include/pbf_hip.h) — TEST INFRASTRUCTURE.

Written from the header's text, operation for operation in arrays of dtype N: NumPy's +, -, *, / and sqrt on float32 /
float64 are the IEEE operations and nothing here is contracted, so equality with the device is exact
(tests/test_whitewater_solids_gpu.py).  It calls collider_ref.project, collider_pose_ref.project and whitewater_ref.advect and
shares nothing else with the library.

`mutation` names what the tests must tell from the contract: "scenery_first" (the scenery applied before the collider),
"r_at_q" (the arm r taken at q rather than q1), "no_vb" (the solid's velocity left out), "always" (the response applied when
un >= 0 as well).

The bars of the response's properties, in units of u = eps_N / 2 times the speed scale S = |v| + |vb| (every intermediate is
bounded by a small multiple of S; n is a unit vector up to 2.5u: three squares, two sums, a sqrt, a quotient per axis):
  u_a = v_a - vb_a                                    1 rounding                      |u_a| <= S
  un  = (u_x n_x + u_y n_y) + u_z n_z                 3 products, 2 sums, n's 2.5u:    |d un| <= (5 + 2.5 + 1) u sqrt(3) S -> 15u S
  ut_a = u_a - un * n_a                               1 product, 1 sum, n's 2.5u, d un: |d ut_a| <= (2 + 2.5 + 15) u S     -> 20u S
  v'_a = (vb_a + (1 - f) ut_a) - (e un) n_a           1 - f: 1; the products 2; e un: 1; times n: 1 + 2.5; two sums 2:     -> 10u S more
  relative normal velocity of v':  (v' - vb) . n      one more subtraction per axis and the dot product's 8.5u sqrt(3):
       = (1 - f) ut . n - e un (n . n);  ut . n carries 3 * 20u S (it is 0 exactly in the reals), n . n - 1 carries 5u
  NORMAL_UNITS  = 3 * (20 + 10 + 1) + 15 + 5 + 15  = 128     |rel_n(v') + e un| <= 128 u S
  TANGENT_UNITS = 20 + 10 + 1                      = 31      per axis: |(v' - vb)_a - ((1 - f) ut_a - e un n_a)| <= 31 u S
"""
import numpy as np

import collider_pose_ref as PR
import collider_ref as CR
import whitewater_ref as WR

MUTATIONS = ("scenery_first", "r_at_q", "no_vb", "always")
NORMAL_UNITS, TANGENT_UNITS = 128.0, 31.0


def bar_speed(dtype, units, speed):
    return units * float(np.finfo(dtype).eps) / 2 * speed


def respond(N, hit, d, vb, v, e, f, always=False):
    """response(d, vb) on v (n,3) of dtype N -> (v', dict(act, go, un, n, ut))"""
    with np.errstate(all="ignore"):
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        act = hit & (ln > N(0))
        n = d / ln[:, None]
        u = v - vb
        un = (u[:, 0] * n[:, 0] + u[:, 1] * n[:, 1]) + u[:, 2] * n[:, 2]
        ut = u - un[:, None] * n
        go = act if always else act & (un < N(0))
        omf = N(1) - f
        new = (vb + omf * ut) - (e * un)[:, None] * n
    assert new.dtype == N and un.dtype == N
    return np.where(go[:, None], new, v), dict(act=act, go=go, un=un, n=n, ut=ut)


def collide(dtype, fr, x, v, alive, nF, collider=None, pose=None, scenery=None, V=None, W=None, t=None, e=0.0, f=0.0, absorb=False,
            mutation=None):
    """One pass over what whitewater_ref.advect returned.  fr = collider_ref.frame(...); x (n,3) world, v (n,3) solver frame,
    both of dtype N; alive (n,) bool, nF (n,) int.  collider / scenery: collider_ref.Lattice or None; pose: (N(R), N(t)) when
    the collider is posed, else None; V, W: (3,) world, the solid's velocities (None: the solid has none: vb = 0); t: the pose
    record's trans (None: 0).  A particle that is dead on entry is skipped.
    -> dict(pos, vel, alive, hit1, hit2, absorbed, q, q1, q2, first=dict, second=dict)"""
    N = np.dtype(dtype).type
    scale, minB, maxB = fr
    x, v = np.asarray(x), np.asarray(v)
    assert x.dtype == N and v.dtype == N
    e, f = N(e), N(f)
    n = len(x)
    with np.errstate(all="ignore"):
        q = x / scale

        def first(q0):
            if collider is None:
                return q0, np.zeros(n, bool)
            _, q1, h = PR.project(collider, fr, pose, q0) if pose is not None else CR.project(collider, fr, q0)
            return q1, h

        def second(q0):
            if scenery is None:
                return q0, np.zeros(n, bool)
            _, q2, h = CR.project(scenery, fr, q0)
            return q2, h

        if mutation == "scenery_first":
            qs, hit2 = second(q)
            qc, hit1 = first(qs)
            q1, q2 = qc, qc          # (what the particle ends at)
            d1, d2 = qc - qs, qs - q
        else:
            q1, hit1 = first(q)
            q2, hit2 = second(q1)
            d1, d2 = q1 - q, q2 - q1
        hit1, hit2 = hit1 & alive, hit2 & alive
        if V is None or mutation == "no_vb":
            vb = np.zeros((n, 3), N)
        else:
            Vn, Wn = np.asarray(V, np.float64).astype(N), np.asarray(W, np.float64).astype(N)
            tn = np.zeros(3, N) if t is None else np.asarray(t).astype(N)
            at = q if mutation == "r_at_q" else q1
            r = at * scale - tn
            c = np.stack([Wn[1] * r[:, 2] - Wn[2] * r[:, 1], Wn[2] * r[:, 0] - Wn[0] * r[:, 2], Wn[0] * r[:, 1] - Wn[1] * r[:, 0]], 1)
            vb = (Vn + c) / scale
        assert vb.dtype == N
        always = mutation == "always"
        if mutation == "scenery_first":
            v1, b = respond(N, hit2, d2, np.zeros((n, 3), N), v, e, f, always)
            v2, a = respond(N, hit1, d1, vb, v1, e, f, always)
        else:
            v1, a = respond(N, hit1, d1, vb, v, e, f, always)
            v2, b = respond(N, hit2, d2, np.zeros((n, 3), N), v1, e, f, always)
        hit = hit1 | hit2
        xn = np.where(hit[:, None], np.fmin(maxB, np.fmax(minB, q2 * scale)), x)
        vn = np.where(hit[:, None], v2, v)
        absorbed = alive & hit & (np.asarray(nF) == 0) & bool(absorb)
    assert xn.dtype == N and vn.dtype == N
    return dict(pos=xn, vel=vn, alive=alive & ~absorbed, hit1=hit1, hit2=hit2, absorbed=absorbed, q=q, q1=q1, q2=q2, vb=vb, first=a,
                second=b)


def step(pool, sample, cfg, params, dtype, **solids):
    """whitewater_ref.advect, then collide() -> collide()'s dict + life, kind of the advection"""
    adv = WR.advect(pool, sample, cfg, params, dtype)
    fr = CR.frame(params.scale, list(params.min_bound), list(params.max_bound), dtype)
    out = collide(dtype, fr, adv["pos"], adv["vel"], adv["alive"], adv["nF"], **solids)
    out.update(life=adv["life"], kind=adv["kind"], advected=adv)
    return out


def counts(res):
    return dict(hit_collider=int(res["hit1"].sum()), hit_scenery=int(res["hit2"].sum()), absorbed=int(res["absorbed"].sum()))


def children(dtype, fr, x, collider=None, pose=None, scenery=None):
    """the two position contracts on the children's positions x (n,3) world -> (x', born_inside (n,) bool)"""
    n = len(x)
    z = np.zeros((n, 3), np.dtype(dtype))
    r = collide(dtype, fr, np.asarray(x), z, np.ones(n, bool), np.ones(n, np.int64), collider=collider, pose=pose, scenery=scenery)
    return r["pos"], r["hit1"] | r["hit2"]


def settings_ok(restitution=0.0, friction=0.0, reserved=0):
    """the check of pbf_set_whitewater_solids restated"""
    return bool(0 <= restitution <= 1) and bool(0 <= friction <= 1) and reserved == 0


# ---- the case the CPU and GPU tests share ----------------------------------------------------------------------------------
# scenery_ref.wedge_case: a ball (the collider) resting on a tilted plane (the scenery) in the stock box at scale 500.  The
# points: the cube about the ball (both solids, the wedge between them) and the rest of the box (mostly no hit).
def wedge_pool(dtype, n, seed=5):
    """-> x (n,3) world of dtype N, v (n,3) solver frame, nF (n,), alive (n,): a third in and around the solids"""
    import scenery_ref as SR
    rng = np.random.default_rng(seed)
    c = SR.wedge_centre()
    x = rng.random((n, 3)) * 1000.0
    k = n // 3
    x[:k] = c + (rng.random((k, 3)) - 0.5) * 2.4 * SR.WEDGE_BALL_R
    v = (rng.random((n, 3)) - 0.5) * 3.0
    nF = rng.integers(0, 3, n) * rng.integers(0, 12, n)
    return np.clip(x, 0.0, 1000.0).astype(dtype), v.astype(dtype), nF.astype(np.int64), rng.random(n) > 0.05


# A solid that covers the whole box and pushes out of it: phi = -50 - y on an axis-aligned lattice, the fluid side beyond the
# face y = 0.  At scale 512 (collider_ref.EDGE_SCALE: q * scale / scale is q exactly, and g_x = g_z = 0 exactly) a point ON
# that face is pushed out, the box clamp brings it back to where it was, and d = 0: hit && len == 0.
def cover_case(dtype, n=40, seed=6):
    """-> (Lattice, frame, x (n,3) world of dtype N: the first half on the face y = 0, the rest inside the box)"""
    dims, spacing, origin = (5, 5, 5), 300.0, (-100.0, -100.0, -100.0)
    lat = CR.Lattice(CR.lattice_of(lambda w: -50.0 - w[..., 1], origin, spacing, dims), origin, spacing, CR.MARGIN, dtype)
    fr = CR.frame(CR.EDGE_SCALE, CR.BOX[0], CR.BOX[1], dtype)
    x = np.random.default_rng(seed).integers(1, 999, (n, 3)).astype(np.float64)
    x[:n // 2, 1] = 0.0
    return lat, fr, x.astype(dtype)
