"""NumPy restatement of the body's contact with the scenery (pbf_set_collider_body_contact, include/pbf_hip.h), written from the
text of csrc/pbf_body_contact.hpp's head and of the header, operation for operation and in the order written there:

  evaluate()  the static contract's trilinear code up to (inside, hit, s, g), in arrays of dtype N — the same operations as
              collider_ref.project (tests/test_body_contact_cpu.py holds the two together bit for bit)
  points()    the body's surface points from the collider's lattice, in N, in cell-index order
  terms()     the per-point terms of one detection pass: r, the in-contact mask, m and d in float64
  Contact     the parameters and the state; resolve() is one pass's response on a collider_body_ref.Body, every value a
              numpy.float64 scalar, so each operation rounds once, as the header's double arithmetic does without contraction
"""
import numpy as np

import collider_ref as CR

F = np.float64


def evaluate(lat, b):
    """lat: collider_ref.Lattice (its margin is the level or the skin); b (n, 3) of dtype N in the lattice's frame ->
    inside (n,) bool, hit (n,) bool, s (n,) N, g (n, 3) N, phi (n,) N; outside the lattice nothing is meaningful"""
    N = lat.N
    b = np.asarray(b)
    assert b.dtype == N and b.ndim == 2 and b.shape[1] == 3
    with np.errstate(all="ignore"):
        u = [(b[:, a] - lat.origin[a]) * lat.inv for a in range(3)]
        inside = np.ones(len(b), bool)
        for a in range(3):
            inside &= (u[a] >= N(0)) & (u[a] <= N(lat.dims[a] - 1))
        us = [np.where(inside, u[a], N(0)) for a in range(3)]
        i = [np.minimum(us[a].astype(np.int64), lat.dims[a] - 2) for a in range(3)]
        f = [us[a] - i[a].astype(N) for a in range(3)]
        c = [[[lat.phi[i[0] + x, i[1] + y, i[2] + z] for z in range(2)] for y in range(2)] for x in range(2)]
        d = [[c[x][y][1] - c[x][y][0] for y in range(2)] for x in range(2)]
        cz = [[c[x][y][0] + f[2] * d[x][y] for y in range(2)] for x in range(2)]
        e = [cz[x][1] - cz[x][0] for x in range(2)]
        cy = [cz[x][0] + f[1] * e[x] for x in range(2)]
        gx = cy[1] - cy[0]
        phi = cy[0] + f[0] * gx
        gy = e[0] + f[0] * (e[1] - e[0])
        t = [d[x][0] + f[1] * (d[x][1] - d[x][0]) for x in range(2)]
        gz = t[0] + f[0] * (t[1] - t[0])
        ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
        hit = inside & (phi < lat.margin) & (ln > N(0))
        s = (lat.margin - phi) / ln
    g = np.stack([gx, gy, gz], axis=1)
    assert s.dtype == N and g.dtype == N
    return inside, hit, s, g, phi


def points(phi, origin, spacing, level, stride, dtype):
    """the surface points of pbf_set_collider_body_contact -> (n, 3) of dtype N, body frame, cell-index order"""
    N = np.dtype(dtype).type
    lat = CR.Lattice(phi, origin, spacing, level, dtype)
    dims = lat.dims
    idx = [np.arange(0, dims[a] - 1, int(stride)) for a in range(3)]
    I = np.stack(np.meshgrid(*idx, indexing="ij"), axis=-1).reshape(-1, 3)       # (C order: (i * cells_y + j) * cells_z + k)
    nodes = np.stack([lat.phi[I[:, 0] + x, I[:, 1] + y, I[:, 2] + z] for x in range(2) for y in range(2) for z in range(2)], axis=1)
    ok = np.isfinite(nodes).all(axis=1) & (nodes < lat.margin).any(axis=1) & (nodes >= lat.margin).any(axis=1)
    I = I[ok]
    sp = N(spacing)
    with np.errstate(all="ignore"):
        b = np.stack([lat.origin[a] + (I[:, a].astype(N) + N(0.5)) * sp for a in range(3)], axis=1)
        inside, _, s, g, _ = evaluate(lat, b)
        ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        p = np.stack([b[:, a] + s * g[:, a] for a in range(3)], axis=1)
    keep = inside & (ln > N(0)) & np.isfinite(p).all(axis=1)
    assert p.dtype == N
    return np.ascontiguousarray(p[keep])


def terms(pts, rot, x, scenery, skin):
    """One detection pass.  pts (n, 3) N, body frame; rot (9,) or (3, 3) and x (3,): the body record's pose in float64;
    scenery: (phi, origin, spacing) of the scenery's lattice -> r (n, 3), contact (n,) bool, m (n, 3), d (n,), all float64 (m and d
    are meaningful where contact holds)"""
    N = pts.dtype.type
    lat = CR.Lattice(scenery[0], scenery[1], scenery[2], skin, pts.dtype)
    R = np.asarray(rot, F).reshape(3, 3)
    x = np.asarray(x, F).reshape(3)
    b = pts.astype(F)
    with np.errstate(all="ignore"):
        r = np.stack([(R[a, 0] * b[:, 0] + R[a, 1] * b[:, 1]) + R[a, 2] * b[:, 2] for a in range(3)], axis=1)
        w = np.stack([r[:, a] + x[a] for a in range(3)], axis=1).astype(N)
        inside, hit, s, g, _ = evaluate(lat, w)
        m = np.stack([s.astype(F) * g[:, a].astype(F) for a in range(3)], axis=1)
        d = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        contact = inside & hit & (d > 0) & np.isfinite(d)
    return r, contact, m, d


def cross(p, q):
    return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]


def dot(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


class Contact:
    """the parameters of a pbf_body_contact that reach the device record, and struct pbf_body_contact_state"""

    def __init__(self, skin=0.0, restitution=0.0, friction=0.0, correction=0.8, slop=0.0, points=0):
        self.skin, self.e, self.mu, self.beta, self.slop = F(skin), F(restitution), F(friction), F(correction), F(slop)
        self.points = int(points)
        self.depth_sum = self.depth_max = F(0.0)
        self.push, self.arm, self.impulse, self.shift = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)
        self.passes = self.contacts = self.rejected = 0
        self.branch = None                 # of the last pass's friction: None, "slide" or "stick"

    def _W(self, body, R, c):
        k = [((R[b] * c[0] + R[3 + b] * c[1]) + R[6 + b] * c[2]) / body.inertia[b] for b in range(3)]
        return [((R[3 * a] * k[0] + R[3 * a + 1] * k[1]) + R[3 * a + 2] * k[2]) * body.angular_factor[a] for a in range(3)]

    def resolve(self, body, S, M, A, D, count):
        """one pass: moves `body` (a collider_body_ref.Body: x, v, w; rot and q stay) and this state"""
        S, D = F(S), F(D)
        M, A = [F(v) for v in M], [F(v) for v in A]
        x, v, w = body.x, body.v, body.w
        R, Fl = [F(t) for t in body.rot], body.linear_factor
        zero, one = F(0.0), F(1.0)
        self.passes += 1
        self.depth_sum, self.depth_max = S, D
        self.push, self.arm = np.array(M, F), np.array(A, F)
        self.impulse, self.shift, self.branch = np.zeros(3), np.zeros(3), None
        if int(count) == 0:
            return self
        with np.errstate(all="ignore"):
            ln = np.sqrt((M[0] * M[0] + M[1] * M[1]) + M[2] * M[2])
            if not np.isfinite([S, D, ln] + M + A).all() or not ln > 0:
                self.rejected += 1
                return self
            n, r = [M[a] / ln for a in range(3)], [A[a] / S for a in range(3)]
            self.contacts += 1
            Wn = self._W(body, R, cross(r, n))
            kn = ((Fl[0] * n[0] * n[0] + Fl[1] * n[1] * n[1]) + Fl[2] * n[2] * n[2]) / body.mass + dot(n, cross(Wn, r))
            c = cross(w, r)
            u = [v[a] + c[a] for a in range(3)]
            un = dot(u, n)
            j, jt, t = zero, zero, [zero] * 3
            if un < 0 and kn > 0:
                j = -((one + self.e) * un) / kn
                for a in range(3):
                    v[a] = v[a] + ((j * n[a]) / body.mass) * Fl[a]
                    w[a] = w[a] + j * Wn[a]
            if self.mu > 0 and j > 0:
                c = cross(w, r)
                u = [v[a] + c[a] for a in range(3)]
                cn = dot(u, n)
                ut = [u[a] - cn * n[a] for a in range(3)]
                lt = np.sqrt((ut[0] * ut[0] + ut[1] * ut[1]) + ut[2] * ut[2])
                if lt > 0:
                    tt = [ut[a] / lt for a in range(3)]
                    Wt = self._W(body, R, cross(r, tt))
                    kt = ((Fl[0] * tt[0] * tt[0] + Fl[1] * tt[1] * tt[1]) + Fl[2] * tt[2] * tt[2]) / body.mass + dot(tt, cross(Wt, r))
                    if kt > 0:
                        stick, slide = lt / kt, self.mu * j
                        jt = slide if slide < stick else stick
                        self.branch = "slide" if slide < stick else "stick"
                        t = tt
                        for a in range(3):
                            v[a] = v[a] - ((jt * tt[a]) / body.mass) * Fl[a]
                            w[a] = w[a] - jt * Wt[a]
            self.impulse = np.array([j * n[a] - jt * t[a] for a in range(3)], F)
            over = D - self.slop
            sh = self.beta * (over if over > 0 else zero)
            for a in range(3):
                self.shift[a] = (sh * n[a]) * Fl[a]
                x[a] = x[a] + self.shift[a]
                if x[a] < body.centre_min[a]:
                    x[a], v[a] = body.centre_min[a], zero
                elif x[a] > body.centre_max[a]:
                    x[a], v[a] = body.centre_max[a], zero
        return self

    def state_words(self):
        """the 18 64-bit words of struct pbf_body_contact_state, as bytes"""
        f = np.concatenate([[self.depth_sum], self.push, self.arm, [self.depth_max], self.impulse, self.shift]).astype(F)
        return f.tobytes() + np.array([self.points, self.passes, self.contacts, self.rejected], np.uint64).tobytes()


def simulate(body, contact, pts, scenery, dt, steps, iterations=1, each=None):
    """The NumPy loop of a body the fluid does not touch: per step advance() with zero sums, then `iterations` passes of terms(),
    fold() and resolve().  each(step, pass, D, count) runs after every pass.  Moves body and contact."""
    for k in range(steps):
        body.advance(dt, np.zeros(3), np.zeros(3))
        for it in range(iterations):
            r, c, m, d = terms(pts, body.rot, body.x, scenery, contact.skin)
            S, M, A, D, count, _ = fold(r, c, m, d)
            contact.resolve(body, S, M, A, D, count)
            if each:
                each(k, it, D, count)
    return body, contact


def fold(r, contact, m, d):
    """math.fsum of the per-point terms -> (S, M (3,), A (3,), D, count) and the sums of |term| in the same layout (7,)"""
    import math
    k = contact
    S = math.fsum(d[k])
    M = [math.fsum(m[k, a]) for a in range(3)]
    A = [math.fsum(d[k] * r[k, a]) for a in range(3)]
    D = float(d[k].max()) if k.any() else 0.0
    absum = [S] + [math.fsum(np.abs(m[k, a])) for a in range(3)] + [math.fsum(np.abs(d[k] * r[k, a])) for a in range(3)]
    return S, np.array(M), np.array(A), D, int(k.sum()), np.array(absum)
