"""NumPy restatement of the mesh collider (pbf_mesh_records / pbf_sdf_from_mesh, include/pbf_hip.h), parametrised by dtype.

records() restates csrc/pbf_mesh_records.hpp in float64; field() restates the kernel's fold in `dtype`, one NumPy operation per
operation of the contract, in its order: every pair is tested (no cull), every candidate is computed and the result selected
with np.where.  The winding number (van Oosterom & Strackee 1983) is the independent check of the sign."""
import numpy as np

# |phi32 - phi64| over lattice A and the four shapes of tests/mesh_shapes.py, measured with this restatement: 1.39e-4 world
# units (ico2; box 7.7e-5, tetra 1.0e-4, torus 1.1e-4) = 1.2 * eps32 * 1000.  test_mesh_sdf_cpu holds the float32 field to 8x.
F32_WORST = 1.4e-4


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def info(vertices, triangles):
    """the counts, volume and box of pbf_mesh_info for a mesh whose indices are in range"""
    v, t = np.asarray(vertices, np.float64), np.asarray(triangles, np.int64)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    n = _cross(b - a, c - a)
    six = 0.0
    for x in _dot(a, _cross(b, c)):
        six = six + x
    uses = {}
    for k in range(len(t)):
        for s in range(3):
            f, g = int(t[k, s]), int(t[k, (s + 1) % 3])
            uses.setdefault((min(f, g), max(f, g)), []).append(f < g)
    return dict(n_edges=len(uses), boundary_edges=sum(len(u) == 1 for u in uses.values()),
                nonmanifold_edges=sum(len(u) > 2 for u in uses.values()),
                misoriented_edges=sum(len(u) == 2 and u[0] == u[1] for u in uses.values()),
                degenerate_triangles=int((np.sqrt(_dot(n, n)) == 0).sum()), volume=six / 6,
                aabb_min=tuple(v.min(axis=0)), aabb_max=tuple(v.max(axis=0)))


def records(vertices, triangles):
    """(nt, 30) float64: a, b, c, fu, the edge pseudonormals of ab, bc, ca, the vertex pseudonormals of a, b, c"""
    v, t = np.asarray(vertices, np.float64), np.asarray(triangles, np.int64)
    nt = len(t)
    p = [v[t[:, s]] for s in range(3)]
    n = _cross(p[1] - p[0], p[2] - p[0])
    fu = n / np.sqrt(_dot(n, n))[:, None]
    owner = {(int(t[k, s]), int(t[k, (s + 1) % 3])): k for k in range(nt) for s in range(3)}
    vn = np.zeros((len(v), 3))
    for k in range(nt):
        for s in range(3):
            e1, e2 = p[(s + 1) % 3][k] - p[s][k], p[(s + 2) % 3][k] - p[s][k]
            x = _cross(e1, e2)
            angle = np.arctan2(np.sqrt(_dot(x, x)), _dot(e1, e2))
            vn[t[k, s]] = vn[t[k, s]] + angle * fu[k]
    out = np.zeros((nt, 30))
    for s in range(3):
        out[:, 3 * s:3 * s + 3] = p[s]
        mate = np.array([owner[(int(t[k, (s + 1) % 3]), int(t[k, s]))] for k in range(nt)])
        out[:, 12 + 3 * s:15 + 3 * s] = fu + fu[mate]
        out[:, 21 + 3 * s:24 + 3 * s] = vn[t[:, s]]
    out[:, 9:12] = fu
    return out


def nodes(origin, spacing, dims, dtype):
    """(nodes, 3) of dtype: origin_a + dtype(i_a) * dtype(spacing), node (i, j, k) at (i * dims[1] + j) * dims[2] + k"""
    o, h = np.asarray(origin, np.float64).astype(dtype), dtype(spacing)
    ax = [o[a] + np.arange(int(dims[a])).astype(dtype) * h for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def _pairs(p, rec):
    """every node of p (P, 3) against every record of rec (C, 30), all of one dtype -> (d2, s), each (P, C)"""
    P = [p[:, None, a] for a in range(3)]
    R = [rec[None, :, k] for k in range(30)]

    def sub(u, v):
        return [u[0] - v[0], u[1] - v[1], u[2] - v[2]]

    def dot(u, v):
        return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]

    def axpy(u, t, v):
        return [u[0] + t * v[0], u[1] + t * v[1], u[2] + t * v[2]]

    def sel(c, u, v):
        return [np.where(c, u[0], v[0]), np.where(c, u[1], v[1]), np.where(c, u[2], v[2])]

    a, b, c = R[0:3], R[3:6], R[6:9]
    fu, eab, ebc, eca, na, nb, nc = R[9:12], R[12:15], R[15:18], R[18:21], R[21:24], R[24:27], R[27:30]
    ab, ac, cb = sub(b, a), sub(c, a), sub(c, b)
    ap, bp, cp = sub(P, a), sub(P, b), sub(P, c)
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e, f = d4 - d3, d5 - d6
    in_a = (d1 <= 0) & (d2 <= 0)
    in_b = (d3 >= 0) & (d4 <= d3)
    in_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    in_c = (d6 >= 0) & (d5 <= d6)
    in_ca = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    in_bc = (va <= 0) & (e >= 0) & (f >= 0)
    with np.errstate(all="ignore"):
        q_ab = axpy(a, d1 / (d1 - d3), ab)
        q_ca = axpy(a, d2 / (d2 - d6), ac)
        q_bc = axpy(b, e / (e + f), cb)
        den = (va + vb) + vc
        q_f = axpy(axpy(a, vb / den, ab), vc / den, ac)
    ones = np.ones(np.broadcast(d1, d1).shape, bool)
    q, n = q_f, [x + np.zeros_like(d1) for x in fu]
    for hold, cand, normal in ((in_bc, q_bc, ebc), (in_ca, q_ca, eca), (in_c, c, nc), (in_ab, q_ab, eab), (in_b, b, nb),
                               (in_a, a, na)):           # the first region in the contract's order wins: applied last
        q, n = sel(hold & ones, cand, q), sel(hold & ones, normal, n)
    r = sub(P, q)
    return dot(r, r), dot(r, n)


def field(rec, origin, spacing, dims, dtype, pairs_per_chunk=1 << 20):
    """the fold over ALL pairs -> (best (nodes,) dtype, neg (nodes,) bool); rec (nt, 30) is rounded to dtype here"""
    dtype = np.dtype(dtype).type
    rec = np.asarray(rec).astype(dtype)
    p = nodes(origin, spacing, dims, dtype)
    best, neg = np.full(len(p), np.inf, dtype), np.zeros(len(p), bool)
    step, rows = max(1, pairs_per_chunk // len(p)), np.arange(len(p))
    for t0 in range(0, len(rec), step):
        d2, s = _pairs(p, rec[t0:t0 + step])
        assert d2.dtype == dtype and s.dtype == dtype
        d2 = np.where(d2 != d2, dtype(np.inf), d2)              # a NaN never replaces
        first = np.argmin(d2, axis=1)                           # the lowest index among a chunk's ties
        m = d2[rows, first]
        take = m < best                                         # strictly: an earlier chunk keeps a tie
        best, neg = np.where(take, m, best), np.where(take, s[rows, first] < 0, neg)
    return best, neg


def phi(best, neg, dims, negate=False):
    d = np.sqrt(best)
    return np.where(neg != bool(negate), -d, d).reshape([int(v) for v in dims])


def sdf(vertices, triangles, origin, spacing, dims, dtype=np.float64, negate=False, rec=None):
    best, neg = field(records(vertices, triangles) if rec is None else rec, origin, spacing, dims, dtype)
    return phi(best, neg, dims, negate)


def winding_number(vertices, triangles, points):
    """the generalised winding number of the mesh at `points` (P, 3), float64, all triangles: the solid angles by van
    Oosterom & Strackee's formula, summed and divided by 4 pi.  1 inside a closed outward-oriented mesh, 0 outside."""
    v, t = np.asarray(vertices, np.float64), np.asarray(triangles, np.int64)
    x = np.asarray(points, np.float64)
    w = np.zeros(len(x))
    for k in range(len(t)):
        a, b, c = v[t[k, 0]] - x, v[t[k, 1]] - x, v[t[k, 2]] - x
        la, lb, lc = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1), np.linalg.norm(c, axis=1)
        num = np.einsum("ij,ij->i", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("ij,ij->i", a, b) * lc + np.einsum("ij,ij->i", b, c) * la + np.einsum("ij,ij->i", c, a) * lb
        w += 2 * np.arctan2(num, den)
    return w / (4 * np.pi)
