"""NumPy restatement of the winding-number sign (PBF_MESH_SIGN_WINDING / pbf_mesh_winding, include/pbf_hip.h), parametrised by
dtype: float32, float64 or np.longdouble.  One NumPy operation per operation of the contract, in its order, everything in
`dtype`; the sum runs over the triangles in ascending index from 0.  The distance side is tests/mesh_sdf_ref.py's fold on the
soup's a, b, c (records30 pads them to the 30 columns it reads; the normals it ignores for `best` are zero).

The bars (tests/test_mesh_winding_cpu.py measures them and holds these figures): WORST[N] is the largest |w_N - w_longdouble|
of this restatement over the seven soups and five closed meshes of tests/mesh_soups.py on the lattices 3x5x4 and A, at the
nodes with sqrt(best) >= 1e-3 spacing; bar_w(N) = 8 WORST[N], the factor this project gives its restatements for an
unrelated libm and summation."""
import numpy as np

import mesh_sdf_ref as MR

# measured by test_mesh_winding_cpu.test_value_bar (which asserts the measurement stays within them)
WORST = {np.float32: 2.8e-6, np.float64: 9.7e-15}      # (both on `bowl` x A: 2.76e-6 and 9.68e-15)
NEAR = 1e-3          # nodes nearer to the mesh than NEAR * spacing are left out of the value check: num's sign is rounding there


def bar_w(dtype):
    return 8 * WORST[np.dtype(dtype).type]


def pi_of(dtype):
    dtype = np.dtype(dtype).type
    return 4 * np.arctan(np.longdouble(1)) if dtype is np.longdouble else dtype(np.pi)


def two_pi_of(dtype):
    dtype = np.dtype(dtype).type
    return 8 * np.arctan(np.longdouble(1)) if dtype is np.longdouble else dtype(2 * np.pi)


def soup_records(vertices, triangles):
    """(nt, 9) float64: a, b, c"""
    v, t = np.asarray(vertices, np.float64), np.asarray(triangles, np.int64)
    return np.concatenate([v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]], axis=1)


def records30(rec9):
    out = np.zeros((len(rec9), 30), np.asarray(rec9).dtype)
    out[:, :9] = rec9
    return out


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def angles(p, rec, cross_sign=1, with_lll=True):
    """atan2(num, den) of every node of p (P, 3) against every record of rec (C, 9), all of one dtype -> (P, C).  The two
    switches are the mutations of test_mesh_winding_cpu: b x c with the wrong sign, den without the la lb lc term."""
    P = [p[:, None, k] for k in range(3)]
    a, b, c = ([rec[None, :, 3 * s + k] - P[k] for k in range(3)] for s in range(3))
    la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
    x = [b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]]
    if cross_sign < 0:
        x = [-x[0], -x[1], -x[2]]
    num = _dot(a, x)
    if with_lll:
        den = ((la * lb) * lc + _dot(a, b) * lc) + (_dot(b, c) * la + _dot(c, a) * lb)
    else:
        den = (_dot(a, b) * lc) + (_dot(b, c) * la + _dot(c, a) * lb)
    return np.arctan2(num, den)


def winding_sum(rec9, origin, spacing, dims, dtype, pairs_per_chunk=1 << 20, **mutation):
    """S (nodes,) of dtype: the sum over ALL triangles in ascending index; rec9 (nt, 9) is rounded to dtype here"""
    dtype = np.dtype(dtype).type
    rec = np.asarray(rec9).astype(dtype)
    p = MR.nodes(origin, spacing, dims, dtype)
    S = np.zeros(len(p), dtype)
    step = max(1, pairs_per_chunk // len(p))
    for t0 in range(0, len(rec), step):
        A = angles(p, rec[t0:t0 + step], **mutation)
        assert A.dtype == dtype
        for k in range(A.shape[1]):
            S = S + A[:, k]
    return S


def w_of(S):
    return S / two_pi_of(S.dtype)


def neg_of(best, S, threshold=None):
    return (best > 0) & (S > (pi_of(S.dtype) if threshold is None else S.dtype.type(threshold)))


def phi(best, neg, dims, negate=False):
    return MR.phi(best, neg, dims, negate)


# ---- the cases the CPU and the GPU tests share: computed once per process and left unchanged -----------------------------------
_cache = {}


def case(name, lattice, dtype):
    """(best, S) of the restatement in dtype for a mesh of tests/mesh_soups.py on a lattice of tests/mesh_shapes.py; best is
    mesh_sdf_ref's fold on the soup's a, b, c (float64 for the longdouble case, which is the reference of S alone)"""
    import mesh_shapes as MS
    import mesh_soups as SP
    dtype = np.dtype(dtype).type
    key = (name, lattice, dtype)
    if key not in _cache:
        v, t = SP.mesh(name, lattice)
        L = MS.LATTICES[lattice]
        rec = soup_records(v, t)
        if dtype is np.longdouble:
            best = case(name, lattice, np.float64)[0]
        else:
            best, _ = MR.field(records30(rec), L["origin"], L["spacing"], L["dims"], dtype)
        S = winding_sum(rec, L["origin"], L["spacing"], L["dims"], dtype)
        best.setflags(write=False), S.setflags(write=False)
        _cache[key] = (best, S)
    return _cache[key]


def far_nodes(best, spacing):
    """the nodes of the value check: not nearer to the mesh than NEAR * spacing"""
    return np.sqrt(best.astype(np.float64)) >= NEAR * spacing
