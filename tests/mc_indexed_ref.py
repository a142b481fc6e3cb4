"""The indexed marching-cubes mesh, restated in numpy from its definition (test infrastructure; the checker of
tests/test_mc_indexed_cpu.py and tests/test_mc_indexed_gpu.py).

Definition (include/pbf_hip.h, pbf_surface_indexed):
  * lattice node (x, y, z), index idx = (x * sy + y) * sz + z, OWNS the lattice edges to its +x, +y and +z neighbours,
    where those exist;
  * an edge is CROSSED iff exactly one of its two node values is < isolevel;
  * the vertex of a crossed edge is interpolated from the owner `f` to the +axis node `t`:
        wgt = (iso - v_f) / (v_t - v_f),   mix(a, b) = a * (1 - wgt) + b * wgt,
    position from coord(k, axis) = (min_extent[axis] + k * step) * scale, normal and colour from the lattice; every operation
    rounded once, in the lattice's own precision;
  * vertices are numbered by ascending owner idx, x < y < z within a node;
  * triangles: cubes in index order over the (sx - 1, sy - 1, sz - 1) march range (z fastest), inside a cube in the order
    of its kMcTriTable row; every entry, a cube edge, becomes the index of that lattice edge's vertex.

Nothing here reads the kernels: the cube's corner and edge numbering comes from the case tables' own convention
(tests/test_mc_tables.py CORNERS / EDGES), the tables from csrc/mc_tables.hpp.
"""
import os

import numpy as np

from test_mc_tables import CORNERS, EDGES, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = os.path.join(ROOT, "pbf-sph_amd", "csrc", "mc_tables.hpp")

# cube edges whose first corner (the end the soup interpolates FROM) is the lower node: the soup's vertex on them is the
# indexed mesh's bit for bit; on the others (2, 3, 6, 7) the soup starts from the upper node
POSITIVE_EDGES = tuple(e for e, (p, q) in enumerate(EDGES) if all(a <= b for a, b in zip(CORNERS[p], CORNERS[q])))
assert POSITIVE_EDGES == (0, 1, 4, 5, 8, 9, 10, 11)


def grid_constants(h, scale, min_bound, resolution, dtype):
    """(min_extent[3], step, scale) in `dtype`, one rounding per operation: min_bound / scale - 2 h and h / resolution
    (reference src/omp/ompsph.hpp:132-135, :291)."""
    t = np.dtype(dtype).type
    mn = np.asarray(min_bound, dtype)
    return mn / t(scale) - t(h) * t(2), t(h) / t(resolution), t(scale)


def _edge_owner():
    """Per cube edge: (corner offset of the owning node, axis)."""
    out = []
    for p, q in EDGES:
        a, b = np.array(CORNERS[p]), np.array(CORNERS[q])
        d = b - a
        assert np.abs(d).sum() == 1
        out.append((tuple(np.minimum(a, b)), int(np.nonzero(d)[0][0])))
    return out


def extract(sample, pn, c, min_extent, step, scale, isolevel):
    """-> dict(vs (V,3), ns (V,3), cs (V,4), tris (T,3) uint32, owner (V,) node index, axis (V,), cube_edge (3T,) the
    cube edge number behind every de-indexed vertex, end_f / end_t (3T,) the node indices the SOUP interpolates that vertex
    from and to)."""
    dtype = pn.dtype
    t = dtype.type
    assert c.dtype == dtype and np.asarray(min_extent).dtype == dtype
    sx, sy, sz = (int(v) for v in sample)
    n = sx * sy * sz
    assert pn.shape == (n, 4) and c.shape == (n, 4)
    iso = t(isolevel)
    stride = (sy * sz, sz, 1)
    below = (pn[:, 0] < iso).reshape(sx, sy, sz)
    crossed = np.zeros((sx, sy, sz, 3), bool)
    crossed[:-1, :, :, 0] = below[:-1] != below[1:]
    crossed[:, :-1, :, 1] = below[:, :-1] != below[:, 1:]
    crossed[:, :, :-1, 2] = below[:, :, :-1] != below[:, :, 1:]
    flat = crossed.reshape(-1)                       # (node, axis): ascending owner index, x < y < z inside a node
    vid = np.cumsum(flat) - 1
    at = np.nonzero(flat)[0]
    owner, axis = at // 3, at % 3
    nv = len(at)
    f, to = owner, owner + np.array(stride)[axis]
    with np.errstate(all="ignore"):
        wgt = (iso - pn[f, 0]) / (pn[to, 0] - pn[f, 0])
        one = t(1)

        def mix(a, b):
            return a * (one - wgt) + b * wgt

        xyz = np.stack([owner // stride[0], (owner // sz) % sy, owner % sz], 1)
        vs = np.empty((nv, 3), dtype)
        for k in range(3):
            cf = (min_extent[k] + xyz[:, k].astype(dtype) * step) * scale
            ct = (min_extent[k] + (xyz[:, k] + (axis == k)).astype(dtype) * step) * scale
            vs[:, k] = mix(cf, ct)
        ns = np.stack([mix(pn[f, k], pn[to, k]) for k in (1, 2, 3)], 1)
        cs = np.stack([mix(c[f, k], c[to, k]) for k in range(4)], 1)
    assert vs.dtype == dtype and ns.dtype == dtype and cs.dtype == dtype and wgt.dtype == dtype

    empty = dict(vs=vs, ns=ns, cs=cs, tris=np.zeros((0, 3), np.uint32), owner=owner, axis=axis,
                 cube_edge=np.zeros(0, np.int64), end_f=np.zeros(0, np.int64), end_t=np.zeros(0, np.int64))
    if min(sx, sy, sz) < 2:
        return empty
    _, _, tri = load(TABLES)
    own = _edge_owner()
    corner_off = np.array([(cx * sy + cy) * sz + cz for cx, cy, cz in CORNERS])
    own_off = np.array([(o[0] * sy + o[1]) * sz + o[2] for o, _ in own])
    own_axis = np.array([a for _, a in own])
    edge_f = np.array([p for p, _ in EDGES])
    edge_t = np.array([q for _, q in EDGES])
    ci = np.zeros((sx - 1, sy - 1, sz - 1), np.int64)
    for k, (cx, cy, cz) in enumerate(CORNERS):
        ci |= below[cx:sx - 1 + cx, cy:sy - 1 + cy, cz:sz - 1 + cz].astype(np.int64) << k
    ci = ci.reshape(-1)                              # cube order: x slowest, z fastest over the march range
    cube = np.nonzero((ci != 0) & (ci != 255))[0]
    rows = tri[ci[cube]]                             # (m, 16) cube edges, 255-terminated
    valid = rows != 255
    rz, ry = sz - 1, sy - 1
    base = ((cube // (ry * rz)) * sy + (cube // rz) % ry) * sz + cube % rz
    e = np.where(valid, rows, 0)
    node = base[:, None] + own_off[e]
    idx = vid[node * 3 + own_axis[e]]
    assert flat[(node * 3 + own_axis[e])[valid]].all(), "a table entry names an edge that is not crossed"
    tris = idx[valid].astype(np.uint32).reshape(-1, 3)   # row-major: cube order, then table order
    return dict(vs=vs, ns=ns, cs=cs, tris=tris, owner=owner, axis=axis, cube_edge=e[valid],
                end_f=(base[:, None] + corner_off[edge_f[e]])[valid], end_t=(base[:, None] + corner_off[edge_t[e]])[valid])


def node_coords(sample, min_extent, step, scale, nodes):
    """(len(nodes), 3) coordinates of lattice nodes, in the lattice's precision."""
    sx, sy, sz = (int(v) for v in sample)
    dtype = np.asarray(min_extent).dtype
    xyz = np.stack([nodes // (sy * sz), (nodes // sz) % sy, nodes % sz], 1)
    return np.stack([(min_extent[k] + xyz[:, k].astype(dtype) * step) * scale for k in range(3)], 1)


def soup_bound(a, b):
    """Largest difference between the soup's and the indexed mesh's value on an edge interpolated from opposite ends, for
    end values a, b (float64 arrays of the lattice's values) in the precision `u` — derivation in
    tests/test_mc_indexed_cpu.py.  Returned per unit roundoff: multiply by u and add the underflow term there."""
    return 6.0 * np.maximum(np.abs(a), np.abs(b)) + 3.0 * np.abs(b - a)


def compare_with_soup(ix, soup, lattice, consts, isolevel):
    """De-index `ix` (extract()'s dict, or the device's arrays plus extract()'s cube_edge / end_f / end_t) and compare
    it with a soup dict(vs, ns, cs).  -> dict(n_pos, n_neg, n_inf, worst): worst = the largest |difference| / bound over
    the vertices on negative-oriented cube edges (0 if there are none).  Raises AssertionError when a positive-oriented
    vertex differs in any bit, NaNs sit in different places, or a ratio exceeds 1.

    The bound presupposes finite field values.  A particle exactly on a node makes that node's value +inf (size / 0), and
    then the direction decides by IEEE rules alone: from the infinite end the weight is inf / inf = NaN, towards it
    (iso - v) / inf = 0 and the vertex is the finite end.  The n_inf negative-oriented vertices on such edges are held to
    something stricter than a bound instead: the soup's value must equal, bit for bit, the same expressions evaluated
    here from the soup's end."""
    sample, pn, c = lattice
    min_extent, step, scale = consts
    dtype = pn.dtype
    t = dtype.type
    u = float(np.finfo(dtype).eps) / 2
    eta = float(np.finfo(dtype).smallest_subnormal)
    flat = ix["tris"].reshape(-1)
    assert len(flat) == len(soup["vs"]) == len(ix["cube_edge"]), (len(flat), len(soup["vs"]))
    pos = np.isin(ix["cube_edge"], POSITIVE_EDGES)
    neg = ~pos
    worst = 0.0
    vf, vt = pn[ix["end_f"], 0], pn[ix["end_t"], 0]
    inf = neg & ~(np.isfinite(vf) & np.isfinite(vt))
    neg = neg & ~inf
    with np.errstate(all="ignore"):
        wsoup = (t(isolevel) - vf[inf]) / (vt[inf] - vf[inf])
    ends = {"vs": (node_coords(sample, min_extent, step, scale, ix["end_f"]),
                   node_coords(sample, min_extent, step, scale, ix["end_t"])),
            "ns": (pn[ix["end_f"], 1:], pn[ix["end_t"], 1:]),
            "cs": (c[ix["end_f"]], c[ix["end_t"]])}
    for k in ("vs", "ns", "cs"):
        mine, theirs = ix[k][flat], soup[k]
        assert mine.dtype == theirs.dtype == dtype
        assert np.array_equal(mine[pos], theirs[pos], equal_nan=True), (k, "positive-oriented edges must agree bit for bit")
        assert np.array_equal(np.isnan(mine[~inf]), np.isnan(theirs[~inf])), (k, "NaN in different places")
        with np.errstate(all="ignore"):
            ef, et = ends[k][0][inf], ends[k][1][inf]
            want = ef * (t(1) - wsoup)[:, None] + et * wsoup[:, None]
        assert want.dtype == dtype and np.array_equal(theirs[inf], want, equal_nan=True), (k, "edge with a non-finite field value")
        a, b = (v.astype(np.float64)[neg] for v in ends[k])
        with np.errstate(all="ignore"):
            bound = (soup_bound(a, b) * u) * (1 + 10 * u) + eta * (np.abs(b - a) + 2)
            d = np.abs(mine[neg].astype(np.float64) - theirs[neg].astype(np.float64))
            ratio = d / bound
        both_nan = np.isnan(mine[neg]) & np.isnan(theirs[neg])
        ratio = np.where(both_nan | (d == 0), 0.0, ratio)
        assert not np.isnan(ratio).any(), (k, "a finite vertex between non-finite ends")
        if ratio.size:
            worst = max(worst, float(ratio.max()))
    assert worst <= 1.0, ("the derivation of the bound is wrong, or the interpolation is", worst)
    return dict(n_pos=int(pos.sum()), n_neg=int(neg.sum()), n_inf=int(inf.sum()), worst=worst)


def directed_edge_defects(tris):
    """Index-level watertightness: the number of undirected edges that are NOT used by exactly two triangles, once in each
    direction, and the number of undirected edges.  Degenerate triangles (a repeated index) cannot exist in an indexed
    mesh whose three vertices sit on three different lattice edges; they are counted like any other."""
    t = np.asarray(tris, np.int64)
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    n = int(t.max()) + 1 if t.size else 1
    fwd = np.unique(a * n + b, return_counts=True)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    und, cnt = np.unique(lo * n + hi, return_counts=True)
    bad = int((cnt != 2).sum()) + int((fwd[1] != 1).sum())   # (a directed edge used twice: same direction on both sides)
    return bad, len(und)
