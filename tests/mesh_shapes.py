"""Closed triangle meshes for the mesh-collider tests (pbf_sdf_from_mesh): every generator returns (vertices (nv, 3) float64,
triangles (nt, 3) uint32), counter-clockwise seen from outside, each vertex once (no seams), plus the lattices and the broken
variants the tests share."""
import numpy as np

CENTRE = (520.0, 500.0, 600.0)
LATTICE_A = dict(origin=(203.3, 197.1, 211.7), spacing=37.0, dims=(23, 19, 27))
LATTICE_TIES = dict(origin=(200.0, 200.0, 200.0), spacing=50.0, dims=(13, 13, 13))
LATTICES = {"2x2x2": dict(origin=(480.0, 470.0, 560.0), spacing=90.0, dims=(2, 2, 2)),
            "3x5x4": dict(origin=(310.0, 280.0, 330.0), spacing=110.0, dims=(3, 5, 4)),
            "A": LATTICE_A, "ties": LATTICE_TIES}
TIE_BOX = ((300.0, 300.0, 300.0), (700.0, 700.0, 700.0))
BOX = ((300.0, 310.0, 320.0), (700.0, 640.0, 820.0))
TORUS_R, TORUS_r = 200.0, 70.0
ICO_R = 250.0


def box(lo=BOX[0], hi=BOX[1]):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if (n >> a) & 1 else lo)[a] for a in range(3)] for n in range(8)])      # bit a of n: hi on axis a
    quads = [(0, 2, 6, 4), (1, 5, 7, 3),      # x = lo, x = hi
             (0, 1, 3, 2), (4, 6, 7, 5),      # z = lo, z = hi   (bit 2)
             (0, 4, 5, 1), (2, 3, 7, 6)]      # y = lo, y = hi   (bit 1)
    t = []
    for q in quads:
        t += [(q[0], q[2], q[1]), (q[0], q[3], q[2])]
    return _outward(v, np.array(t, np.uint32))


def tetra(corner=(310.0, 290.0, 333.0), leg=300.0):
    o = np.asarray(corner, np.float64)
    v = np.array([o, o + (leg, 0, 0), o + (0, leg, 0), o + (0, 0, leg)])
    return _outward(v, np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], np.uint32))


def torus(R=TORUS_R, r=TORUS_r, nu=24, nv=12, centre=CENTRE):
    """axis z through `centre`; nu quads round the axis, nv round the tube, two triangles per quad"""
    u = 2 * np.pi * np.arange(nu) / nu
    w = 2 * np.pi * np.arange(nv) / nv
    U, W = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1).reshape(-1, 3)
    t = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            t += [(a, b, c), (a, c, d)]
    return _outward(v + np.asarray(centre, np.float64), np.array(t, np.uint32))


def icosphere(subdivisions=2, R=ICO_R, centre=CENTRE):
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in t:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = out
    return _outward(np.asarray(v) * R + np.asarray(centre, np.float64), np.array(t, np.uint32))


def _outward(v, t):
    vol = np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6
    assert vol > 0, vol
    return np.ascontiguousarray(v, np.float64), np.ascontiguousarray(t, np.uint32)


SHAPES = {"box": box, "tetra": tetra, "torus": torus, "ico2": icosphere}
TRIANGLES = {"box": 12, "tetra": 4, "torus": 576, "ico2": 320, "ico3": 1280}


def shape(name):
    return icosphere(3) if name == "ico3" else SHAPES[name]()


def torus_phi(x, R=TORUS_R, r=TORUS_r, centre=CENTRE):
    d = np.asarray(x, np.float64) - np.asarray(centre, np.float64)
    return np.hypot(np.hypot(d[..., 0], d[..., 1]) - R, d[..., 2]) - r


def broken(name):
    """a closed mesh spoilt in one way -> (vertices, triangles, the pbf_mesh_info count that must say so, its value)"""
    v, t = shape("ico2")
    if name == "open":
        return v, t[:-1].copy(), "boundary_edges", 3
    if name == "flipped":
        t = t.copy()
        t[7] = t[7, ::-1]
        return v, t, "misoriented_edges", 3
    if name == "duplicate":
        return v, np.concatenate([t, t[5:6]]), "nonmanifold_edges", 3
    raise KeyError(name)
