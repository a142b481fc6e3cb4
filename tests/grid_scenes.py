"""Scenes on large, non-cubic and offset grids (test infrastructure).

Every bit-exact test of tests/test_hip_parity.py runs on a 24-26-cell cube with h = 0.1, scale = 500 and
min_bound = 0.  The default device path switches mechanisms on grid size: the 16-bit wrap of the quantised positions
(every 32 cells), the 64-cell x-segments of k_diffuse_rows, the row cube's shift (P = 2^pshift) and, at
P = 1024, the reference's 10-bit wrap of x +- 1 at a face (ROW_FALLBACK walkers).  The geometries here put each of them
under the parity tests (tests/test_grid_geometry_gpu.py); tests/test_grid_geometry_cpu.py checks on the oracle that
each geometry really exercises what it is for.

Particles are sparse: bundles of 2 x 2 lines at rest spacing (0.44 h, the scene factory's 22 world units at scale 500)
along the long axis, a few thousand to ~30 000 per scene, every 11th an obstacle, colours per particle.
"""
import numpy as np

import oracle_lib as O

SPACING = 0.44  # in h (pbf_scene.cpp: 22 world units at h = 0.1, scale = 500)

# ext: the grid extent in cells (ompsph.hpp:132-135); axis: the long axis the lines run along; bundles: (u, v) cell
# coordinates of each bundle on the two other axes (in axis order); span: the long axis' cell range the lines cover;
# pshift: the row cube's shift (pbf_hip.hip: the smallest P = 2^pshift with P^3 >= tableN)
GEOMETRIES = {
    # three 64-cell segments per row plus a tail; qpos wraps at x = 32, 64, 96, 128
    "long_x": dict(ext=(150, 10, 12), h=0.1, scale=500.0, min_bound=(0.0, 0.0, 0.0), axis=0, pshift=8,
                   bundles=[(3.3, 4.1), (6.2, 7.7), (3.6, 9.4), (7.5, 2.6)], span=(2.0, 148.0)),
    # the long axis at the other Morton bit positions: long y / z strides of the row layout
    "tall_y": dict(ext=(10, 140, 12), h=0.1, scale=500.0, min_bound=(0.0, 0.0, 0.0), axis=1, pshift=8,
                   bundles=[(3.3, 4.1), (6.2, 7.7), (3.6, 9.4)], span=(2.0, 138.0)),
    "deep_z": dict(ext=(12, 10, 140), h=0.1, scale=500.0, min_bound=(0.0, 0.0, 0.0), axis=2, pshift=8,
                   bundles=[(4.1, 3.3), (7.7, 6.2), (9.4, 3.6)], span=(2.0, 138.0)),
    # other h, scale (kernel factors, quantisation step 2048 / h) and a negative, unaligned frame; x crosses 32 and 64
    "offset": dict(ext=(70, 40, 33), h=0.17, scale=37.5, min_bound=(-123.37, -57.91, -301.13), axis=0, pshift=7,
                   bundles=[(5.3, 4.4), (12.6, 20.7), (31.4, 30.2), (33.5, 12.5), (20.2, 16.6), (8.6, 27.3), (26.4, 5.7)], span=(2.0, 68.0)),
    # large coordinates: fp32 rounding of p - gridMin and of the quantisation
    "far": dict(ext=(30, 30, 30), h=0.1, scale=1.0, min_bound=(20000.0137, 19999.9709, 20000.0419), axis=0, pshift=5,
                bundles=[(u + 0.37, v + 0.61) for u in (3, 9, 15, 21, 26) for v in (4, 12, 20, 25)], span=(2.0, 28.0)),
    # pshift 10: the reference's x +- 1 wraps between columns 0 and 1023 inside the table; the lines reach both
    # columns (outside the bounds: legal input), the second and third bundles lie on the y = 0 and z = 0 faces
    "edge_x": dict(ext=(1023, 8, 8), h=0.1, scale=500.0, min_bound=(0.0, 0.0, 0.0), axis=0, pshift=10,
                   bundles=[(3.5, 4.5), (0.5, 3.3), (5.2, 0.5)], span=(0.2, 1023.8)),
}
NAMES = list(GEOMETRIES)

# column-0 / column-1023 particles of edge_x get these colours: what the wrap carries across is recognisable
EDGE_LO_COLOUR = (0.9, 0.12, 0.08, 0.5)
EDGE_HI_COLOUR = (0.07, 0.15, 0.95, 0.8)


def morton(x, y, z):
    """curves.h: 10 bits per axis, x at bit 0, y at bit 1, z at bit 2."""
    def spread(v):
        v = int(v) & 0x3FF
        return sum(((v >> b) & 1) << (3 * b) for b in range(10))
    return spread(x) | spread(y) << 1 | spread(z) << 2


def table_len(ext):
    """makeGridTable's length: the Morton code of the extent itself (sph.hpp:238-240)."""
    return morton(*ext)


def row_shift(tn):
    """pbf_hip.hip: the row cube P = 2^pshift that holds every Morton code below tableN."""
    p = 1
    while p < 10 and (1 << (3 * p)) < tn:
        p += 1
    return p


def grid_frame(g, dt):
    """minExtent and extent exactly as ompsph.hpp:132-135 computes them in N (make_consts / grid_extent)."""
    N = dt
    h, scale = N(g["h"]), N(g["scale"])
    lo = np.array([N(N(v) / scale) - N(h * N(2)) for v in g["min_bound"]], N)
    hi = np.array([N(N(v) / scale) + N(h * N(2)) for v in g["max_bound"]], N)
    ext = tuple(int(N((b - a)) / h) for a, b in zip(lo, hi))
    return lo, ext


def bounds(name):
    """The geometry with max_bound solved from its target extent: (max - min) / scale = (ext - 4 + 0.5) h, i.e. half a
    cell of margin on both sides of the truncation, in fp32 and fp64 alike."""
    g = dict(GEOMETRIES[name])
    g["max_bound"] = tuple(m + (e - 3.5) * g["h"] * g["scale"] for m, e in zip(g["min_bound"], g["ext"]))
    for dt in (np.float32, np.float64):
        assert grid_frame(g, dt)[1] == tuple(g["ext"]), (name, dt, grid_frame(g, dt)[1])
    assert row_shift(table_len(g["ext"])) == g["pshift"], (name, row_shift(table_len(g["ext"])))
    return g


def positions(name):
    """World positions (float64) and a per-particle column marker (edge_x: -1 / +1 for x-columns 0 / 1023, else 0)."""
    g = bounds(name)
    h, scale, ax = g["h"], g["scale"], g["axis"]
    others = [a for a in range(3) if a != ax]
    lo = np.array(g["min_bound"]) / scale - 2 * h        # sim units (float64: the cell a particle lies in is decided
    s = SPACING                                          # in N by the kernels; lattice points stay off cell faces)
    along = np.arange(g["span"][0], g["span"][1], s)
    cells = []
    for (u, v) in g["bundles"]:
        for du in (-s / 2, s / 2):
            for dv in (-s / 2, s / 2):
                c = np.zeros((len(along), 3))
                c[:, ax] = along
                c[:, others[0]] = u + du
                c[:, others[1]] = v + dv
                cells.append(c)
    c = np.concatenate(cells)
    pos = (lo + c * h) * scale
    side = np.where(np.floor(c[:, 0]) == 0, -1, np.where(np.floor(c[:, 0]) == 1023, 1, 0)) if name == "edge_x" \
        else np.zeros(len(c), np.int64)
    return pos, side


def make_geometry(name, fp64, pkg=None):
    """-> (scene dict, device Params or None without pkg, oracle params, h).  Jacobi / stable sort, K = 4."""
    g = bounds(name)
    dt = np.float64 if fp64 else np.float32
    pos, side = positions(name)
    n = len(pos)
    rng = np.random.default_rng(sum(map(ord, name)))
    colour = rng.uniform(0.03, 1.0, (n, 4))
    colour[side < 0] = EDGE_LO_COLOUR
    colour[side > 0] = EDGE_HI_COLOUR
    ty = np.zeros(n, np.uint8)
    ty[5::11] = 1
    ty[side != 0] = 0                                     # the wrap's carriers are fluid: they count as candidates
    perm = rng.permutation(n)                             # upload unsorted
    sc = dict(id=np.arange(n, dtype=np.uint64), type=ty[perm], mass=np.ones(n, dt), pos=pos[perm].astype(dt),
              vel=np.zeros((n, 3), dt), colour=colour[perm].astype(dt))
    q = O.make_params(h=g["h"], scale=g["scale"], min_bound=g["min_bound"], max_bound=g["max_bound"], mode=O.JACOBI,
                      sort=O.SORT_STABLE)
    p = None
    if pkg is not None:
        p = pkg.default_params(4, 1000.0)
        p.scale = g["scale"]
        for k in range(3):
            p.min_bound[k] = g["min_bound"][k]
            p.max_bound[k] = g["max_bound"][k]
        assert p.dt == q.dt and list(p.constant_force) == list(q.constant_force) and p.iteration == q.iteration
    return sc, p, q, g["h"]
