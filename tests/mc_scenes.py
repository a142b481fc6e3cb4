"""Scenes that take the marching-cubes field to its edges (test infrastructure, beside tests/grid_scenes.py).

Each scene is a few thousand particles at most, so that the all-pairs evaluation of tests/nversion_mc.py stays in
seconds.  tests/test_mc_nversion_cpu.py proves on the CPU that each scene exercises the mechanism it is for.

  faces      iteration = 0, zero force, zero velocity: particles stay where they are put, through the whole padded
             grid (2 h beyond the bounds, where delta-p's clamp would never leave them), with groups in the face, edge
             and corner cells at both ends of all three axes.  Extent (10, 9, 8): with resolution 1.5 extent * res is
             an integer on x and z (a last node plane whose cell is the extent itself) and not on y.
  obstacles  the two-cube blob, a slab of its particles turned into obstacles, settled for three frames.
  on_node    h = 0.125, scale = 512, bounds [0, 512]: every lattice coordinate (-0.25 + k/16) * 512 = -128 + 32 k is
             exact in fp32 and fp64, and so is pos / scale * scale.  One particle on node (8, 10, 6), exactly one
             threshold (64) from six other nodes; one particle 1e-3 from node (10, 9, 5), along the diagonal; forty ordinary
             particles around the 4 x 4 x 4 node block [8, 12) x [8, 12) x [4, 8); 150 more in the far corner of the box.
  blob       oracle_lib.scene_cubes(2048) after three frames.
  cloud      test_nversion_cpu.scene("cloud") after two frames of two iterations.
"""
import numpy as np

import nversion as NV
import oracle_lib as O

NAMES = ("faces", "obstacles", "on_node", "blob", "cloud")

# (resolution, isolevel, particle size, particle influence) per scene: the stock set (sph.hpp:179-184) and three
# others; each isolevel lies inside the range of v of its scene, so that the mesh is non-trivial (asserted on the CPU)
PARAMS = {
    "faces": [(2.0, 100.0, 25.0, 0.5), (1.5, 40.0, 25.0, 0.75), (1.0, 15.0, 25.0, 1.0), (3.0, 60.0, 25.0, 0.5)],
    "obstacles": [(2.0, 100.0, 25.0, 0.5), (1.5, 40.0, 25.0, 0.75), (1.0, 15.0, 25.0, 1.0), (3.0, 100.0, 25.0, 0.5)],
    # on_node: the particle coincides with a node at resolutions 2 and 1 only (h / 1.5 and h / 3 are not exact); at
    # the other two the scene still has the 1e-3 particle and the block
    "on_node": [(2.0, 20.0, 25.0, 0.5), (1.5, 8.0, 25.0, 0.75), (1.0, 2.0, 25.0, 1.0), (3.0, 20.0, 25.0, 0.5)],
    "blob": [(2.0, 100.0, 25.0, 0.5), (1.5, 40.0, 25.0, 0.75), (1.0, 15.0, 25.0, 1.0), (3.0, 100.0, 25.0, 0.5)],
    "cloud": [(2.0, 100.0, 25.0, 0.5), (1.5, 40.0, 25.0, 0.75), (1.0, 15.0, 25.0, 1.0), (3.0, 100.0, 25.0, 0.5)],
}

# The surface in slab mode (tests/test_slab_surface_cpu.py, tests/test_slab_surface_gpu.py): per case the scene, the
# worker's --cuts, the cuts as cell columns, the precisions and the parameter sets in call order.  A set that begins with
# "!" must be refused (an interior rank without a node plane).  Resolution 0.7 on `faces` (extent 10 on x: nodes in
# the cells 0 1 2 4 5 7 8 10, so columns own one or no plane each); its isolevel 50 is near the median of v over the
# nodes with hits (45; quartiles 31 and 66).
FACES_07 = (0.7, 50.0, 25.0, 0.5)
SLAB_PARAMS = {
    "faces-3": dict(scene="faces", extent_x=10, cuts="c:3,7", columns=(0, 3, 7, 1024), fp64=(False, True),
                    sets=PARAMS["faces"] + [FACES_07]),
    # rank 2 is one column wide: its particles are in both neighbours' ghost sets
    "faces-4": dict(scene="faces", extent_x=10, cuts="c:3,4,7", columns=(0, 3, 4, 7, 1024), fp64=(False, True),
                    sets=PARAMS["faces"] + [("!",) + FACES_07, PARAMS["faces"][0]]),
    # slab.column_of(210) = 6 runs through the obstacle sheet (columns 5 and 6), column_of(700) = 15 (1.4 + 0.2 rounds below
    # 1.6) through the second cube
    "obstacles-3": dict(scene="obstacles", extent_x=24, cuts="x:210,700", columns=(0, 6, 15, 1024), fp64=(False, True),
                        sets=PARAMS["obstacles"][:2]),
    # the cubes start in the columns 4-7 and 13-17 and spread to 2-9 and 12-19 by the third frame: rank 1 (columns 10-12)
    # starts without a particle, steps with none, and is reached by migrants and copies from its right-hand neighbour
    "blob-3": dict(scene="blob", extent_x=24, cuts="c:10,13", columns=(0, 10, 13, 1024), fp64=(False,), sets=PARAMS["blob"][:1]),
    # nothing ever reaches column 20: ranks 1 and 2 own no particle and receive no copy, from the upload to the surface
    "blob-empty": dict(scene="blob", extent_x=24, cuts="c:21,23", columns=(0, 21, 23, 1024), fp64=(False,),
                       sets=PARAMS["blob"][:1]),
}

FACES_EXT = (10, 9, 8)
ON_NODE = (8, 10, 6)            # lattice index of the node that carries a particle (resolution 2; (4, 5, 3) at 1)
NEAR_NODE = (10, 9, 5)
BLOCK = ((8, 12), (8, 12), (4, 8))


def _scene(pos, colour, ptype=None, vel=None):
    n = len(pos)
    return dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8) if ptype is None else ptype,
                mass=np.ones(n), pos=np.asarray(pos, np.float64), vel=np.zeros((n, 3)) if vel is None else vel,
                colour=np.asarray(colour, np.float64))


def make(name):
    """-> dict(sc, h, scale, min_bound, max_bound, iteration, force, frames)."""
    if name == "faces":
        rng = np.random.default_rng(20260)
        h, scale = 0.1, 500.0
        ext = np.array(FACES_EXT)
        mn = np.zeros(3)
        mx = mn + (ext - 3.5) * h * scale                   # half a cell of margin around the truncation
        cells = [rng.integers(0, ext, (1500, 3))]
        ends = [(0, e - 1) for e in ext]
        for cx in ends[0]:                                  # corners: six particles in each of the eight cells
            for cy in ends[1]:
                for cz in ends[2]:
                    cells.append(np.tile([cx, cy, cz], (6, 1)))
        for ax in range(3):                                 # edges: three particles in four cells of each of the 12
            o = [a for a in range(3) if a != ax]
            for c0 in ends[o[0]]:
                for c1 in ends[o[1]]:
                    for k in rng.integers(1, ext[ax] - 1, 4):
                        c = np.zeros(3, np.int64)
                        c[ax], c[o[0]], c[o[1]] = k, c0, c1
                        cells.append(np.tile(c, (3, 1)))
        cells = np.concatenate(cells)
        frac = rng.uniform(0.08, 0.92, cells.shape)         # off the cell faces: the cell is the same in every precision
        lo = mn / scale - 2 * h
        pos = (lo + (cells + frac) * h) * scale
        return dict(sc=_scene(pos, rng.uniform(0.03, 1.0, (len(pos), 4))), h=h, scale=scale, min_bound=tuple(mn),
                    max_bound=tuple(mx), iteration=0, force=(0.0, 0.0, 0.0), frames=1, placed_cells=cells)
    if name == "on_node":
        rng = np.random.default_rng(7)
        h, scale = 0.125, 512.0
        node = -128.0 + 32.0 * np.array(ON_NODE)
        near = -128.0 + 32.0 * np.array(NEAR_NODE) + 1e-3 / np.sqrt(3.0)
        lo = np.array([-128.0 + 32.0 * b[0] for b in BLOCK]) - 30.0
        hi = np.array([-128.0 + 32.0 * (b[1] - 1) for b in BLOCK]) + 30.0
        rest = lo + rng.random((40, 3)) * (hi - lo)
        # a second group away from the block.  With h / 3 inexact, the particle on the node lies within rounding of one
        # threshold from 30 nodes at resolution 3 (offsets with i^2 + j^2 + k^2 = 9 steps): they are band nodes by
        # arithmetic, and the scene is large enough that they stay below 1 % of its nodes with hits
        far = np.array([250.0, 250.0, 250.0]) + rng.random((150, 3)) * 230.0
        pos = np.concatenate([node[None], near[None], rest, far])
        return dict(sc=_scene(pos, rng.uniform(0.03, 1.0, (len(pos), 4))), h=h, scale=scale, min_bound=(0.0,) * 3,
                    max_bound=(512.0,) * 3, iteration=0, force=(0.0, 0.0, 0.0), frames=1)
    std = dict(h=0.1, scale=500.0, min_bound=(0.0,) * 3, max_bound=(1000.0,) * 3, force=(0.0, 9.8, 0.0))
    if name == "blob":
        return dict(sc=O.scene_cubes(2048, True), iteration=4, frames=3, **std)
    if name == "obstacles":
        sc = O.scene_cubes(2048, True)
        x = sc["pos"][:, 0]
        first = x < 450.0                                   # the cube at (100, 0, 100)
        mid = np.median(x[first])
        sc["type"][first & (np.abs(x - mid) < 30.0)] = 1    # a slab of two to three lattice planes across it
        return dict(sc=sc, iteration=4, frames=3, **std)
    if name == "cloud":
        import test_nversion_cpu
        return dict(sc=test_nversion_cpu.scene("cloud"), iteration=2, frames=2, **std)
    raise KeyError(name)


def oracle_params(s, **kw):
    return O.make_params(h=s["h"], scale=s["scale"], iteration=s["iteration"], force=s["force"],
                         min_bound=s["min_bound"], max_bound=s["max_bound"], mode=O.JACOBI, sort=O.SORT_STABLE, **kw)


def device_params(pkg, s):
    p = pkg.default_params(s["iteration"], 1000.0)
    p.scale = s["scale"]
    for k in range(3):
        p.constant_force[k] = s["force"][k]
        p.min_bound[k] = s["min_bound"][k]
        p.max_bound[k] = s["max_bound"][k]
    q = oracle_params(s)
    assert p.dt == q.dt and p.iteration == q.iteration
    return p


def cast(sc, dtype):
    return {k: (v.astype(dtype) if v.dtype.kind == "f" else v.copy()) for k, v in sc.items()}


def predict_time_cells(before, s, ids_after):
    """The cells the surface's table was built from: nversion.predict on the state BEFORE the last step, binned by
    nversion.predict_cells, returned in the order of `ids_after` (the state after the step, matched by id)."""
    f = lambda a: np.asarray(a, np.float64)
    _, ps = NV.predict(f(before["pos"]), f(before["vel"]), f(before["mass"]), O.make_params().dt, s["scale"],
                       s["force"])
    ps = np.where((np.asarray(before["type"]) == 1)[:, None], f(before["pos"]) / s["scale"], ps)
    cells = NV.predict_cells(ps, s["h"], s["scale"], s["min_bound"])
    order = np.argsort(before["id"])
    at = np.searchsorted(before["id"][order], ids_after)
    assert np.array_equal(before["id"][order][at], ids_after)
    return cells[order][at]



def lattice_of(s, mc, fp64):
    import nversion_mc as NM
    return NM.Lattice(s["h"], s["scale"], s["min_bound"], s["max_bound"], mc[0], np.float64 if fp64 else np.float32)


def on_node_index(mc):
    """on_node: the lattice index (x, y, z) of the node that carries the particle, or None at a resolution where no
    node coincides with it."""
    if mc[0] not in (1.0, 2.0):
        return None
    return np.array(ON_NODE) * int(mc[0]) // 2


def exact_nodes(name, lat, mc):
    """on_node: the six nodes exactly one threshold from the particle on a node (every operation on the way to len is
    exact there, asserted in test_mc_nversion_cpu.py::test_on_node_scene_is_exact)."""
    k = on_node_index(mc) if name == "on_node" else None
    if k is None:
        return ()
    d = int(mc[0])                                          # one threshold = h * scale = res lattice steps
    out = []
    for ax in range(3):
        for sgn in (-d, d):
            j = k.copy()
            j[ax] += sgn
            out.append(int(lat.index(*j)))
    return out
