"""NumPy restatement of the static SDF collider's device function (csrc/pbf_collider.hpp, the contract in include/pbf_hip.h),
operation for operation in arrays of dtype N.  NumPy's +, -, *, / and sqrt on float32 / float64 are the IEEE operations and
nothing here is contracted, so equality with the device is exact (tests/test_collider_gpu.py).  Beside it: the float64
closed forms of a plane and a sphere, which the restatement itself is held to (tests/test_collider_cpu.py)."""
import numpy as np


class Lattice:
    """What pbf_set_collider keeps, rounded to N: the nodes, N(origin), inv = N(1) / N(spacing), N(margin)."""

    def __init__(self, phi, origin, spacing, margin, dtype):
        N = np.dtype(dtype).type
        self.N = N
        self.phi = np.ascontiguousarray(np.asarray(phi, np.float64).astype(N))
        assert self.phi.ndim == 3 and min(self.phi.shape) >= 2
        self.dims = self.phi.shape
        self.origin = np.asarray(origin, np.float64).astype(N)
        self.inv = N(1) / N(spacing)
        self.margin = N(margin)


def frame(scale, min_bound, max_bound, dtype):
    """(N(scale), N(min_bound), N(max_bound)) of a pbf_params"""
    N = np.dtype(dtype).type
    return N(scale), np.asarray(min_bound, np.float64).astype(N), np.asarray(max_bound, np.float64).astype(N)


def project(lat, fr, q):
    """q (n,3) of dtype N, the solver-frame position DeltaOp::end computes after the box clamp -> (phi (n,), q' (n,3), hit (n,)
    bool).  phi is +inf outside the lattice; a particle that does not hit keeps its q bit for bit."""
    N = lat.N
    scale, minB, maxB = fr
    q = np.asarray(q)
    assert q.dtype == N and q.ndim == 2 and q.shape[1] == 3
    with np.errstate(all="ignore"):
        w = [q[:, a] * scale for a in range(3)]
        u = [(w[a] - lat.origin[a]) * lat.inv for a in range(3)]
        inside = np.ones(len(q), bool)
        for a in range(3):
            inside &= (u[a] >= N(0)) & (u[a] <= N(lat.dims[a] - 1))  # (NaN compares false: outside)
        us = [np.where(inside, u[a], N(0)) for a in range(3)]  # (an outside u indexes nothing; its results are discarded)
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
        g = [gx, gy, gz]
        ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
        hit = inside & (phi < lat.margin) & (ln > N(0))
        s = (lat.margin - phi) / ln
        out = np.empty_like(q)
        for a in range(3):
            # the device's min / max are fmin / fmax: a NaN operand loses (it cannot arise with a hit on a finite lattice)
            moved = np.fmin(maxB[a] / scale, np.fmax(minB[a] / scale, (w[a] + s * g[a]) / scale))
            out[:, a] = np.where(hit, moved, q[:, a])
        phi = np.where(inside, phi, N(np.inf))
    assert phi.dtype == N and out.dtype == N
    return phi, out, hit


def sample(lat, fr, points):
    """pbf_collider_sample: world points (float64) -> round to N, q = point / scale in N, then project()"""
    N = lat.N
    with np.errstate(all="ignore"):
        q = np.asarray(points, np.float64).reshape(-1, 3).astype(N) / fr[0]
    return project(lat, fr, q)


def on_face(fr, q):
    """(n,) bool: q lies on an image of a box face under the stock clamp (minB / scale or maxB / scale) on some axis"""
    scale, minB, maxB = fr
    return ((q == (minB / scale)[None, :]) | (q == (maxB / scale)[None, :])).any(axis=1)


# ---- float64 closed forms -----------------------------------------------------------------------
def plane_phi(normal, d, w):
    """signed distance of world points w (n,3) to the plane n.w = d (n normalised here), negative on the -n side"""
    n = np.asarray(normal, np.float64)
    n = n / np.sqrt((n * n).sum())
    with np.errstate(invalid="ignore"):
        return np.asarray(w, np.float64) @ n - float(d)


def sphere_phi(centre, r, w):
    x = np.asarray(w, np.float64) - np.asarray(centre, np.float64)
    return np.sqrt((x * x).sum(axis=-1)) - float(r)


# ---- the cases the CPU and GPU tests share --------------------------------------------------------------------------------
SCALE = 500.0
BOX = ((0.0, 0.0, 0.0), (1000.0, 1000.0, 1000.0))
MARGIN = 13.5                                   # half the rest spacing of 27 world units
PLANE_N = (0.2, -0.95, 0.1)                     # not axis-aligned; the fluid side is towards -y (gravity is +y)
PLANE_D = -600.0
PLANE_DIMS, PLANE_SPACING, PLANE_ORIGIN = (23, 19, 27), 47.0, (-15.0, -8.0, -20.0)     # non-cubic, negative origin
PLANE_UNIT = 1600.0                             # largest |coordinate| + |d|: the magnitude the roundings scale with
# worst |n.w' - d - margin| / (eps_N * PLANE_UNIT) over the hit particles that end on no face, measured with project() on
# 2e5 random points (seed 1, tests/test_collider_cpu.py).  The bar is 8 x that: the factor covers other seeds, planes and
# scenes, not the code under test.
PLANE_WORST = {"float32": 0.6963, "float64": 0.96}


def plane_bar_units(dtype):
    return 8.0 * PLANE_WORST[np.dtype(dtype).name]


def plane_bar_world(dtype):
    return plane_bar_units(dtype) * float(np.finfo(dtype).eps) * PLANE_UNIT


def lattice_of(fn, origin, spacing, dims):
    """fn (float64, points (..., 3)) on the nodes origin + (i, j, k) * spacing -> array of shape dims"""
    ax = [float(origin[a]) + np.arange(dims[a], dtype=np.float64) * float(spacing) for a in range(3)]
    return fn(np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1))


def plane_case(dtype, d=PLANE_D, dims=PLANE_DIMS, spacing=PLANE_SPACING, origin=PLANE_ORIGIN, normal=PLANE_N):
    """-> (Lattice of the tilted plane n.w = d, frame of the stock box at scale 500)"""
    phi = lattice_of(lambda x: plane_phi(normal, d, x), origin, spacing, dims)
    return Lattice(phi, origin, spacing, MARGIN, dtype), frame(SCALE, BOX[0], BOX[1], dtype)


# the edge cases of the index arithmetic: scale 512 makes q * scale the point itself, so a point sits ON a node exactly
EDGE_SCALE = 512.0
EDGE_N, EDGE_D = (0.3, 0.5, -0.4), 300.0
EDGE_LATTICES = {(2, 2, 2): ((96.0, 160.0, 32.0), 512.0), (3, 5, 4): ((-64.0, 32.0, 8.0), 128.0),
                 (23, 19, 27): (PLANE_ORIGIN, PLANE_SPACING)}


def edge_case(dims, dtype, n_random=0, seed=11):
    """-> (Lattice, frame, points (float64, each exactly a value of N), names of the leading points).  first / last: the
    outermost values of N that are still inside on that axis (u == 0 and, where the arithmetic is exact, u == dims - 1: i =
    dims - 2, f = 1); before / beyond: their neighbours one ulp further out, which are outside."""
    N = np.dtype(dtype).type
    origin, spacing = EDGE_LATTICES[tuple(dims)]
    n = np.asarray(EDGE_N) / np.linalg.norm(EDGE_N)
    lat = Lattice(lattice_of(lambda x: x @ n - EDGE_D, origin, spacing, dims), origin, spacing, MARGIN, dtype)
    fr = frame(EDGE_SCALE, BOX[0], BOX[1], dtype)
    mid = np.array([origin[a] + 0.37 * (dims[a] - 1) * spacing for a in range(3)]).astype(N).astype(np.float64)

    def inside(a, v):           # the contract's test on axis a for the world coordinate v (a value of N)
        u = (N(v) - lat.origin[a]) * lat.inv
        return bool(u >= N(0) and u <= N(dims[a] - 1))

    pts, names = [], []
    for a in range(3):
        first = N(origin[a])
        while inside(a, np.nextafter(first, N(-np.inf))):
            first = np.nextafter(first, N(-np.inf))
        while not inside(a, first):
            first = np.nextafter(first, N(np.inf))
        last = N(origin[a] + (dims[a] - 1) * spacing)
        while inside(a, np.nextafter(last, N(np.inf))):
            last = np.nextafter(last, N(np.inf))
        while not inside(a, last):
            last = np.nextafter(last, N(-np.inf))
        for name, v in ((f"first{a}", first), (f"before{a}", np.nextafter(first, N(-np.inf))), (f"last{a}", last),
                        (f"beyond{a}", np.nextafter(last, N(np.inf)))):
            p = mid.copy()
            p[a] = float(v)
            pts.append(p), names.append(name)
    pts.append(np.array([origin[a] + (dims[a] - 1) * spacing for a in range(3)])), names.append("corner")
    pts.append(np.full(3, np.nan)), names.append("nan")
    pts.append(np.full(3, np.inf)), names.append("+inf")
    pts.append(np.full(3, -np.inf)), names.append("-inf")
    pts.append(np.array([mid[0], np.nan, mid[2]])), names.append("mixed")
    pts = np.array(pts)
    if n_random:
        rng = np.random.default_rng(seed)
        lo = np.asarray(origin) - 0.1 * spacing * (np.asarray(dims) - 1)
        hi = np.asarray(origin) + 1.1 * spacing * (np.asarray(dims) - 1)
        pts = np.concatenate([pts, (lo + rng.random((n_random, 3)) * (hi - lo)).astype(N).astype(np.float64)])
    return lat, fr, pts, names


# the physics scene: an 8^3 block of fluid at rest spacing falls (gravity +y) onto the tilted plane, which passes ~110
# world units below the block and ~400 above the box floor; the lattice covers the box plus one spacing
BLOCK_PLANE_D = -430.0
BLOCK_STEPS = 30
BLOCK_LATTICE = dict(dims=(23, 23, 23), spacing=50.0, origin=(-50.0, -50.0, -50.0))


def block_scene(k=8):
    g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3)
    n = len(g)
    pos = g * 27.0 + np.array([400.0, 300.0, 400.0])
    return dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n), pos=pos,
                vel=np.zeros((n, 3)), colour=np.full((n, 4), 0.5))
