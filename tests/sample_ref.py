"""Reference for pbf_sample_points / pbf_sample_lattice — TEST INFRASTRUCTURE.

Written from the comment in include/pbf_hip.h alone: numpy float64, every point against every particle, no table, no sort,
no walk.  Its inputs are what a caller can read back: the download() arrays, pstar(), keys() and extent().

  the point      rounded to N, x_s = point / scale in N (numpy: the same bits the device starts from), its cell
                 trunc((x_s - minExtent) / h) per axis in N; in the grid iff every coordinate is in [0, extent) and the
                 cell's Morton code + 1 < table size — otherwise outside, all zeros;
  the candidates the particles j with |cell_j - cell_x| <= 1 per axis, cell_j decoded from the predict-time key, and
                 key_j + 1 < table size (the walk's 10-bit wrap needs no modelling: a wrapped cell is >= 1022 cells away);
  the term       r = |x_s - pStar_j| in float64, in = r <= threshold (h by default), w = m_j K (h^2 - r^2)^3 with
                 K = 315 / (64 pi h^9); obstacles count in rho and count[1] only.

Per output it returns the sum, the sum of |term| and `cap` = sum over the in-range candidates of m_j W(0) |f_j| (f = 1, v
or c): the two quantities the rounding bars of tests/test_sample_gpu.py scale with.

`mutate` breaks the evaluation on purpose, one rule at a time, so that tests/test_sample_cpu.py can show that the closed
forms it holds this module to would notice: "drop_cell" (the (+1, 0, 0) cell of the 27 is skipped), "sampler_mass" (mass 1
instead of the candidate's), "obstacles_as_fluid", "strict" (r < h for r <= h).
"""
import numpy as np

RHO0 = 6378.0


def poly6_factor(h):
    return 315.0 / (64.0 * np.pi * h ** 9)


def compact10(v):
    v = np.asarray(v, np.uint32) & np.uint32(0x09249249)
    v = (v | (v >> np.uint32(2))) & np.uint32(0x030C30C3)
    v = (v | (v >> np.uint32(4))) & np.uint32(0x0300F00F)
    v = (v | (v >> np.uint32(8))) & np.uint32(0x030000FF)
    v = (v | (v >> np.uint32(16))) & np.uint32(0x000003FF)
    return v.astype(np.int64)


def spread10(x):
    x = np.asarray(x, np.uint32)
    x = (x | (x << np.uint32(16))) & np.uint32(0x030000FF)
    x = (x | (x << np.uint32(8))) & np.uint32(0x0300F00F)
    x = (x | (x << np.uint32(4))) & np.uint32(0x030C30C3)
    x = (x | (x << np.uint32(2))) & np.uint32(0x09249249)
    return x


def morton(cx, cy, cz):
    return spread10(cx) | (spread10(cy) << np.uint32(1)) | (spread10(cz) << np.uint32(2))


def key_cells(keys):
    k = np.asarray(keys, np.uint32)
    return np.stack([compact10(k), compact10(k >> np.uint32(1)), compact10(k >> np.uint32(2))], -1)


def point_cells(points, dtype, h, scale, min_extent):
    """-> (x_s in N, integer cell per axis); every operation in N, as the header states it"""
    N = np.dtype(dtype).type
    xs = np.asarray(points, np.float64).reshape(-1, 3).astype(dtype) / N(scale)
    q = (xs - np.asarray(min_extent, np.float64).astype(dtype)) / N(h)
    assert q.dtype == np.dtype(dtype)
    return xs, np.trunc(q.astype(np.float64)).astype(np.int64)


def in_grid(cells, extent, table_size):
    ext = np.asarray(extent, np.int64)
    ok = ((cells >= 0) & (cells < ext)).all(1)
    c = np.where(ok[:, None], cells, 0).astype(np.uint32)
    code = morton(c[:, 0], c[:, 1], c[:, 2]).astype(np.int64)
    return ok & (code + 1 < int(table_size))


def sample(points, dtype, down, pstar, keys, extent, min_extent, table_size, h, scale, threshold=None, mutate=None):
    """points: (n,3) world.  down: download() dict.  h: the smoothing length as the context holds it (rounded to N).
    -> dict: rho, weight (n,), mv (n,3), mc (n,4), count (n,2), outside (n,), and abs_* / cap_* beside each sum."""
    h = float(h)
    thr = h if threshold is None else float(threshold)
    xs, cx = point_cells(points, dtype, h, scale, min_extent)
    inside = in_grid(cx, extent, table_size)
    keys = np.asarray(keys, np.uint32)
    cj = key_cells(keys)
    dc = cj[None, :, :] - cx[:, None, :]
    cand = (np.abs(dc) <= 1).all(-1) & (keys.astype(np.int64) + 1 < int(table_size))[None, :] & inside[:, None]
    if mutate == "drop_cell":
        cand &= ~((dc[..., 0] == 1) & (dc[..., 1] == 0) & (dc[..., 2] == 0))
    ps = np.asarray(pstar, np.float64)[:, :3]
    d = xs.astype(np.float64)[:, None, :] - ps[None, :, :]
    r = np.sqrt((d * d).sum(-1))
    hit = cand & ((r < thr) if mutate == "strict" else (r <= thr))
    mass = np.asarray(down["mass"], np.float64)
    if mutate == "sampler_mass":
        mass = np.ones_like(mass)
    fluid = np.asarray(down["type"]) == 0
    if mutate == "obstacles_as_fluid":
        fluid = np.ones_like(fluid)
    K = poly6_factor(h)
    w = np.where(hit, mass[None, :] * (K * (h * h - r * r) ** 3), 0.0)
    w0 = np.where(hit, mass[None, :] * (K * h ** 6), 0.0)
    f = hit & fluid[None, :]
    wf, w0f = np.where(f, w, 0.0), np.where(f, w0, 0.0)
    vel, col = np.asarray(down["vel"], np.float64), np.asarray(down["colour"], np.float64)
    with np.errstate(invalid="ignore"):
        tv = np.where(f[..., None], wf[..., None] * vel[None, :, :], 0.0)
        tc = np.where(f[..., None], wf[..., None] * col[None, :, :], 0.0)
        cv = np.where(f[..., None], w0f[..., None] * np.abs(vel)[None, :, :], 0.0)
        cc = np.where(f[..., None], w0f[..., None] * np.abs(col)[None, :, :], 0.0)
    return dict(rho=w.sum(1), abs_rho=np.abs(w).sum(1), cap_rho=w0.sum(1),
                weight=wf.sum(1), abs_weight=np.abs(wf).sum(1), cap_weight=w0f.sum(1),
                mv=tv.sum(1), abs_mv=np.abs(tv).sum(1), cap_mv=cv.sum(1),
                mc=tc.sum(1), abs_mc=np.abs(tc).sum(1), cap_mc=cc.sum(1),
                count=np.stack([f.sum(1), (hit & ~fluid[None, :]).sum(1)], -1).astype(np.int64),
                outside=(~inside).astype(np.uint8), r=np.where(cand, r, np.inf))


def point_set(pos, keys, extent, min_extent, table_size, h, scale, seed):
    """The GPU test's points (world, float64; about 500) for a state given by download()['pos'], keys() and extent():
    every 7th particle's own position; cell corners and face centres (exact multiples of h * scale); uniform random points
    in the box (half of them in the part of it the particles occupy); points in the grid's first and last cell per axis; points outside the grid
    on each side; points within h of every particle that lies outside the grid (none in a scene whose particles all stay
    inside the box: the class is then empty).  -> (points, dict class name -> slice)"""
    rng = np.random.default_rng(seed)
    pos = np.asarray(pos, np.float64)
    ext, lo = np.asarray(extent, np.float64), np.asarray(min_extent, np.float64)
    cell = h * scale
    parts, names = [], []

    def add(name, p):
        names.append((name, len(p)))
        parts.append(np.asarray(p, np.float64).reshape(-1, 3))

    add("particles", pos[::7])
    k = rng.integers(-3, int(ext.max()) + 2, (60, 3)).astype(np.float64)
    add("corners", k * cell)
    f = rng.integers(0, int(ext.min()) - 4, (60, 3)).astype(np.float64) + 0.5
    f[np.arange(60), rng.integers(0, 3, 60)] -= 0.5
    add("faces", f * cell)
    box_lo, box_hi = (lo + 2 * h) * scale, (lo + (ext - 2) * h) * scale
    aabb_lo, aabb_hi = np.maximum(pos.min(0) - cell, box_lo), np.minimum(pos.max(0) + cell, box_hi)
    add("random", np.concatenate([box_lo + rng.random((75, 3)) * (box_hi - box_lo),          # the whole box: mostly empty
                                  aabb_lo + rng.random((75, 3)) * (aabb_hi - aabb_lo)]))     # where the particles are
    edge = []
    for a in range(3):
        for at in (0.5, ext[a] - 0.5):
            p = lo + rng.random((6, 3)) * ext * h
            p[:, a] = lo[a] + at * h
            edge.append(p * scale)
    add("edge_cells", np.concatenate(edge))
    out = []
    for a in range(3):
        for at in (-1.5, -40.0, ext[a] + 0.5, ext[a] + 700.0, 2000.0):
            p = lo + rng.random((2, 3)) * ext * h
            p[:, a] = lo[a] + at * h
            out.append(p * scale)
    add("outside", np.concatenate(out))
    cj = key_cells(keys)
    stray = ((cj >= np.asarray(extent, np.int64)).any(1)) | (np.asarray(keys, np.int64) + 1 >= int(table_size))
    add("near_strays", pos[stray] + (rng.random((int(stray.sum()), 3)) - 0.5) * (1.6 * cell))
    pts = np.concatenate(parts)
    at, classes = 0, {}
    for name, n in names:
        classes[name] = slice(at, at + n)
        at += n
    return pts, classes
