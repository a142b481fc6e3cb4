"""Reference for pbf_anisotropy_compute — TEST INFRASTRUCTURE.

Written from Yu & Turk 2013 ("Reconstructing surfaces of particle-based fluids using anisotropic kernels", ACM TOG 32(1))
and the comment in include/pbf_hip.h alone: numpy float64, every particle against every particle, numpy.linalg.eigh, no
grid, no sort, no walk, no Jacobi.  Its inputs are what a caller can read back: pstar(), download() and keys().

  candidates   fluid j with r = |p_j - p_i| <= threshold (h by default), i itself included; `cells` (the predict-time cell
               of every particle) restricts the pairs to |cell_i - cell_j| <= 1 per axis, the mask of tests/nversion.py:
               after the solver has moved pStar a neighbour within h can lie outside the 27 cells;
  the sums     w = 1 - (r / h)^3,  S = sum w,  M = sum w d,  Q = sum w d d^T,  d = p_j - p_i,  n = the candidates j != i;
  the record   mu = M / S,  centre = (p_i + smoothing mu) scale,  C = (Q / S - mu mu^T) / h^2 = R diag(sigma) R^T (eigh,
               sorted descending, clamped at 0),  st = k_s max(sigma, sigma_1 / k_r) if n > min_neighbours else k_n with
               R = I,  G = R diag(1 / st) R^T / h.

Per particle it also returns what the GPU test's bars scale with: `amp` = A_i = tr(Q / S) / (h^2 sigma_1), the cancellation
in Q / S - mu mu^T seen from the largest eigenvalue; `edge` = min over the fluid candidates of | r - h |, the distance of the
nearest candidate to the threshold; `k` = the candidate count; `abs_m` = sum |w d| and `cap_m` = sum |d| per axis.
"""
import numpy as np


def predict_cells_from_keys(keys):
    """integer cell coordinates decoded from the 10-bit-per-axis Morton keys"""
    def compact(v):
        v = np.asarray(v, np.uint32) & np.uint32(0x09249249)
        v = (v | (v >> np.uint32(2))) & np.uint32(0x030C30C3)
        v = (v | (v >> np.uint32(4))) & np.uint32(0x0300F00F)
        v = (v | (v >> np.uint32(8))) & np.uint32(0x030000FF)
        v = (v | (v >> np.uint32(16))) & np.uint32(0x000003FF)
        return v.astype(np.int64)
    k = np.asarray(keys, np.uint32)
    return np.stack([compact(k), compact(k >> np.uint32(1)), compact(k >> np.uint32(2))], -1)


def anisotropy(pstar, obstacle, h, scale, pos_world=None, cells=None, smoothing=0.9, k_r=4.0, k_s=20.0 / 3.0, k_n=0.5,
               min_neighbours=25, threshold=None, dtype=np.float64):
    """pstar (n,3+) solver frame, obstacle (n,) bool.  -> dict of float64 arrays: centre (n,3) world, G (n,3,3), axes (n,3,3)
    rows, radii (n,3), sigma (n,3), neighbours (n,), and amp, edge, k, abs_m, cap_m (see the module text).  Obstacles:
    centre = pos_world, everything else 0.  dtype = float32 evaluates the very same expressions in float32 (what the GPU
    test measures the constant of its G bar with)."""
    h = float(h)
    thr = h if threshold is None else float(threshold)
    p = np.asarray(pstar, np.float64)[:, :3].astype(dtype)
    n = len(p)
    obstacle = np.asarray(obstacle, bool)
    d = p[None, :, :] - p[:, None, :]                      # d[i, j] = p_j - p_i
    r = np.sqrt((d * d).sum(-1))
    cand = np.broadcast_to(~obstacle[None, :], (n, n)).copy()
    if cells is not None:
        c = np.asarray(cells, np.int64)
        cand &= (np.abs(c[:, None, :] - c[None, :, :]) <= 1).all(-1)
    inside = cand & (r <= thr)
    w = np.where(inside, 1.0 - (r / h) ** 3, 0.0).astype(dtype)
    S = w.sum(1)
    S1 = np.where(S > 0, S, 1.0)
    M = (w[..., None] * d).sum(1)
    Q = np.einsum("ij,ija,ijb->iab", w, d, d)
    nbr = (inside & ~np.eye(n, dtype=bool)).sum(1)
    mu = M / S1[:, None]
    centre = (p + smoothing * mu) * scale
    C = (Q / S1[:, None, None] - mu[:, :, None] * mu[:, None, :]) / (h * h)
    sig, vec = np.linalg.eigh(C)                            # ascending, eigenvectors as columns
    sig, vec = np.maximum(sig[:, ::-1], 0.0), vec[:, :, ::-1]
    enough = nbr > int(min_neighbours)
    st = np.where(enough[:, None], k_s * np.maximum(sig, sig[:, :1] / k_r), k_n)
    R = np.where(enough[:, None, None], vec, np.eye(3, dtype=dtype)[None])
    st1 = np.where(st > 0, st, 1.0)
    G = np.einsum("iak,ik,ibk->iab", R, 1.0 / st1, R) / h
    axes = np.swapaxes(R, 1, 2).copy()
    flip = np.linalg.det(axes) < 0
    axes[flip, 2] *= -1.0
    trQ = np.trace(Q, axis1=1, axis2=2) / S1
    amp = np.where(sig[:, 0] > 0, trQ / (h * h * np.where(sig[:, 0] > 0, sig[:, 0], 1.0)), np.inf)
    edge = np.where(cand, np.abs(r - h), np.inf).min(1)
    out = dict(centre=centre, G=G, axes=axes, radii=st, sigma=sig, neighbours=nbr.astype(np.int64), amp=amp, edge=edge,
               k=inside.sum(1), abs_m=(np.abs(w)[..., None] * np.abs(d)).sum(1), S=S, enough=enough,
               cap_m=np.where(inside[..., None], np.abs(d), 0).sum(1))
    if obstacle.any():
        o = obstacle
        out["centre"][o] = 0.0 if pos_world is None else np.asarray(pos_world, np.float64)[o]
        for name in ("G", "axes", "radii", "sigma", "neighbours", "k", "abs_m", "cap_m", "S"):
            out[name][o] = 0
        out["amp"][o], out["edge"][o], out["enough"][o] = 0.0, np.inf, False
    return out


def sym6(G):
    """(n,3,3) -> (n,6) in the library's order xx yy zz xy xz yz"""
    return np.stack([G[:, 0, 0], G[:, 1, 1], G[:, 2, 2], G[:, 0, 1], G[:, 0, 2], G[:, 1, 2]], -1)


def full3(g6):
    """(n,6) -> (n,3,3)"""
    g6 = np.asarray(g6, np.float64)
    G = np.empty((len(g6), 3, 3))
    G[:, 0, 0], G[:, 1, 1], G[:, 2, 2] = g6[:, 0], g6[:, 1], g6[:, 2]
    G[:, 0, 1] = G[:, 1, 0] = g6[:, 3]
    G[:, 0, 2] = G[:, 2, 0] = g6[:, 4]
    G[:, 1, 2] = G[:, 2, 1] = g6[:, 5]
    return G
