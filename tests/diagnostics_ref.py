"""Reference for pbf_diagnostics — TEST INFRASTRUCTURE.  numpy float64 and math.fsum, nothing shared with the kernels.

Stream part: from the arrays pbf_download returns, widened to float64; every term formed in double in the order the header
gives (m * x; m * (vx*vx + vy*vy + vz*vz)), summed EXACTLY by math.fsum.  Beside each sum the sum of the terms' magnitudes,
which is what the test's error bound scales with.

Density part: tests/nversion.py — all pairs at once in float64, restricted to the predict-time 27 cells — for rho; the
neighbour counts from the same pair table with a threshold of the caller's choosing, so that a test can bracket the count
between h (1 - delta) and h (1 + delta).
"""
import math

import numpy as np

import nversion as NV

RHO0 = NV.RHO


def fsum(x):
    return math.fsum(np.asarray(x, np.float64).ravel().tolist())


def stream(d):
    """d: dict of pbf_download's arrays -> dict of the stream fields, `max_speed2`, and `abs_<sum>` for every sum."""
    pos, vel = d["pos"].astype(np.float64), d["vel"].astype(np.float64)
    m = d["mass"].astype(np.float64)
    obstacle = (d["type"] & 1) == 1
    finite = np.isfinite(pos).all(1) & np.isfinite(vel).all(1)
    keep = ~obstacle & finite
    out = dict(n_fluid=int(keep.sum()), n_obstacle=int(obstacle.sum()), n_nonfinite=int((~obstacle & ~finite).sum()))
    zero3 = np.zeros(3)
    if not keep.any():
        out.update(mass=0.0, moment=zero3, momentum=zero3, kinetic=0.0, max_speed=0.0, max_speed2=0.0, aabb_min=zero3,
                   aabb_max=zero3, abs_mass=0.0, abs_moment=zero3, abs_momentum=zero3, abs_kinetic=0.0)
        return out
    x, v, m = pos[keep], vel[keep], m[keep]
    mx, mv = m[:, None] * x, m[:, None] * v
    v2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    mk = m * v2
    out.update(mass=fsum(m), moment=np.array([fsum(mx[:, k]) for k in range(3)]),
               momentum=np.array([fsum(mv[:, k]) for k in range(3)]), kinetic=0.5 * fsum(mk),
               max_speed2=float(v2.max()), max_speed=math.sqrt(float(v2.max())), aabb_min=x.min(0), aabb_max=x.max(0),
               abs_mass=fsum(np.abs(m)), abs_moment=np.array([fsum(np.abs(mx[:, k])) for k in range(3)]),
               abs_momentum=np.array([fsum(np.abs(mv[:, k])) for k in range(3)]), abs_kinetic=0.5 * fsum(np.abs(mk)))
    return out


def neighbour_counts(ps, h, obstacle, cells, threshold):
    """candidates j != i (obstacles included) of the predict-time 27 cells with r <= threshold; 0 for obstacles"""
    r, _ = NV.pair_tables(ps, h, cells)
    hit = r <= threshold
    np.fill_diagonal(hit, False)
    return np.where(obstacle, 0, hit.sum(1))


def density(ps, mass, h, obstacle, cells, delta=0.0):
    """-> (rho per particle with 0 for obstacles, neighbour counts at h (1 - delta), at h (1 + delta))"""
    rho = NV.lambdas(ps, mass, h, obstacle, cells)[1]
    rho = np.where(obstacle, 0.0, rho)
    return rho, neighbour_counts(ps, h, obstacle, cells, h * (1 - delta)), neighbour_counts(ps, h, obstacle, cells, h * (1 + delta))


def density_fields(rho, nbr, obstacle):
    """the density fields of pbf_diag from per-particle values"""
    f = ~obstacle
    n = int(f.sum())
    if n == 0:
        return dict(n_density=0, nbr_max=0, rho_min=0.0, rho_max=0.0, rho_mean=0.0, err_mean=0.0, err_max=0.0,
                    compression_mean=0.0, nbr_mean=0.0)
    r = rho[f]
    c = r / RHO0 - 1.0
    return dict(n_density=n, nbr_max=int(nbr[f].max()), rho_min=float(r.min()), rho_max=float(r.max()),
                rho_mean=fsum(r) / n, err_mean=fsum(np.abs(c)) / n, err_max=float(np.abs(c).max()),
                compression_mean=fsum(np.maximum(c, 0.0)) / n, nbr_mean=fsum(nbr[f]) / n)


def lattice(n, spacing=27.0, origin=(100.0, 100.0, 100.0), seed=5, fp64=False, side=None):
    """n fluid particles on a cubic lattice with random velocities and unequal masses (the reduction's size tests)"""
    dt = np.float64 if fp64 else np.float32
    rng = np.random.default_rng(seed)
    side = side or max(1, int(math.ceil(n ** (1.0 / 3.0))))
    i = np.arange(n)
    g = np.stack([i % side, (i // side) % side, i // (side * side)], -1).astype(np.float64)
    return dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=(0.5 + rng.random(n)).astype(dt),
                pos=(g * spacing + np.asarray(origin)).astype(dt), vel=((rng.random((n, 3)) - 0.5) * 4.0).astype(dt),
                colour=np.full((n, 4), 0.5, dt))
