"""Grid-free, all-pairs float64 restatement of the opt-in surface tension and adhesion (Akinci, Akinci & Teschner 2013,
"Versatile Surface Tension and Adhesion for SPH Fluids", ACM TOG 32(6)) exactly as include/pbf_hip.h defines it, in the
solver frame (pStar after finalise, h = pbf_desc.h, m = particle mass, rho0 = RHO):

  rho_i = sum_{j in N(i) u {i}} m_j W_poly6(r)                              (obstacle neighbours included)
  n_i   = h sum_{fluid j != i} (m_j / rho_j) grad W_spiky(x_ij)
  dv_i  = -dt [ sum_{fluid j} K_ij (gamma m_j C(r) x_ij / r + gamma (n_i - n_j))
                + sum_{obstacle b} beta m_b A(r) x_ib / r ],        K_ij = 2 rho0 / (rho_i + rho_j)

(the force divided by m_i).  N(i) = candidates within h in the 27 predict-time cells (nversion.pair_tables with cells);
direction terms need r >= EPSILON (the spiky convention).  Obstacles: zero records, dv = 0.  Akinci's boundary
pseudo-mass Psi_b is the obstacle particle's own mass here.
"""
import numpy as np

import nversion as NV


def cohesion_kernel(r, h):
    """Akinci's cohesion spline C(r): 32 / (pi h^9) {(h - r)^3 r^3 on (h/2, h];  2 (h - r)^3 r^3 - h^6 / 64 on (0, h/2]}"""
    r = np.asarray(r, float)
    f = 32.0 / (np.pi * h ** 9)
    q = (h - r) ** 3 * r ** 3
    return np.where((r > h / 2) & (r <= h), f * q, np.where((r > 0) & (r <= h / 2), f * (2.0 * q - h ** 6 / 64.0), 0.0))


def adhesion_kernel(r, h):
    """Akinci's adhesion kernel A(r) = 0.007 / h^3.25 (-4 r^2 / h + 6 r - 2 h)^(1/4) on (h/2, h], else 0"""
    r = np.asarray(r, float)
    x = np.maximum(-4.0 * r * r / h + 6.0 * r - 2.0 * h, 0.0)
    return np.where((r > h / 2) & (r <= h), 0.007 / h ** 3.25 * np.sqrt(np.sqrt(x)), 0.0)


def surface_state(ps, mass, h, obstacle=None, cells=None):
    """-> (rho, normals, r, grad): the density and the surface normal of every particle (zero rows for obstacles)"""
    n = len(ps)
    obstacle = np.zeros(n, bool) if obstacle is None else np.asarray(obstacle, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        r, g = NV.pair_tables(ps, h, cells)      # r = inf outside the 27 cells; g = grad_i W_spiky(x_ij), 0 unless EPS <= r <= h
        rho = (mass[None, :] * NV.poly6(r, h)).sum(1)
    rho = np.where(obstacle, 0.0, rho)
    fluid = ~obstacle
    wj = np.where(fluid, mass / np.where(fluid, rho, 1.0), 0.0)
    nrm = h * (g * wj[None, :, None]).sum(1)
    nrm = np.where(obstacle[:, None], 0.0, nrm)
    return rho, nrm, r, g


def delta_v(ps, mass, h, dt, cohesion, adhesion, obstacle=None, cells=None, rho0=NV.RHO):
    """-> (dv, rho, normals): the velocity increment of the surface-tension pass"""
    n = len(ps)
    obstacle = np.zeros(n, bool) if obstacle is None else np.asarray(obstacle, bool)
    rho, nrm, r, _ = surface_state(ps, mass, h, obstacle, cells)
    fluid = ~obstacle
    d = ps[:, None, :] - ps[None, :, :]                          # x_ij
    within = r <= h
    direct = within & (r >= NV.EPSILON)
    rs = np.where(direct, r, 1.0)
    xhat = np.where(direct[..., None], d / rs[..., None], 0.0)
    K = 2.0 * rho0 / (rho[:, None] + np.where(fluid, rho, 1.0)[None, :])
    ff = fluid[:, None] & fluid[None, :]
    fo = fluid[:, None] & obstacle[None, :]
    coh = np.where(ff & direct, K * cohesion * mass[None, :] * cohesion_kernel(np.where(direct, r, 0.0), h), 0.0)
    adh = np.where(fo & direct, adhesion * mass[None, :] * adhesion_kernel(np.where(direct, r, 0.0), h), 0.0)
    curv = np.where(ff & within, K * cohesion, 0.0)
    f = ((coh + adh)[..., None] * xhat).sum(1) + (curv[..., None] * (nrm[:, None, :] - nrm[None, :, :])).sum(1)
    dv = -dt * f
    dv = np.where(obstacle[:, None], 0.0, dv)
    return dv, rho, nrm


def two_particle_dv(r, h, m, dt, cohesion, rho0=NV.RHO):
    """Closed form for two fluid particles of mass m at distance r <= h, alone: the signed velocity increment of each
    ALONG the unit vector towards the other (> 0: attraction).  rho = m (W(0) + W(r)), K = rho0 / rho, and the two
    normals are opposite: n_1 - n_2 = 2 h (m / rho) spiky (h - r)^2 x_12 / r."""
    rho = m * (float(NV.poly6(np.array(0.0), h)) + float(NV.poly6(np.array(r), h)))
    K = rho0 / rho
    curv = 2.0 * h * (m / rho) * NV.spiky_factor(h) * (h - r) ** 2       # n_1 - n_2 along x_12 / r (negative)
    return dt * K * cohesion * (m * float(cohesion_kernel(r, h)) + curv)
