"""Value and per-particle rounding bar of the six opt-in velocity records — TEST INFRASTRUCTURE.

  omega, confinement increment, XSPH increment      Macklin & Mueller 2013 eq. 15-17: the values come from tests/nversion.py
  rho, n, surface-tension increment                 Akinci et al. 2013:               the values come from tests/surface_tension_ref.py

Everything is numpy float64 over all pairs, on the DEVICE'S OWN INPUTS widened to float64: the pStar, velocity and mass a
caller reads back, and h, dt, gamma, beta as the kernels hold them (rounded to the kernel's type N).  Rounding of the inputs is
therefore not charged to the kernel.  Candidates are the pairs within each other's 27 predict-time cells (`cells`).

How a bar is made (u = eps_N / 2 + eps_64 / 2: one rounding of the kernel plus this module's own; g(k) = k u / (1 - k u) is
the exact first-order count k u with its higher orders).  No factor in it is fitted: each count is a number of roundings in
the kernel text, pbf-sph_amd/csrc/pbf_kernels.hpp, named by function.

pair_geom (PRECISE branch)
  bx = b.x - a.x                                  1 rounding: each d_c carries u
  d2 = bx*bx + by*by + bz*bz                      (2 + 1) u per square, 2 additions: 5 u
  r  = sqrt_rsq(d2) (the IEEE root)               5/2 + 1 = 3.5 u relative, so at most 3.5 u h absolute
  hr = h - r                                      dhr = 3.5 u h + u hr <= 4.5 u h ABSOLUTE: near r = h nothing relative is left
  hr2_over_r = div_seeded(hr * hr, r) (IEEE)      Q = hr^2 / r:  (2 hr + dhr) dhr / r  +  (1 + 3.5 + 1) u Q
make_consts: spiky_factor / poly6_factor          pi in N, the quotient rounded to N: 2 u on either constant

VorticityOp::add_bf       s = spikyFactor * Q: 5.5 + 2 + 1 = 8.5 u, sE = |K| [8.5 u Q + (2 hr + dhr) dhr / r], sA = |K| Q
                          g_c = d_c * s: 2 u;  u_c = v_b - v_a: u;  g_y * u_z: u;  the difference of the two products: u
                          |dt_x| <= (|d_y| |u_z| + |d_z| |u_y|) (sE + 5 u sA);   w_x + t: n_i additions
                          bar = sum_j |dt| + g(n_i) sum_j |t|,  n_i = candidates within h (R = 13.5 in the form (R + n_i) u sum |t|)
VorticityForceOp::add_bf  |omega_b| = sqrt of three squares of INPUTS (the device's own omega): 2.5 u
                          t_c = (d_c * s) * |omega_b|: 2 + 2.5 + 1 = 5.5 u over sE;   eta_c + t: n_i additions
                 ::end    the unit vector of eta moves by at most e = min(2, 2 |d eta| / |eta|) (e = 2 within |d eta| of the
                          EPSILON threshold); len, 1 / len, e_c * inv: 2.5 + 1 + 1 = 4.5 u per component
                          (n_y w_z - n_z w_y) * k: product u, difference u, k = VORTICITY_EPSILON * dt u, product u: 8.5 u with n's
                          bar_x = k [(|w_y| + |w_z|) e + (|n_y w_z| + |n_z w_y|) 8.5 u]  +  u_N |v_new|  (the add into the velocity)
XsphOp::add_bf            d = h*h - r*r: u h^2 + (2 * 3.5 + 1) u r^2 + u d <= dd = 9 u h^2 + u d ABSOLUTE
                          w = poly6Factor * (d*d*d): wE = K6 [(d + dd)^3 - d^3 + (2 + 2 + 1) u (d + dd)^3], wA = K6 d^3
                          (v_b - v_a)_c * w: u + u;   a_c + t: n_i additions;   a_c * C_XSPH: 1 more
                          bar = C [sum |u_c| (wE + 2 u wA) + g(n_i + 1) sum |u_c| wA]  +  u_N |v_new|
SurfaceDensityOp::add_bf  b.m * (poly6Factor * d^3): 1 over wE;   bar = sum m_j (wE + u wA) + g(n_i) rho;   e_j = bar_j / rho_j
SurfaceNormalOp::add_bf   s = (spikyFactor * Q) * (b.m / b.f.w): the quotient u and the INPUT rho_j e_j, the product u
                          d_c * s: 2 u:   |dt_c| <= |d_c| (m_j / rho_j) (sE + (4 u + e_j) sA);   end: h * n_c 1 more
SurfaceTensionOp::add_bf  K = 2 rho0 / (rho_i + rho_j): eK = (bar_i + bar_j) / (rho_i + rho_j) + 2 u
                          q = (hr*hr*hr) * (r*r*r): qE = r^3 [(hr + dhr)^3 - hr^3] + (2 + 3 * 3.5 + 2 + 1) u (hr + dhr)^3 r^3
                          surface_tension_impl makes cohFactor, h6over64, adhFactor, adhQuad from the DOUBLE h and rounds them:
                          (9 + 1), (6 + 1), (3.25 + 1), (1 + 1) u against the same formulas at h in N
                          coh = cohFactor * (q | 2 q - h6over64): F (qE | 2 qE + 7 u h^6 / 64 + u |2 q - h^6 / 64|) + 11 u |coh|
                          x = fma(adhQuad * r, r, fma(6, r, -2 h)): dx = 10 u 4 r^2 / h + 3.5 u 6 r + u |6 r - 2 h| + u |x|
                          adh = adhFactor * x^(1/4) by two roots: x^(1/4) has an infinite slope at x = 0 (r = h / 2 and r = h), so
                          its bar is the SPAN (x + dx)^(1/4) - max(x - dx, 0)^(1/4), + 2.5 u; adhFactor and the product 5.25 u
                          radial = gamma * (K * m) * coh: eK + 3 u  |  beta * m * adh: 2 u;   t = radial / r: 3.5 + 1;  t * d_c: 2:  6.5 u
                          k (n_i - n_j)_c: the INPUT normals' bars bn_i + bn_j, the difference u, K eK, the product u
                 ::end    dt * s_c: 1;  (dt * gamma) * c_c: 2;  their sum: 1;  the add into the velocity u_N |v_new|
PBF_FLAG_FAST_MATH        v_rsq / v_rcp have no rounding count.  Under it every bar gets 3e-5 of the record's column maximum
                          more: INHERITED from the whitewater, sampling and diagnostics tests, not derived (`fast_allowance`).
                          tests/test_extras_paths_gpu.py prints what the fast kernels need of the derived bar alone (measured
                          on an MI355X: at most 0.62 of it, XSPH; every other record below 0.16), so it can be tightened.

A pair within 4 u of r = h counts with the pairs inside (both sides of the test are then covered: every term is continuous
there); a pair within 4 u of r = EPSILON, where the spiky term jumps, makes its walker AMBIGUOUS, and so does a confinement
increment whose bar exceeds half its own length (N = eta / |eta| where eta = grad |omega| nearly vanishes).

`emulate_surface` restates the three Akinci passes operation by operation in N (numpy, sequential sums): the oracle has no
surface tension, so this is what the CPU test holds the three surface bars to before a device sees them.  It is a weaker
witness than the oracle is for the Macklin ops: written beside the bars, its float64 fma one rounding off the device's, its
sums in index order and not in the walk's.  The check of those three bars that counts is the device's own, in
tests/test_extras_paths_gpu.py.
"""
import numpy as np

import nversion as NV
import surface_tension_ref as ST

FAST_ALLOWANCE = 3e-5
AMBIGUOUS_CAP = 0.02       # tests/test_whitewater_gpu.py's
GAMMA, BETA = 0.05, 0.5    # tests/test_surface_tension_gpu.py's calibration
# test_nversion_cpu.scene(name) -> (solver iterations, warm steps before the step under test, constant force)
GRAVITY, NO_FORCE = (0.0, 9.8, 0.0), (0.0, 0.0, 0.0)
SCENES = {"obstacles_moving": (2, 3, GRAVITY), "cloud": (2, 0, GRAVITY), "pile": (0, 0, NO_FORCE),
          "edges1": (0, 0, NO_FORCE), "edges65": (0, 0, NO_FORCE), "edges257": (0, 0, NO_FORCE)}


def kernel_inputs(dtype, h, dt, gamma=0.0, beta=0.0):
    """h, dt, gamma, beta as the kernels hold them: rounded to N, widened"""
    N = np.dtype(dtype).type
    return float(N(h)), float(N(dt)), float(N(gamma)), float(N(beta))


def fast_allowance(value):
    v = np.abs(np.asarray(value, np.float64))
    return FAST_ALLOWANCE * (v.max(0) if v.size else 0.0)


class Pairs:
    """The all-pairs geometry every record shares, with the pair-term bars of pair_geom and of the two kernels."""

    def __init__(self, ps, h, dtype, cells=None, fast=False):
        """fast: the counts of pair_geom's FAST branch in place of the PRECISE ones (tests/core_ref.py lists them); the six
        records of this module keep the PRECISE counts under PBF_FLAG_FAST_MATH too, as they were validated"""
        self.h, self.dtype = h, np.dtype(dtype)
        self.uN = float(np.finfo(dtype).eps) / 2
        self.u = u = self.uN + float(np.finfo(np.float64).eps) / 2
        self.ps, self.cells = ps, cells
        # roundings of r and of Q = (h - r)^2 / r after d2's 5 u (2.5 u once the root is taken)
        rsq = 2.0 if self.dtype == np.float64 else 0.0           # fast_rsq(double) = 1 / sqrt: two; v_rsq_f32: no count
        self.cr, self.cQ = (2.5 + rsq + 1.0, 1.0 + 2.5 + rsq + 1.0) if fast else (3.5, 5.5)
        d = ps[:, None, :] - ps[None, :, :]
        r = np.sqrt((d * d).sum(-1))
        if cells is not None:
            r = np.where((np.abs(cells[:, None, :] - cells[None, :, :]) <= 1).all(-1), r, np.inf)
        self.ad = [np.abs(d[..., c]) for c in range(3)]
        self.r = r
        self.inH = r <= h * (1.0 + 4.0 * u)
        self.spiky = self.inH & (r >= NV.EPSILON * (1.0 - 4.0 * u))
        self.near_eps = (np.abs(r - NV.EPSILON) <= 4.0 * u * NV.EPSILON).any(1)
        self.n_i = self.inH.sum(1).astype(np.float64)
        rs = np.where(self.spiky, r, 1.0)
        self.rs = rs
        hr = np.where(self.spiky, np.maximum(h - r, 0.0), 0.0)
        self.hr, self.dhr = hr, (self.cr + 1.0) * u * h
        K = abs(NV.spiky_factor(h))
        Q = hr * hr / rs
        self.sA = K * Q
        self.sE = np.where(self.spiky, K * (self.g(self.cQ + 3.0) * Q + (2.0 * hr + self.dhr) * self.dhr / rs), 0.0)
        d2 = np.where(self.inH, np.maximum(h * h - np.where(self.inH, r, 0.0) ** 2, 0.0), 0.0)
        dd = (2.0 * self.cr + 2.0) * u * h * h + u * d2
        K6 = NV.poly6_factor(h)
        self.wA = K6 * d2 ** 3
        self.wE = np.where(self.inH, K6 * ((d2 + dd) ** 3 - d2 ** 3 + self.g(5) * (d2 + dd) ** 3), 0.0)

    def g(self, k):
        k = np.asarray(k, np.float64)
        return k * self.u / (1.0 - k * self.u)


def _fluid(n, obstacle):
    return np.ones(n, bool) if obstacle is None else ~np.asarray(obstacle, bool)


def vorticity(P, vel, obstacle=None):
    """-> (omega (n,3), bar (n,3), ambiguous (n,))"""
    value = NV.vorticity(P.ps, vel, P.h, P.cells, obstacle=obstacle)
    au = [np.abs(vel[None, :, c] - vel[:, None, c]) for c in range(3)]
    bar = np.zeros_like(value)
    for c in range(3):
        a, b = (c + 1) % 3, (c + 2) % 3
        cr = P.ad[a] * au[b] + P.ad[b] * au[a]
        bar[:, c] = (cr * (P.sE + P.g(5) * P.sA)).sum(1) + P.g(P.n_i) * (cr * P.sA).sum(1)
    fluid = _fluid(len(vel), obstacle)
    return value, np.where(fluid[:, None], bar, 0.0), P.near_eps & fluid


def confinement(P, vel, omega, dt, obstacle=None):
    """omega: the field the force pass READS (the device's own).  -> (increment (n,3), bar (n,3), ambiguous (n,))"""
    fluid = _fluid(len(vel), obstacle)
    value, ln = NV.vorticity_force_dv(P.ps, omega, P.h, dt, P.cells, return_eta=True, obstacle=obstacle)
    mag = np.where(fluid, np.sqrt((omega * omega).sum(-1)), 0.0)
    deta2 = np.zeros(len(vel))
    eta = np.zeros_like(value)
    _, grad = NV.pair_tables(P.ps, P.h, P.cells)
    for c in range(3):
        t = P.ad[c] * mag[None, :]
        be = (t * (P.sE + P.g(5.5) * P.sA)).sum(1) + P.g(P.n_i) * (t * P.sA).sum(1)
        deta2 += be * be
        eta[:, c] = (grad[..., c] * mag[None, :]).sum(1)
    deta = np.sqrt(deta2)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(ln > NV.EPSILON + deta, np.minimum(2.0, 2.0 * deta / ln), np.where(deta > 0, 2.0, 0.0))
        nn = np.where((ln > NV.EPSILON)[:, None], eta / ln[:, None], 0.0)
    k = NV.VORTICITY_EPSILON * dt
    aw, an = np.abs(omega), np.abs(nn)
    bar = np.zeros_like(value)
    for c in range(3):
        a, b = (c + 1) % 3, (c + 2) % 3
        bar[:, c] = k * ((aw[:, a] + aw[:, b]) * e + (an[:, a] * aw[:, b] + an[:, b] * aw[:, a]) * P.g(8.5))
    amb = (np.sqrt((bar * bar).sum(1)) > 0.5 * np.sqrt((value * value).sum(1))) | P.near_eps   # (the direction's part)
    bar += P.uN * (np.abs(vel) + np.abs(value) + bar)
    bar = np.where(fluid[:, None], bar, 0.0)
    return value, bar, amb & fluid


def xsph(P, vel, obstacle=None):
    """-> (increment (n,3), bar (n,3), ambiguous (n,): never)"""
    fluid = _fluid(len(vel), obstacle)
    value = NV.xsph(P.ps, vel, P.h, P.cells, obstacle=obstacle) - vel
    bar = np.zeros_like(value)
    for c in range(3):
        au = np.abs(vel[None, :, c] - vel[:, None, c])
        bar[:, c] = NV.C_XSPH * ((au * (P.wE + P.g(2) * P.wA)).sum(1) + P.g(P.n_i + 1) * (au * P.wA).sum(1))
    bar += P.uN * (np.abs(vel) + np.abs(value) + bar)
    return value, np.where(fluid[:, None], bar, 0.0), np.zeros(len(vel), bool)


def surface(P, vel, mass, dt, gamma, beta, obstacle=None):
    """-> dict(rho, n, dv: (value, bar)), ambiguous (n,)"""
    n, h, u, g = len(vel), P.h, P.u, P.g
    fluid = _fluid(n, obstacle)
    obst = ~fluid
    dv, rho, nrm = ST.delta_v(P.ps, mass, h, dt, gamma, beta, obst, P.cells)
    # density
    bar_rho = (mass[None, :] * (P.wE + u * P.wA)).sum(1) + g(P.n_i) * rho
    bar_rho = np.where(fluid, bar_rho, 0.0)
    rho1 = np.where(fluid, rho, 1.0)
    e = bar_rho / rho1
    e = e / (1.0 - e)
    # normal
    mr = np.where(fluid, mass / rho1, 0.0)
    bar_n = np.zeros_like(nrm)
    for c in range(3):
        t = P.ad[c] * mr[None, :]
        bar_n[:, c] = h * ((t * (P.sE + (g(4) + e)[None, :] * P.sA)).sum(1) + g(P.n_i + 1) * (t * P.sA).sum(1))
    bar_n = np.where(fluid[:, None], bar_n, 0.0)
    # tension
    r, rs, hr, dhr = P.r, P.rs, P.hr, P.dhr
    ff = fluid[:, None] & fluid[None, :]
    fo = fluid[:, None] & obst[None, :]
    rsum = rho1[:, None] + rho1[None, :]
    K = 2.0 * NV.RHO / rsum
    eK = (bar_rho[:, None] + bar_rho[None, :]) / rsum
    eK = eK / (1.0 - eK) + g(2)
    r3 = np.where(P.spiky, rs, 0.0) ** 3
    q = hr ** 3 * r3
    qE = r3 * ((hr + dhr) ** 3 - hr ** 3) + g(15.5) * (hr + dhr) ** 3 * r3
    F, c6 = 32.0 / (np.pi * h ** 9), h ** 6 / 64.0
    outer = r > 0.5 * h
    coh = F * np.where(outer, q, 2.0 * q - c6)
    cohE = F * np.where(outer, qE, 2.0 * qE + g(7) * c6 + u * np.abs(2.0 * q - c6)) + g(11) * np.abs(coh)
    rad_f = np.where(ff & P.spiky, gamma * mass[None, :] * K * np.abs(coh), 0.0)
    radE_f = np.where(ff & P.spiky, gamma * mass[None, :] * K * (cohE + np.abs(coh) * (eK + g(3))), 0.0)
    x = -4.0 * rs * rs / h + 6.0 * rs - 2.0 * h
    dx = g(10) * 4.0 * rs * rs / h + g(3.5) * 6.0 * rs + u * np.abs(6.0 * rs - 2.0 * h) + u * np.abs(x)
    supp = fo & P.spiky & (r > 0.5 * h * (1.0 - 8.0 * u))
    xp = np.where(supp, np.maximum(x, 0.0), 0.0)
    Fa = 0.007 / h ** 3.25
    root = xp ** 0.25
    rootE = (xp + dx) ** 0.25 - np.maximum(xp - dx, 0.0) ** 0.25 + g(2.5) * (xp + dx) ** 0.25
    A = Fa * root
    rad_o = np.where(supp, beta * mass[None, :] * A, 0.0)
    radE_o = np.where(supp, beta * mass[None, :] * (Fa * rootE + g(5.25) * A + g(2) * A), 0.0)
    rad, radE = rad_f + rad_o, radE_f + radE_o + (rad_f + rad_o) * g(6.5)
    curv = ff & P.inH & ~np.eye(n, dtype=bool)
    kk = np.where(curv, K, 0.0)
    bar_dv = np.zeros_like(dv)
    for c in range(3):
        dirn = P.ad[c] / rs
        S_P, S_E = (dirn * rad).sum(1), (dirn * radE).sum(1)
        dn = np.abs(nrm[:, None, c] - nrm[None, :, c])
        C_P = (kk * dn).sum(1)
        C_E = (kk * (bar_n[:, None, c] + bar_n[None, :, c] + dn * (eK + g(2)))).sum(1)
        bar_dv[:, c] = dt * (S_E + g(P.n_i + 2) * S_P) + dt * gamma * (C_E + g(P.n_i + 3) * C_P)
    bar_dv += P.uN * (np.abs(vel) + np.abs(dv) + bar_dv)
    bar_dv = np.where(fluid[:, None], bar_dv, 0.0)
    return dict(rho=(rho, bar_rho), n=(nrm, bar_n), dv=(dv, bar_dv)), P.near_eps & fluid


def worst(got, value, bar, keep, extra=0.0):
    """-> (largest error / bar over the kept rows, largest error): a zero bar allows only a zero error, and a result, a
    value or a bar that is not finite on a kept row is infinitely far out (never "no error")"""
    got, value, bar = (np.asarray(a, np.float64).reshape(len(keep), -1) for a in (got, value, bar))
    err = np.abs(got - value)[keep]
    b = (bar + np.asarray(extra, np.float64).reshape(1, -1))[keep]
    if err.size == 0:
        return 0.0, 0.0
    if not (np.isfinite(err).all() and np.isfinite(b).all()):
        return float("inf"), float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / b)
    return float(ratio.max()), float(err.max())


# ---- the three Akinci passes restated in N, operation by operation (CPU validation of the surface bars) ---------------------------------

def emulate_surface(ps, vel, mass, obstacle, h, dt, gamma, beta, cells, dtype):
    """SurfaceDensityOp, SurfaceNormalOp, SurfaceTensionOp (PRECISE) in N = dtype: every operation of add_bf and end() in
    the order of the kernel text, IEEE root and quotient where the kernel's seeded forms equal them, the running sums
    sequential over the candidates in index order.  ps, vel, mass: exact in N; h, dt, gamma, beta: as the HOST holds them
    (doubles).  -> rho (n,), n (n,3), velocity increment (n,3), all in N"""
    T = np.dtype(dtype)
    N = T.type
    n = len(ps)
    p, v, m = ps.astype(T), vel.astype(T), mass.astype(T)
    hN, dtN, gN, bN = N(h), N(dt), N(gamma), N(beta)
    pi = N(np.arccos(N(-1)))
    K6 = N(float(N(315.0)) / (float(N(64.0) * pi) * float(hN) ** 9))      # make_consts: poly6_factor<N>
    Ks = N(-(float(N(45.0)) / (float(pi) * float(hN) ** 6)))               # spiky_factor<N>
    h = float(h)                                                           # surface_tension_impl: from the double h
    cohF, c6 = N(32.0 / (np.pi * h ** 9)), N(h ** 6 / 64.0)
    adhF, adhQ = N(0.007 / h ** 3.25), N(-4.0 / h)
    cand = np.ones((n, n), bool) if cells is None else (np.abs(cells[:, None, :] - cells[None, :, :]) <= 1).all(-1)
    fluid = ~np.asarray(obstacle, bool)

    def seq(t):                                                            # a running sum in N, candidate by candidate
        return np.cumsum(t, axis=1, dtype=T)[:, -1]

    with np.errstate(all="ignore"):
        b = [p[None, :, c] - p[:, None, c] for c in range(3)]              # pair_geom: b - a, a - b its negation
        d = [-x for x in b]
        r = np.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
        inH = cand & (r <= hN)
        inS = inH & (r >= N(NV.EPSILON))
        hr = hN - r
        Q = (hr * hr) / r
        dd = (hN * hN) - r * r
        w = m[None, :] * (K6 * (dd * dd * dd))
        rho = np.where(fluid, seq(np.where(inH, w, N(0))), N(0)).astype(T)
        s = np.where(inS & fluid[None, :], (Ks * Q) * (m[None, :] / rho[None, :]), N(0)).astype(T)
        nrm = np.stack([hN * seq(d[c] * s) for c in range(3)], -1)
        nrm = np.where(fluid[:, None], nrm, N(0)).astype(T)
        outer = r > N(0.5) * hN
        q = (hr * hr * hr) * (r * r * r)
        coh = cohF * np.where(outer, q, N(2) * q - c6)
        # fma(adhQuad * r, r, fma(6, r, -2 h)): each fma rounds once.  Formed in float64 and rounded to N: the products are
        # exact for N = float32; for N = float64 this is one rounding more than the device, inside the bar's own u
        r64 = r.astype(np.float64)
        inner = (6.0 * r64 + np.float64(N(-2) * hN)).astype(T)
        x = ((adhQ * r).astype(np.float64) * r64 + inner.astype(np.float64)).astype(T)
        adh = adhF * np.sqrt(np.sqrt(np.maximum(x, N(0))))
        K = N(2.0 * NV.RHO) / (rho[:, None] + rho[None, :])
        radial = np.where(fluid[None, :], gN * (K * m[None, :]) * coh, np.where(outer, bN * m[None, :] * adh, N(0)))
        t = np.where(inS, radial / r, N(0)).astype(T)
        k = np.where(inH & fluid[None, :], K, N(0)).astype(T)
        kc = dtN * gN
        out = np.zeros((n, 3), T)
        for c in range(3):
            sc = seq(t * d[c])
            cc = seq(k * (nrm[:, None, c] - nrm[None, :, c]))
            out[:, c] = v[:, c] - (dtN * sc + kc * cc)
    out = np.where(fluid[:, None], out, v)
    return rho, nrm, (out.astype(np.float64) - v.astype(np.float64)).astype(np.float64)
