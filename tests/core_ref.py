"""Value and per-particle rounding bar of lambda and of the delta-p MOVE (new pStar - old pStar) — TEST INFRASTRUCTURE.

The values are tests/nversion.py's (`lambdas`, `delta`: numpy float64 over all pairs), evaluated on the DEVICE'S OWN INPUTS
widened to float64: the pStar, mass and type a caller reads back and, for delta-p, the lambda the device produced; h, scale and
the bounds as the kernels hold them (extras_ref.kernel_inputs).  Input rounding is therefore not charged to the kernel.  From
the second solver iteration on the pairs are masked to the predict-time cells (`cells`, nversion.predict_cells).

The bars continue tests/extras_ref.py: u = eps_N / 2 + eps_64 / 2, g(k) = k u / (1 - k u), and `extras_ref.Pairs` supplies what
pair_geom and the two kernels leave on a pair: sA / sE (value and bar of s = spikyFactor * hr2_over_r), wA / wE (of
poly6Factor * d^3), n_i (candidates within h), near_eps.  No factor is fitted: each count is a number of roundings in the kernel
text, pbf-sph_amd/csrc/pbf_kernels.hpp, named by function.  M = 1 + g(1) below.

LambdaOp::add_bf   s = spikyFactor * hr2_over_r              sE (extras_ref: 8.5 u and the absolute part near r = h)
                   (d_c * s) * RHO_RECIP                     d_c u, the product u, the second product u: 3 u over sE
                                                             |dt_c| <= |d_c| RHO_RECIP (sE + g(3) (sA + sE))
                   d = h*h - r*r;  poly6Factor * (d*d*d)     wE (extras_ref: dd = 9 u h^2 + u d ABSOLUTE, then 5 u)
                   mass * (...)                              1 u over wE:  |dw| <= m_i (wE + g(1) (wA + wE))
                   gx, gy, gz, rho += ...                    n_i additions each: g(n_i) sum (|t| + |dt|), in ANY order — a
                                                             sequential walk, COOP interleaved partial sums and a butterfly
                                                             all add every term into a sum of at most n_i terms
           ::end   norm2 = gx*gx + gy*gy + gz*gz             sum_c (2 |g_c| bg_c + bg_c^2) + g(3) sum_c (|g_c| + bg_c)^2
                   C = rho / RHO - 1                         the quotient u, the difference u, and rho's bar / RHO: ABSOLUTE in
                                                             rho (C cancels): bC = (brho + g(1) (rho + brho)) / RHO + g(1) (|C| + ..)
                   -C / (norm2 + CFM_EPSILON)                D = norm2 + 600: bD = bnorm2 + g(1) (D + bnorm2);  the quotient u:
                                                             blam = (bC + |lam| bD) / (D - bD), times M, + g(1) |lam|
DeltaOp::add_bf    q = poly6Factor d^3 / p6DeltaQ            p6DeltaQ (make_consts, pbf_hip.hip: r = N(0.3 h) u, d = h*h - r*r
                                                             2.4 u of d, d*d*d, the factor's 2 u, the product: 12.2 u) 13 u, the
                                                             quotient u:  qE = wE / p6 + g(14) (wA + wE) / p6
                   q2 = q*q;  q2*q2                          (q + qE)^4 - q^4 + g(3) (q + qE)^4
                   corr = -CorrK * (q2*q2)                   1 more: g(4)
                   (lambda_a + lambda_b + corr)              the lambdas are INPUTS; two additions: g(2) (|la| + |lb| + |corr|)
                   / RHO                                     u:  fE = numE / RHO + g(1) (|num| + numE) / RHO
                   (d_c * s) * factor                        3 u:  |dt_c| <= |d_c| [(sA + sE) (|f| + fE) (1 + g(3)) - sA |f|]
                   ax, ay, az += ...                         n_i additions: g(n_i) sum (|t| + |dt|), in any order
        ::end      (pa + a) * scale                          the sum u |pa + a|, the product u |x|
                   min(maxB, max(minB, x))                   monotone and 1-Lipschitz: the bar passes through unchanged
                   x / scale                                 u |x| / scale
                   bar of the move, per component            ba_c + g(3) (|pa_c| + |a_c| + ba_c): the ABSOLUTE part 3 u |x|
pair_geom (FAST)   d2 = fma(bz, bz, fma(by, by, bx*bx))      2 u of the squares + three roundings: 5 u, as PRECISE
                   rinv = fast_rsq(d2)                       v_rsq_f32: NO COUNT.  fast_rsq(double) = 1 / sqrt: two IEEE roundings
                   r = d2 * rinv                             2.5 + (0 | 2) + 1 = 3.5 | 5.5 u            (PRECISE: 3.5)
                   (hr * hr) * rinv                          1 + 2.5 + (0 | 2) + 1 = 4.5 | 6.5 u        (PRECISE: 5.5)
                   inH: d2 <= h*h                            5 u of d2 and u of h*h: within 3 u of r = h, inside Pairs' 4 u
                   the plain `/` of DeltaOp                  the compiler's IEEE quotient: u, as counted above
                   extras_ref.Pairs(fast=True) carries these counts.  `hold_iterations(allowance=True)` adds
                   extras_ref.fast_allowance of the record's column on top: the project's INHERITED 3e-5 of the column
                   maximum, NOT DERIVED, for the roundings that have no count.  tests/test_core_paths_gpu.py does not use
                   it: every FAST case it runs stays below the derived bar alone (figures at the end).

An obstacle's lambda is 0 and its pStar is kept: value and bar are 0, so only the exact result passes.  A particle with a pair
within 4 u of r = EPSILON (where the spiky term jumps) is AMBIGUOUS and left out, at most extras_ref.AMBIGUOUS_CAP of a scene
by condition; found: 0 on all eight scenes (the coincident pairs of `pile` are at r = 0 exactly, those of `cloud` part at
predict: both far from EPSILON).

`Coop` restates k_gather_from_lists_coop<N, LambdaOp | DeltaOp, K> (PRECISE) operation by operation in N: lane `sub` folds
the entries sub, sub + K, sub + 2 K, ... of the particle's list sequentially from +0, then the __shfl_xor butterfly m = 1, 2, ...
< K, then end().  The list order is FIXED AND WRITTEN DOWN HERE: the candidates inside the particle's 27 predict-time cells with
float64 d2 <= h^2 (1 + 1e-5) (maybe_within_h's bound), itself included, by ascending index in the sorted arrays.  The device's
lists hold the same set but for the quantised filter's margin — entries that add +0 — in walk order; the bar does not depend on
the order, and showing that is what the restatement is for.

Measured on the CPU (tests/test_core_ref_cpu.py: the oracle with device_pow, to which the PRECISE kernels are bit-equal, and
`Coop` at K = 2, 4, 8; eight scenes, both iterations), worst error / bar: fp32 lambda 0.13, move 0.89 (edges257: the rounding
of pStar itself, 3 u |x|, is most of that bar); fp64 lambda 0.05, move 0.29 (Coop).  Six mutations of the evaluation are each
at least 1.1e3 bars out on every scene they apply to.
Measured on an MI355X (tests/test_core_paths_gpu.py: eight scenes, both iterations, coop 0 / 2 / 4 / 8 with split_build 5 and
coop 2 / 4 / 8 with the default build), worst error / DERIVED bar, one lane per particle | cooperative:
  fp32 PRECISE   lambda 0.13 | 0.13   move 0.89 | 0.90          fp64 PRECISE   lambda 0.05 | 0.05   move 0.26 | 0.35
  fp32 FAST      lambda 0.13 | 0.13   move 0.91 | 0.91          fp64 FAST      lambda 0.05 | 0.05   move 0.46 | 0.46
so FAST needs nothing of the inherited allowance.  The fp32 move is close to its bar at every variant for one reason: the
result is a rounded pStar of magnitude 1 to 2, and 3 u |x| is that rounding with the two before it.
"""
import numpy as np

import extras_ref as ER
import nversion as NV

# test_nversion_cpu.scene(base(name)) -> (warm steps before the step under test, constant force); K = 2 solver iterations
# throughout.  cubes1024 after three warm steps has spread out to at most 26 candidates within h; its start lattice, 1.84 x
# the rest density, is the scene with lists on either side of the 40 row slots (432 of 41 .. 57 entries, 592 within 40)
SCENES = {"cubes1024": (3, ER.GRAVITY), "cubes1024_start": (0, ER.GRAVITY), "cloud": (0, ER.GRAVITY),
          "obstacles": (0, ER.GRAVITY), "pile": (0, ER.NO_FORCE), "edges1": (0, ER.NO_FORCE), "edges65": (0, ER.NO_FORCE),
          "edges257": (0, ER.NO_FORCE)}
ITERATIONS = 2
FILTER = 1.00001            # maybe_within_h: d2 <= h^2 (1 + 1e-5)


def base(name):
    """the name test_nversion_cpu.scene knows the scene by"""
    return name.split("_")[0]


def _fluid(n, obstacle):
    return np.ones(n, bool) if obstacle is None else ~np.asarray(obstacle, bool)


def lambdas(P, mass, obstacle=None):
    """-> (lambda (n,), bar (n,), ambiguous (n,))"""
    g = P.g
    fluid = _fluid(len(mass), obstacle)
    lam, rho = NV.lambdas(P.ps, mass, P.h, obstacle, P.cells)
    _, grad = NV.pair_tables(P.ps, P.h, P.cells)
    gs = grad.sum(1) * NV.RHO_RECIP
    del grad
    one = g(1)
    nrm2, bn2a, bn2b = 0.0, 0.0, 0.0
    for c in range(3):
        t = P.ad[c] * (NV.RHO_RECIP * P.sA)
        dt = P.ad[c] * (NV.RHO_RECIP * (P.sE + g(3) * (P.sA + P.sE)))
        bg = dt.sum(1) + g(P.n_i) * (t + dt).sum(1)
        a = np.abs(gs[:, c])
        nrm2 = nrm2 + a * a
        bn2a = bn2a + 2.0 * a * bg + bg * bg
        bn2b = bn2b + (a + bg) ** 2
    bn2 = bn2a + g(3) * bn2b
    dw = mass[:, None] * (P.wE + one * (P.wA + P.wE))
    w = mass[:, None] * P.wA
    brho = dw.sum(1) + g(P.n_i) * (w + dw).sum(1)
    C = rho / NV.RHO - 1.0
    bC = (brho + one * (rho + brho)) / NV.RHO
    bC = bC + one * (np.abs(C) + bC)
    D = nrm2 + NV.CFM_EPSILON
    bD = bn2 + one * (D + bn2)
    al = np.abs(np.where(fluid, -C / D, 0.0))
    bar = (bC + al * bD) / (D - bD) * (1.0 + one) + one * al
    return lam, np.where(fluid, bar, 0.0), P.near_eps & fluid


def delta(P, lam, scale, min_bound, max_bound, obstacle=None):
    """lam: the lambdas the kernel READS (the device's own).  -> (move (n,3), bar (n,3), ambiguous (n,))"""
    n, g = len(lam), P.g
    fluid = _fluid(n, obstacle)
    new, dp = NV.delta(P.ps, lam, P.h, scale, min_bound, max_bound, obstacle, P.cells)
    p6 = float(NV.poly6(np.array(NV.CorrDeltaQ * P.h), P.h))
    q = P.wA / p6
    qE = P.wE / p6 + g(14) * (P.wA + P.wE) / p6
    q4 = q ** 4
    corr = NV.CorrK * q4
    corrE = NV.CorrK * ((q + qE) ** 4 - q4 + g(4) * (q + qE) ** 4)
    del q, qE, q4
    la = np.abs(lam)
    num = np.abs(lam[:, None] + lam[None, :] - corr)
    numE = corrE + g(2) * (la[:, None] + la[None, :] + corr + corrE)
    del corr, corrE
    f = num / NV.RHO
    fE = numE / NV.RHO + g(1) * (num + numE) / NV.RHO
    del num, numE
    T = P.sA * f                                                        # |t_c| = |d_c| T
    dT = (P.sA + P.sE) * (f + fE) * (1.0 + g(3)) - T
    del f, fE
    bar = np.zeros((n, 3))
    for c in range(3):
        ba = (P.ad[c] * dT).sum(1) + g(P.n_i) * (P.ad[c] * (T + dT)).sum(1)
        bar[:, c] = ba + g(3) * (np.abs(P.ps[:, c]) + np.abs(dp[:, c]) + ba)
    return new - P.ps, np.where(fluid[:, None], bar, 0.0), P.near_eps & fluid


# ---- k_gather_from_lists_coop restated in N, operation by operation ---------------------------------------------------------------------

class Coop:
    """The PRECISE pair terms of LambdaOp / DeltaOp::add_bf in N = dtype for every pair, and each particle's list in the order
    the module docstring fixes.  ps, mass: exact in N;  h, scale, the bounds: as the HOST holds them (doubles)."""

    def __init__(self, ps, mass, obstacle, h, cells, dtype):
        self.T = T = np.dtype(dtype)
        self.N = N = T.type
        self.n = n = len(ps)
        self.p, self.m = ps.astype(T), mass.astype(T)
        self.fluid = _fluid(n, obstacle)
        self.hN = hN = N(h)
        pi = N(np.arccos(N(-1)))
        self.K6 = N(float(N(315.0)) / (float(N(64.0) * pi) * float(hN) ** 9))       # make_consts: poly6_factor<N>
        Ks = N(-(float(N(45.0)) / (float(pi) * float(hN) ** 6)))                    # spiky_factor<N>
        cand = np.ones((n, n), bool) if cells is None else (np.abs(cells[:, None, :] - cells[None, :, :]) <= 1).all(-1)
        d64 = ps[:, None, :] - ps[None, :, :]
        listed = cand & ((d64 * d64).sum(-1) <= float(hN) ** 2 * FILTER)
        self.cnt = listed.sum(1)
        width = max(int(self.cnt.max()), 1)
        self.idx = np.argsort(~listed, axis=1, kind="stable")[:, :width]            # the listed candidates first, ascending
        self.valid = np.arange(width)[None, :] < self.cnt[:, None]
        p = self.p
        with np.errstate(all="ignore"):
            b = [p[None, :, c] - p[:, None, c] for c in range(3)]                   # pair_geom: b - a, a - b its negation
            self.d = [-x for x in b]
            r = np.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
            self.inH = cand & (r <= hN)
            self.inS = self.inH & (r >= N(NV.EPSILON))
            hr = hN - r
            self.s = np.where(self.inS, Ks * ((hr * hr) / r), N(0)).astype(T)
            dd = (hN * hN) - r * r
            self.w6 = (self.K6 * (dd * dd * dd)).astype(T)
        assert self.s.dtype == T and self.w6.dtype == T

    def _reduce(self, terms, K, skip_last_stage=False, pad=None):
        """terms (n, n) in N -> lane 0 of the group after the folds and the butterfly.  pad (n,): what a padding entry adds
        when it counts as valid (mutation)"""
        T = self.T
        listed = np.where(self.valid, np.take_along_axis(terms, self.idx, 1), self.N(0)).astype(T)
        lanes = np.zeros((self.n, K), T)
        for sub in range(K):
            cols = listed[:, sub::K]
            if cols.shape[1]:
                lanes[:, sub] = np.cumsum(cols, axis=1, dtype=T)[:, -1]            # sequential, from +0
            if pad is not None:                                                    # its entries: an odd number leaves q1 >= cnt
                mine = np.maximum(self.cnt - sub + K - 1, 0) // K
                lanes[:, sub] = np.where(mine % 2 == 1, lanes[:, sub] + pad, lanes[:, sub])
        stages = [m for m in (1, 2, 4) if m < K]
        for m in stages[:-1] if skip_last_stage else stages:
            lanes = (lanes + lanes[:, np.arange(K) ^ m]).astype(T)
        return lanes[:, 0]

    def lambdas(self, K, skip_last_stage=False, padding_valid=False):
        N, T = self.N, self.T
        with np.errstate(all="ignore"):
            g = [self._reduce(((self.d[c] * self.s) * N(NV.RHO_RECIP)).astype(T), K, skip_last_stage) for c in range(3)]
            w = np.where(self.inH, self.m[:, None] * self.w6, N(0)).astype(T)
            rho = self._reduce(w, K, skip_last_stage, np.diagonal(w).astype(T) if padding_valid else None)
            norm2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2]
            Ci = rho / N(NV.RHO) - N(1)
            lam = -Ci / (norm2 + N(NV.CFM_EPSILON))
        return np.where(self.fluid, lam, N(0)).astype(T)

    def delta(self, lam, scale, min_bound, max_bound, K, skip_last_stage=False):
        """-> new pStar (n,3) in N"""
        N, T, hN = self.N, self.T, self.hN
        lam = lam.astype(T)
        with np.errstate(all="ignore"):
            rq = N(N(NV.CorrDeltaQ) * hN) if T == np.float32 else N(NV.CorrDeltaQ * float(hN))
            dq = (hN * hN) - rq * rq
            p6 = self.K6 * (dq * dq * dq)
            q = self.w6 / p6
            q2 = q * q
            corr = N(-NV.CorrK) * (q2 * q2)
            f = ((lam[:, None] + lam[None, :]) + corr) / N(NV.RHO)
            factor = np.where(self.inS, f, N(0)).astype(T)
            out = np.empty((self.n, 3), T)
            for c in range(3):
                a = self._reduce(((self.d[c] * self.s) * factor).astype(T), K, skip_last_stage)
                x = (self.p[:, c] + a) * N(scale)
                x = np.minimum(N(max_bound[c]), np.maximum(N(min_bound[c]), x))
                out[:, c] = x / N(scale)
        return np.where(self.fluid[:, None], out, self.p).astype(T)


# ---- the stages of one step held to the bars: what the CPU and the GPU test share --------------------------------------------------------

def hold_iterations(stage_lambda, stage_delta, ps0, mass, obstacle, cells, dtype, h, scale, min_bound, max_bound, fast=False,
                    first=None, each=None, allowance=False):
    """stage_lambda() runs one lambda stage and returns the lambdas (n,); stage_delta() one delta-p stage and returns the new
    pStar (n,3).  ps0: pStar after the sort.  first: a dict shared by the callers whose ps0, mass, obstacle and `fast` are equal
    (the pairs and the lambda reference of the first iteration are then computed once and left unchanged).
    each(it, P, lam_in, ps, (lambda, bar, ambiguous), (move, bar, ambiguous)): called after each iteration's bars are taken (the CPU test's restatement and mutations).
    fast: the bars count pair_geom's FAST branch.  allowance: add extras_ref.fast_allowance (inherited, not derived) to them.
    -> [{record, it, ratio, derived, err, ambiguous}]: error / (bar + allowance), error / derived bar alone"""
    ps = np.asarray(ps0, np.float64)
    mass = np.asarray(mass, np.float64)
    fluid = _fluid(len(mass), obstacle)
    out = []

    def record(name, it, got, value, bar, amb):
        keep = fluid & ~amb
        extra = ER.fast_allowance(value) if allowance else 0.0
        ratio, err = ER.worst(got, value, bar, keep, extra)
        derived = ER.worst(got, value, bar, keep)[0]
        exact = np.array_equal(np.asarray(got, np.float64)[~fluid], np.asarray(value, np.float64)[~fluid])   # obstacles: exactly
        out.append(dict(record=name, it=it, ratio=ratio if exact else float("inf"), derived=derived, err=err,
                        ambiguous=int((amb & fluid).sum())))

    for it in range(ITERATIONS):
        cm = None if it == 0 else cells
        if it == 0 and first is not None and "P" in first:
            P, ref = first["P"], first["lambda"]
        else:
            P = ER.Pairs(ps, h, dtype, cm, fast=fast)
            ref = lambdas(P, mass, obstacle)
            if it == 0 and first is not None:
                first["P"], first["lambda"] = P, ref
        lam = np.asarray(stage_lambda()).astype(np.float64)
        record("lambda", it, lam, *ref)
        new = np.asarray(stage_delta()).astype(np.float64)
        ref_move = delta(P, lam, scale, min_bound, max_bound, obstacle)
        record("move", it, new - ps, *ref_move)
        if each is not None:
            each(it, P, lam, ps, ref, ref_move)
        ps = new
    return out
