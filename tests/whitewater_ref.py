"""Reference for pbf_whitewater_step — TEST INFRASTRUCTURE.

Written from the comment in include/pbf_hip.h: numpy float64, every particle against every particle, no table, no sort, no
walk, nothing shared with the library.  Its inputs are what a caller can read back after the steps: download(), pstar(),
keys() and the table's length.

  candidates   j with |cell_j - cell_i| <= 1 per axis, cells decoded from the predict-time keys, key_j + 1 < table length
               (the pbf_sample_points contract: a particle delta-p carried out of its predict-time cell can be missed by
               the library, and is missed here in the same way);
  normals      rho_j = sum over all candidates within h (itself and obstacles included) of m_k W_poly6;
               n_i = h sum over fluid j != i, 1e-8 <= r <= h of (m_j / rho_j) grad W_spiky(x_ij);
  potentials   I_ta, kappa, I_wc, E_k, Phi, n_d as the header states them;
  hash         splitmix64, `unit`;   emission geometry `emit`;   advection rules `advect` (in N: that test is bit for bit).

Error bars (u = eps_N / 2 + eps_64 / 2; every bar is formed from this module's own float64 quantities, none from the device):
  one pair: x_ij per axis 1 rounding, r = sqrt of the sum of squares r (1 + 3.5u), W = 1 - r / h: |dW| <= 6u.
  I_ta     v_ij per axis 1 rounding, |v_ij| (1 + 3.5u); the dot product 5u |v_ij| r, its quotient by |v_ij| r 9u more: the
           cosine carries 14u ABSOLUTE, 1 - cos 15u; term = |v_ij| (1 - cos) W: <= |v_ij| (15 + 2 * 6 + 2 * 5.5)u -> 40u |v_ij|.
           bar = 40u sum |v_ij| + (k + 1) u sum |term|,  k = candidates within h.
  rho_j    tests/test_sample_gpu.py's derivation: 48u cap + (k + 1)u rho, cap = sum m W_poly6(0);  e_j = bar / rho_j.
  n_i      term g = h K (h - r)^2 / r (m_j / rho_j) x_ij per axis: (h - r) carries 4.5u h absolute, its square 9u h (h - r);
           K and the products 16u; m_j / rho_j carries e_j:   |dg| <= h |K| (m_j / rho_j) [(h - r)^2 (16u + e_j) + 9u h (h - r)]
           dn = sqrt(3) (sum |dg| + (k + 1) u sum |g|_inf);   the unit vector moves by at most eps_i = min(2, 2 dn / |n_i|).
  kappa    s = xhat_ji . nhat_i carries eps_i + 12u: a candidate with |s| below that is AMBIGUOUS;
           term (1 - nhat_i . nhat_j) W carries (eps_i + eps_j + 12u) W + 16u;  bar = sum of that + (k + 1) u sum |term|.
  I_wc     vhat_i . nhat_i carries eps_i + 12u: AMBIGUOUS within that of 0.6.
  r at h   a candidate with |r - h| <= 16 eps_N h is AMBIGUOUS.
  E_k      5u relative.   n_d: Phi is Lipschitz with 1 / (tau1 - tau0): dPhi <= dI / (tau1 - tau0) + 4u, product rule, 6u more.
A particle with an ambiguous candidate or test is left out of the comparison; tests cap their share.
"""
import numpy as np

from sample_ref import key_cells

M64 = (1 << 64) - 1
SPRAY, FOAM, BUBBLE = 0, 1, 2
MAX_CHILDREN = 1024


def mix(x):
    x = (int(x) + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def unit(seed, pid, frame, k, s):
    """u for parent id, frame, child k, stream s: 24 bits, exact in float32"""
    w = mix(int(seed) ^ mix(pid) ^ mix(((int(frame) << 32) + int(k) * 4 + int(s)) & M64))
    return (w >> 40) * 2.0 ** -24


def units(seed, ids, frame, k, s):
    return np.array([unit(seed, int(i), frame, k, s) for i in ids], np.float64)


def phi(I, tau):
    return (np.minimum(I, tau[1]) - np.minimum(I, tau[0])) / (tau[1] - tau[0])


def classify(nF, spray_below, bubble_from):
    nF = np.asarray(nF)
    return np.where(nF < spray_below, SPRAY, np.where(nF >= bubble_from, BUBBLE, FOAM)).astype(np.uint8)


def _pairs(ps, keys, table_size, rows):
    """-> (cols, cand, d, r): the block rows x cols of the all-pairs evaluation, cols = the particles that are a candidate of
    at least one of the rows (every other column of the block is excluded from every sum anyway)"""
    cj = key_cells(keys)
    ok = np.asarray(keys, np.int64) + 1 < int(table_size)
    cand = (np.abs(cj[None, :, :] - cj[rows][:, None, :]) <= 1).all(-1) & ok[None, :]
    cols = np.flatnonzero(cand.any(0))
    cand = cand[:, cols]
    d = ps[rows][:, None, :] - ps[cols][None, :, :]
    r = np.sqrt((d * d).sum(-1))
    return cols, cand, d, r


def normals(down, pstar, keys, table_size, h, u, chunk=256):
    """-> rho (n,), e_rho (n,), n (n,3), eps (n,): the surface-tension pass's density and normal, and their error bars"""
    ps = np.asarray(pstar, np.float64)[:, :3]
    mass = np.asarray(down["mass"], np.float64)
    fluid = np.asarray(down["type"]) == 0
    n = len(ps)
    K6, Ks = 315.0 / (64.0 * np.pi * h ** 9), -45.0 / (np.pi * h ** 6)
    rho, cap, cnt = np.zeros(n), np.zeros(n), np.zeros(n)
    for a in range(0, n, chunk):
        rows = np.arange(a, min(n, a + chunk))
        cols, cand, d, r = _pairs(ps, keys, table_size, rows)
        hit = cand & (r <= h)
        rho[rows] = np.where(hit, mass[cols][None, :] * (K6 * (h * h - r * r) ** 3), 0.0).sum(1)
        cap[rows] = np.where(hit, mass[cols][None, :] * (K6 * h ** 6), 0.0).sum(1)
        cnt[rows] = hit.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_rho = np.where(rho > 0, (48 * u * cap + (cnt + 1) * u * rho) / rho, 0.0)
    nrm, dn = np.zeros((n, 3)), np.zeros(n)
    for a in range(0, n, chunk):
        rows = np.arange(a, min(n, a + chunk))
        cols, cand, d, r = _pairs(ps, keys, table_size, rows)
        hit = cand & (r <= h) & (r >= 1e-8) & fluid[cols][None, :] & (cols[None, :] != rows[:, None])
        with np.errstate(divide="ignore", invalid="ignore"):
            mr = np.where(hit, mass[cols][None, :] / rho[cols][None, :], 0.0)
            s = np.where(hit, h * Ks * (h - r) ** 2 / np.where(hit, r, 1.0) * mr, 0.0)
        g = s[..., None] * d
        nrm[rows] = g.sum(1)
        dg = np.where(hit, h * abs(Ks) * mr * ((h - r) ** 2 * (16 * u + e_rho[cols][None, :]) + 9 * u * h * (h - r)), 0.0).sum(1)
        dn[rows] = np.sqrt(3.0) * (dg + (hit.sum(1) + 1) * u * np.abs(g).max(-1).sum(1))
    nrm[~fluid] = 0.0
    nl = np.sqrt((nrm * nrm).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        eps = np.where(nl > 0, np.minimum(2.0, 2.0 * dn / nl), np.where(dn > 0, 2.0, 0.0))
    return rho, e_rho, nrm, eps


def potentials(down, pstar, keys, table_size, h, cfg, dt, frame, dtype, chunk=256):
    """cfg: dict of the pbf_whitewater fields.  -> dict: I_ta, I_wc, E_k, n_d, count (exact floor(n_d + u) of THIS module's
    n_d), bar_* beside each, ambiguous (n,) bool, nbr (fluid candidates within h, itself included), normal (n,3)"""
    eN = float(np.finfo(dtype).eps)
    u = eN / 2 + float(np.finfo(np.float64).eps) / 2
    ps = np.asarray(pstar, np.float64)[:, :3]
    vel = np.asarray(down["vel"], np.float64)
    mass = np.asarray(down["mass"], np.float64)
    fluid = np.asarray(down["type"]) == 0
    n = len(ps)
    rho, e_rho, nrm, eps = normals(down, pstar, keys, table_size, h, u, chunk)
    nl = np.sqrt((nrm * nrm).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        nhat = np.where(nl[:, None] > 0, nrm / nl[:, None], 0.0)
    ita, kappa, bta, bka, nbr = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    amb = np.zeros(n, bool)
    for a in range(0, n, chunk):
        rows = np.arange(a, min(n, a + chunk))
        cols, cand, d, r = _pairs(ps, keys, table_size, rows)
        fl = cand & fluid[cols][None, :]
        nbr[rows] = (fl & (r <= h)).sum(1)
        hit = fl & (r <= h) & (r > 0) & (cols[None, :] != rows[:, None])
        amb[rows] |= (fl & (np.abs(r - h) <= 16 * eN * h)).any(1)
        k = hit.sum(1)
        W = 1.0 - r / h
        vij = vel[rows][:, None, :] - vel[cols][None, :, :]
        vm = np.sqrt((vij * vij).sum(-1))
        with np.errstate(divide="ignore", invalid="ignore"):
            cosv = (vij * d).sum(-1) / (vm * r)
            t = np.where(hit & (vm > 0), vm * (1.0 - cosv) * W, 0.0)
            ita[rows] = t.sum(1)
            bta[rows] = 40 * u * np.where(hit, vm, 0.0).sum(1) + (k + 1) * u * np.abs(t).sum(1)
            s = -(d * nhat[rows][:, None, :]).sum(-1) / r
            have = hit & (nl[rows] > 0)[:, None] & (nl[cols] > 0)[None, :]
            es = (eps[rows] + 12 * u)[:, None]
            amb[rows] |= (have & (np.abs(s) <= es)).any(1)
            w = np.where(have & (s < 0), (1.0 - (nhat[rows][:, None, :] * nhat[cols][None, :, :]).sum(-1)) * W, 0.0)
            kappa[rows] = w.sum(1)
            bka[rows] = np.where(have & (s < 0), (eps[rows][:, None] + eps[cols][None, :] + 12 * u) * W + 16 * u, 0.0).sum(1) + \
                (k + 1) * u * np.abs(w).sum(1)
    v2 = (vel * vel).sum(1)
    vl = np.sqrt(v2)
    with np.errstate(divide="ignore", invalid="ignore"):
        along = np.where((vl > 0) & (nl > 0), (vel * nhat).sum(1) / vl, 0.0)
    moving = (vl > 0) & (nl > 0)
    amb |= moving & (np.abs(along - 0.6) <= eps + 12 * u)
    crest = moving & (along >= 0.6)
    iwc, bwc = np.where(crest, kappa, 0.0), np.where(crest, bka, 0.0)
    ek = mass * v2 * 0.5
    bek = 5 * u * ek
    tta, twc, tk = cfg["tau_ta"], cfg["tau_wc"], cfg["tau_k"]
    pta, pwc, pk = phi(ita, tta), phi(iwc, twc), phi(ek, tk)
    dta, dwc, dk = bta / (tta[1] - tta[0]) + 4 * u, bwc / (twc[1] - twc[0]) + 4 * u, bek / (tk[1] - tk[0]) + 4 * u
    inner = cfg["k_ta"] * pta + cfg["k_wc"] * pwc
    nd = np.where(vl > 0, pk * inner * dt, 0.0)
    bnd = dt * (dk * inner + pk * (cfg["k_ta"] * dta + cfg["k_wc"] * dwc)) + 6 * u * nd
    out = dict(I_ta=ita, I_wc=iwc, E_k=ek, n_d=nd, bar_I_ta=bta, bar_I_wc=bwc, bar_E_k=bek, bar_n_d=bnd, ambiguous=amb,
               nbr=nbr, normal=nrm, kappa=kappa)
    for key in ("I_ta", "I_wc", "E_k", "n_d", "bar_I_ta", "bar_I_wc", "bar_E_k", "bar_n_d"):
        out[key] = np.where(fluid, out[key], 0.0)
    out["ambiguous"] &= fluid
    return out


def counts(n_d, seed, ids, frame, dtype):
    """count_i = min(floor(n_d + u(i, 0)), 1024), formed in N from a given n_d in N"""
    N = np.dtype(dtype).type
    uu = units(seed, ids, frame, 0, 0).astype(dtype)
    c = np.floor((np.asarray(n_d, dtype) + uu).astype(dtype)).astype(np.float64)
    return np.clip(np.nan_to_num(c, nan=0.0), 0, MAX_CHILDREN).astype(np.int64)


def advect(pool, sample, cfg, params, dtype):
    """The advection rules in N (numpy, the header's operation order): pool = dict(pos, vel, life) in N, sample = the dict
    Solver.sample(p, pos, velocity=True) returned on the same state.  -> dict(pos, vel, life, kind, alive)"""
    N = np.dtype(dtype).type
    x, v, life = pool["pos"].astype(dtype), pool["vel"].astype(dtype), pool["life"].astype(dtype)
    dt, scale = N(params.dt), N(params.scale)
    g = np.array(list(params.constant_force), dtype)
    lo, hi = np.array(list(params.min_bound), dtype), np.array(list(params.max_bound), dtype)
    wt = sample["weight"].astype(dtype)
    nF = np.where(wt == 0, 0, sample["count"][:, 0]).astype(np.int64)
    with np.errstate(all="ignore"):
        vf = np.where((nF != 0)[:, None], sample["mv"].astype(dtype) / np.where(wt == 0, N(1), wt)[:, None], N(0)).astype(dtype)
        kind = classify(nF, cfg["spray_below"], cfg["bubble_from"])
        spray = (g * dt + v).astype(dtype)
        b = N(dt * N(-N(cfg["k_b"])))
        bubble = ((v + b * g).astype(dtype) + (N(cfg["k_d"]) * (vf - v).astype(dtype)).astype(dtype)).astype(dtype)
        vn = np.where((kind == SPRAY)[:, None], spray, np.where((kind == BUBBLE)[:, None], bubble, vf)).astype(dtype)
        life = np.where(kind == FOAM, (life - dt).astype(dtype), life).astype(dtype)
        ux = (((vn * dt).astype(dtype) + (x / scale).astype(dtype)).astype(dtype) * scale).astype(dtype)
        # fmax / fmin: a NaN operand gives the other one, as the device's min / max do
        xn = np.fmin(hi, np.fmax(lo, ux)).astype(dtype)
        finite = np.isfinite(ux).all(1) & np.isfinite(vn).all(1)
        wall = (nF == 0) & (xn != ux).any(1)
        alive = (life > 0) & finite & ~wall
    return dict(pos=xn, vel=vn, life=life, kind=kind, alive=alive, nF=nF)


def cylinder(child_pos, child_vel, x, v, h, scale):
    """-> (radial distance from the axis through x along v, axial coordinate, |(v_d - v) . vhat|) in float64"""
    x, v = np.asarray(x, np.float64), np.asarray(v, np.float64)
    vl = np.sqrt((v * v).sum(-1))
    vh = v / vl[:, None]
    d = np.asarray(child_pos, np.float64) - x
    ax = (d * vh).sum(-1)
    rad = np.sqrt(np.maximum(((d - ax[:, None] * vh) ** 2).sum(-1), 0.0))
    dv = np.asarray(child_vel, np.float64) - v
    return rad, ax, np.abs((dv * vh).sum(-1)), vl


def mutate_head_on(v=1.0, r=0.05, h=0.1):
    """two fluid particles approaching head-on along x at speed v each, a distance r apart -> a state for `potentials`"""
    ps = np.array([[1.0, 1.0, 1.0, 0.0], [1.0 + r, 1.0, 1.0, 0.0]])
    down = dict(mass=np.ones(2), type=np.zeros(2, np.uint8), vel=np.array([[v, 0.0, 0.0], [-v, 0.0, 0.0]]),
                id=np.arange(2, dtype=np.uint64))
    return down, ps
