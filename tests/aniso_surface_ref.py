"""Checker for pbf_surface_anisotropic's field — TEST INFRASTRUCTURE.

Written from the section of include/pbf_hip.h alone ("anisotropic-kernel surface"): numpy float64, every node against every
particle, no Morton code, no table, no walk.  Its inputs are what a caller can read back: anisotropy()'s centre, G and radii,
download()'s positions, colours and types, and the predict-time cells as tests/test_mc_field_gpu.py obtains them.  The
lattice geometry is tests/nversion_mc.Lattice (integer decisions in the precision under test, the rest in float64 on inputs
first rounded to it).

  record   e = centre - pos,  disp = |e| / H,  f = max(1, radii_1 / (0.99 - disp)),  G'' = G f / scale,
           D = 1 / (f^3 radii_1 radii_2 radii_3);  an obstacle, a non-finite D / G'' or disp >= 0.99 contributes nothing
  node     the particles whose predict-time cell lies within one cell of the node's on every axis (cells = None: all of them);
           d = a - centre,  y = G'' d,  q2 = |y|^2,  a hit iff q2 < 1;  s = 1 - q2,  t = D s^3,  phi = sum t,
           g = sum (-6 D s^2) G'' y,  C = sum t colour;  stored {phi, -g / |g|}, C / phi;  without a hit all zero
  far      a node with phi == 0 and 6-neighbours with phi > 0: the mean of their colours, order -x +x -y +y -z +z

THE BOUND, counted from the header's expressions (u = the unit round-off of the precision under test).
Node coordinate a: C_COORD = 6 roundings at magnitude <= max|coordinate| (tests/nversion_mc.py counts them).
Record: e_a one rounding; disp = sqrt(three squares, two sums) / H with H = h scale itself rounded: 0.5 (1 + 1 + 2) + 1 + 1 + 1
  -> 5.5 u relative, all terms positive; room = 0.99 - disp (the constant as the precision under test rounds it) carries
  5.5 u disp absolutely and its own rounding, f = radii_1 / room one more: C_F = 5.5 disp / room + 2, relative, PER PARTICLE
  (the difference amplifies disp's error by disp / room; max(1, .) does not increase an error).  f / scale 1, G f' 1 ->
  C_G = C_F + 2, relative, per entry of G''.  D: (f f) f 3 C_F + 2, (r1 r2) r3 2, their product 1, the division 1 ->
  C_D = 3 C_F + 6.
Per pair, per component:  delta d_a = C_COORD u max|coordinate| + u |centre_a|   (absolute)
  and the subtraction's own rounding, u |d_a|, is carried with the relative terms below.
  y_a = (G''_ax d_x + G''_ay d_y) + G''_az d_z: with yabs_a = sum_b |G''_ab| |d_b| (>= |y_a|; equal without cancellation)
      delta y_a <= sum_b |G''_ab| delta d_b + (C_G + 4) u yabs_a          (d 1, G'' C_G, product 1, two sums 2)
  q2 = (y_x^2 + y_y^2) + y_z^2:
      delta q2 <= 2 sum_a |y_a| delta y_a + C_Q u q2,  C_Q = 3             (a square 1, two sums of positives 2)
      — the header form 2 sqrt(q2) |G''| delta d + c_q u q2 with the norms taken entry by entry.
  s = 1 - q2: delta s <= delta q2 + u s.   t = D ((s s) s):
      delta t <= D 3 s^2 delta q2 + C_T u t,  C_T = 3 + 2 + 1 + C_D         (3 u from delta s, two products, the product with D)
  phi: + (n - 1) u sum |t| for n hits.
  k = (-6 D) (s s):  delta k <= 12 D s delta q2 + (C_D + 5) u |k|            (2 u from delta s, -6 D 1, s s 1, product 1)
  z_a = G'' y row:   delta z_a <= sum_b |G''_ab| delta y_b + (C_G + 3) u zabs_a,  zabs_a = sum_b |G''_ab| |y_b|
  term_a = k z_a:    delta <= delta k |z_a| + |k| delta z_a + u |term_a|;  g: + (n - 1) u sum |term_a|
  normal: compared as n_dev |g| against -g with tests/nversion_mc.py's bg_a + |bg| + C_NORM u |g|.
  colour C_c / phi is a weighted mean: an error delta t_j of a weight moves it by delta t_j |colour_j - c| / phi, so
      bc <= min(sum_j delta t_j |colour_jc - c_c| / (phi - bphi), max_j colour_jc - min_j colour_jc) + (n + 3) u max_j colour_jc
      (a mean of positive weights never leaves the range of its values; t colour 1, n - 1 sums, the sum phi's own n - 1
      count in delta t's share, the division 1, rounded up).
Band: a node with a candidate whose |q2 - 1| <= delta q2 — its hit / no-hit pattern rests on a rounding.  Such nodes are left
  out of the bound (never of the NaN check), and the callers cap them at 1 % of the nodes with hits.
The constants are counted, never fitted to the device.  The project's 1e-12 sum|t| bar for fp64 is NOT asserted as well: the
coordinate error is amplified by |G''| |a|, up to about 1e4, and the counted bound is the bar.
"""
import numpy as np

import nversion_mc as NM

OBSTACLE = NM.OBSTACLE
C_Q = 3
SLACK = 1.5
REACH = 0.99

MUTATIONS = ("drop_f", "d_without_f3", "clamp_slots", "g_sign")


def _full(g6):
    g6 = np.asarray(g6, np.float64)
    G = np.empty((len(g6), 3, 3))
    G[:, 0, 0], G[:, 1, 1], G[:, 2, 2] = g6[:, 0], g6[:, 1], g6[:, 2]
    G[:, 0, 1] = G[:, 1, 0] = g6[:, 3]
    G[:, 0, 2] = G[:, 2, 0] = g6[:, 4]
    G[:, 1, 2] = G[:, 2, 1] = g6[:, 5]
    return G


def records(centre, G6, radii, pos, ptype, h, scale, dtype, mutate=None):
    """The per-particle records in float64 from the read-back arrays.  -> dict: centre (P,3), G (P,3,3) = G'', D (P,), f (P,),
    disp (P,), ok (P,) bool (fluid with finite D and G'' and disp < 0.99), rho2 (P,), reach (P,) = (|e| + H radii_1 / f) / H:
    how far the ellipsoid reaches from its particle, in units of H; cG, cD (P,): the rounding counts of the module text.
    dtype: the precision under test (it rounds the constant 0.99)."""
    centre, radii, pos = (np.asarray(a, np.float64) for a in (centre, radii, pos))
    H = float(h) * float(scale)
    e = centre - pos
    dist = np.sqrt((e * e).sum(1))
    disp = dist / H
    room = float(np.dtype(dtype).type(REACH)) - disp
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.maximum(1.0, radii[:, 0] / room)
        cF = 5.5 * disp / room + 2
    fg = np.ones_like(f) if mutate == "drop_f" else f
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        G = _full(G6) * (fg / float(scale))[:, None, None]
        D = 1.0 / ((1.0 if mutate == "d_without_f3" else f ** 3) * radii.prod(1))
        rad = H * radii[:, 0] / f
    ok = (np.asarray(ptype) != OBSTACLE) & (room > 0) & np.isfinite(D) & np.isfinite(G).all((1, 2))
    G, D = np.where(ok[:, None, None], G, 0.0), np.where(ok, D, 0.0)
    return dict(centre=centre, G=G, D=D, f=f, disp=disp, ok=ok, rho2=np.where(ok, rad * rad * SLACK, 0.0),
                reach=np.where(ok, (dist + rad) / H, 0.0), radii=radii, cG=np.where(ok, cF + 2, 0.0), cD=np.where(ok, 3 * cF + 6, 0.0))


def evaluate(rec, colour, cells, lat, dtype, mutate=None):
    """All-pairs float64 field on `lat` with its counted error bounds.  cells (P,3) predict-time, or None for no cell mask.
    -> dict of per-node arrays (index3d order): phi, g (.,3), C (.,4), c (.,4) = C / phi (0 without hits), hits, bphi,
    bg (.,3), bc (.,4), band (bool), pre (the smallest rho2 / |d|^2 over the node's hits, inf without)."""
    u = NM.unit_roundoff(dtype)
    colour = np.asarray(colour, np.float64)
    ok = rec["ok"]
    ctr, G, D = rec["centre"], rec["G"], rec["D"]
    P = len(ctr)
    N = lat.n_nodes
    sx, sy, sz = (int(s) for s in lat.sample)
    out = dict(phi=np.zeros(N), g=np.zeros((N, 3)), C=np.zeros((N, 4)), c=np.zeros((N, 4)), hits=np.zeros(N, np.int64),
               bphi=np.zeros(N), bg=np.zeros((N, 3)), bc=np.zeros((N, 4)), band=np.zeros(N, bool), pre=np.full(N, np.inf))
    if not P or not ok.any():
        return out
    H = lat.threshold
    cmax = max(float(np.abs(ctr).max()), max(float(np.abs(c).max()) for c in lat.coord))
    dd = NM.C_COORD * u * cmax + u * np.abs(ctr)                     # (P,3) delta d_a
    aG = np.abs(G)
    Gdd = np.einsum("pab,pb->pa", aG, dd)                            # sum_b |G''_ab| delta d_b
    if cells is None:
        W = [np.ones((s, P)) for s in (sx, sy, sz)]
    elif mutate == "clamp_slots":
        W = [lat.axis_weight(k, np.asarray(cells)[:, k]).astype(np.float64) for k in range(3)]
    else:
        cells = np.asarray(cells, np.int64)
        W = [(np.abs(lat.node_cell[k][:, None] - cells[None, :, k]) <= 1).astype(np.float64) for k in range(3)]
    sign = +6.0 if mutate == "g_sign" else -6.0
    lo, hi = ctr[ok].min(0) - 1.01 * H, ctr[ok].max(0) + 1.01 * H
    near = [(lat.coord[k] >= lo[k]) & (lat.coord[k] <= hi[k]) for k in range(3)]
    xs = np.nonzero(near[0])[0]
    if len(xs) == 0:
        return out
    ax = lat.coord[0][xs]
    for iz in range(sz):
        for iy in range(sy):
            if not (near[1][iy] and near[2][iz]):
                continue
            wyz = W[1][iy] * W[2][iz]
            ay, az = lat.coord[1][iy], lat.coord[2][iz]
            # (a cull with room to spare: no ellipsoid is longer than H, asserted by the callers through `reach`)
            sub = np.nonzero((wyz > 0) & ok & (np.abs(ctr[:, 1] - ay) <= 1.01 * H) & (np.abs(ctr[:, 2] - az) <= 1.01 * H))[0]
            if len(sub) == 0:
                continue
            idx = lat.index(xs, iy, iz)
            w = W[0][xs][:, sub] * wyz[sub][None, :]                 # [X, S] how often the walk visits the particle
            d = np.empty((len(xs), len(sub), 3))
            d[..., 0] = ax[:, None] - ctr[sub, 0][None, :]
            d[..., 1] = (ay - ctr[sub, 1])[None, :]
            d[..., 2] = (az - ctr[sub, 2])[None, :]
            g, ag = G[sub], aG[sub]
            C_G, C_D = rec["cG"][sub][None, :], rec["cD"][sub][None, :]
            C_T = 3 + 2 + 1 + C_D
            y = np.einsum("sab,xsb->xsa", g, d)
            yabs = np.einsum("sab,xsb->xsa", ag, np.abs(d))
            q2 = (y * y).sum(-1)
            dy = Gdd[sub][None] + ((C_G + 4) * u)[..., None] * yabs
            dq2 = 2 * (np.abs(y) * dy).sum(-1) + C_Q * u * q2
            cand = w > 0
            hit = cand & (q2 < 1.0)
            out["band"][idx] = (cand & (np.abs(q2 - 1.0) <= dq2)).any(1)
            if not hit.any():
                continue
            s = np.where(hit, 1.0 - q2, 0.0)
            Ds = D[sub][None, :]
            t = w * Ds * s ** 3
            dt = w * (Ds * 3 * s * s * dq2 + C_T * u * Ds * s ** 3)
            n = (w * hit).sum(1)
            nm1 = np.maximum(n - 1, 0)
            z = np.einsum("sab,xsb->xsa", g, y)
            zabs = np.einsum("sab,xsb->xsa", ag, np.abs(y))
            k = sign * Ds * s * s
            dk = 12 * Ds * s * dq2 + (C_D + 5) * u * np.abs(k)
            dz = np.einsum("sab,xsb->xsa", ag, dy) + ((C_G + 3) * u)[..., None] * zabs
            term = (w * k)[..., None] * z
            dterm = w[..., None] * (dk[..., None] * np.abs(z) + np.abs(k)[..., None] * dz) + u * np.abs(term)
            col = colour[sub]
            phi = t.sum(1)
            bphi = dt.sum(1) + nm1 * u * np.abs(t).sum(1)
            C = np.einsum("xs,sc->xc", t, col)
            with np.errstate(divide="ignore", invalid="ignore"):
                c = np.where(phi[:, None] > 0, C / phi[:, None], 0.0)
                first = np.einsum("xs,xsc->xc", dt, np.abs(col[None] - c[:, None, :])) / np.maximum(phi - bphi, 0.0)[:, None]
            cmx = np.where(hit[..., None], col[None], -np.inf).max(1)
            cmn = np.where(hit[..., None], col[None], np.inf).min(1)
            any_hit = hit.any(1)
            rng = np.where(any_hit[:, None], cmx - cmn, 0.0)
            bc = np.minimum(np.where(np.isnan(first), np.inf, first), rng) + (n[:, None] + 3) * u * np.where(any_hit[:, None], cmx, 0.0)
            out["phi"][idx], out["bphi"][idx] = phi, bphi
            out["g"][idx] = term.sum(1)
            out["bg"][idx] = dterm.sum(1) + nm1[:, None] * u * np.abs(term).sum(1)
            out["C"][idx], out["c"][idx], out["bc"][idx] = C, c, bc
            out["hits"][idx] = hit.sum(1)
            with np.errstate(divide="ignore"):
                out["pre"][idx] = np.where(hit, rec["rho2"][sub][None, :] / (d * d).sum(-1), np.inf).min(1)
    return out


def fill_far(pn, c, sample, dtype):
    """k_mc_fill_far restated on a stored lattice, in the precision under test (sums in the stated order, one division): the
    colours every node with phi == 0 must hold, given the colours of the nodes with phi > 0."""
    sx, sy, sz = (int(s) for s in sample)
    phi = np.asarray(pn)[:, 0].reshape(sx, sy, sz)
    col = np.asarray(c, dtype).reshape(sx, sy, sz, 4)
    src = phi > 0
    acc = np.zeros((sx, sy, sz, 4), dtype)
    cnt = np.zeros((sx, sy, sz), np.int64)
    for axis in range(3):
        for step in (-1, +1):                                        # -x +x -y +y -z +z
            here = [slice(None)] * 3
            there = [slice(None)] * 3
            here[axis], there[axis] = (slice(1, None), slice(None, -1)) if step < 0 else (slice(None, -1), slice(1, None))
            here, there = tuple(here), tuple(there)
            m = src[there]
            acc[here] = np.where(m[..., None], acc[here] + col[there], acc[here])
            cnt[here] += m
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (acc / cnt[..., None].astype(dtype)).astype(dtype)
    want = np.where((cnt > 0)[..., None], mean, np.zeros(4, dtype))
    return want.reshape(-1, 4), (phi.reshape(-1) == 0)


def _ratio(err, bound):
    return NM._ratio(err, bound)


def compare(pn, c, rec, colour, cells, lat, dtype, mutate=None, ev=None):
    """Hold a stored lattice (pn [N,4] = phi, normal; c [N,4]) to the evaluation.  -> report; the callers assert
    worst <= 1, pattern_bad == 0, nan == 0 and left_out <= 0.01 * with_hits."""
    pn, c = np.asarray(pn), np.asarray(c)
    if ev is None:
        ev = evaluate(rec, colour, cells, lat, dtype, mutate=mutate)
    u = NM.unit_roundoff(dtype)
    N = lat.n_nodes
    assert pn.shape == (N, 4) and c.shape == (N, 4), (pn.shape, c.shape, N)
    p64, c64 = pn.astype(np.float64), c.astype(np.float64)
    band = ev["band"]
    plain = (ev["hits"] > 0) & ~band
    empty = (ev["hits"] == 0) & ~band
    # a node without hits: phi == 0 and a zero normal exactly; its colour is k_mc_fill_far's, from the stored lattice itself
    want, zero_phi = fill_far(pn, c, lat.sample, pn.dtype)
    bad = int((pn[empty, 0] != 0).sum() + (pn[empty, 1:] != 0).sum())
    bad += int((pn[zero_phi, 1:] != 0).sum() + (c[zero_phi] != want[zero_phi]).sum())
    rv = _ratio(np.abs(p64[:, 0] - ev["phi"]), ev["bphi"])
    g = ev["g"]
    gl = np.sqrt((g * g).sum(1))
    bgn = np.sqrt((ev["bg"] ** 2).sum(1))
    bn = ev["bg"] + bgn[:, None] + NM.C_NORM * u * gl[:, None]
    rn = _ratio(np.abs(-p64[:, 1:4] * gl[:, None] - g), bn).max(1)
    rc = _ratio(np.abs(c64 - ev["c"]), ev["bc"]).max(1)
    sel = lambda r: float(r[plain].max(initial=0))
    rep = dict(ev=ev, band=band, plain=plain, empty=empty, pattern_bad=bad, nan=int(np.isnan(pn).sum() + np.isnan(c).sum()),
               with_hits=int((ev["hits"] > 0).sum()), left_out=int((band & ((ev["hits"] > 0) | (pn[:, 0] != 0))).sum()),
               rv=sel(rv), rn=sel(rn), rc=sel(rc), node_rv=rv, node_rn=rn, node_rc=rc,
               pre=float(ev["pre"].min(initial=np.inf)))
    rep["worst"] = max(rep["rv"], rep["rn"], rep["rc"])
    return rep


def summary(rep):
    return (f"phi {rep['rv']:.3g} n {rep['rn']:.3g} c {rep['rc']:.3g} left_out {rep['left_out']}/{rep['with_hits']} "
            f"pattern_bad {rep['pattern_bad']} nan {rep['nan']} pre-test margin {rep['pre']:.3g}")
