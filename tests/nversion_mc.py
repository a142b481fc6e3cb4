"""The marching-cubes field, restated in numpy float64 from the reference's text alone
(ompsph.hpp:277-356, sph.hpp:198-201), with no Morton code, no sort and no cell table.

It was written without looking at pbf_mc.hpp or at pbf_oracle.cpp::mc_field: what the
reference's 27-slot walk over a sorted table amounts to is stated here as a *weight* per pair, and the
sums are taken over all pairs.

What the reference does at a lattice node (x, y, z):
  a       = (minExtent + pos*step) * scale,  step = h / resolution,  minExtent = minBound/scale - 2h
  z_axis  = trunc(pos_axis / resolution)                       the node's cell
  slots   = {clamp(z-1), z, clamp(z+1)} per axis, the outer two clamped to [0, extent-1], the centre not
  walk    = the 27 products of the slots; a particle is visited once per slot triple that names its
            predict-time cell => weight = prod_axis #(slots equal to the particle's cell coordinate)
  hit     = type != Obstacle and len < threshold (strict), threshold = h*scale, l = p - a, len = |l|
  v      += size / len^infl
  normal += (-infl)*size * (l / len^infl)            => points away from the fluid
  colour += colour_b ;  n += 1
  out     = v, normal/|normal| (0 * inf = NaN without hits), colour / n (0/0 = NaN without hits)
The one node whose cell is (extent.x, extent.y, extent.z) returns early and keeps its zero initialisation.

Particles whose predict-time cell lies outside [0, extent-1] on some axis are outside this restatement:
the callers assert that their scenes have none (Morton codes are monotone per coordinate, so every cell
inside has a code below the table length and the reference's `offset >= tableN` test never drops one).

Integer decisions (extent, sample size, node cell) are taken in the precision under test, because a
truncation is not continuous; everything else is float64 on inputs first rounded to that precision, so
that the float64 value is the exact value of the expression the precision under test rounds.
"""
import numpy as np

OBSTACLE = 1  # sph.hpp:15  enum class Type : uint8_t { Fluid = 0, Obstacle = 1 }

# Rounding counts, read off the reference's expressions (ompsph.hpp:132-135, 290-291, 337-343).
#   a = (minExtent + pos*step) * scale:
#       step = h/res (1), pos*step (1), minBound/scale (1), - padding (1; padding = h*2 is exact),
#       minExtent + . (1), * scale (1)                                   => 6 roundings at magnitude <= max|a|
#   l = p - a (1, relative to |l_i| <= len; counted in C_LEN)
C_COORD = 6
#   len = sqrt(lx*lx + ly*ly + lz*lz): subtraction (1), squares (1 on len^2 = 1/2 on len), two sums (2 on
#       len^2 = 1 on len), sqrt (1)                                      => 3.5, rounded up
C_LEN = 4
#   v term = size / denom: one division.
C_V_OPS = 1
#   gradient term = ((-infl)*size) * (l_i / denom): constant product (1), division (1), product (1).
C_G_OPS = 3
#   pow: 1 where the implementation takes the correctly rounded square root (infl == 0.5).  Otherwise the
#   device's pow: the ROCm documentation installed with the toolchain states no ulp bound for pow/powf, so
#   the OpenCL full-profile bound of 16 ulp is used.
C_POW_SQRT = 1
C_POW = 16


def unit_roundoff(dtype):
    return float(np.finfo(dtype).eps) / 2


def _r(x, dtype):
    """x rounded to the precision under test, as float64."""
    return np.asarray(x, dtype=dtype).astype(np.float64)


class Lattice:
    """The reference's lattice geometry for one configuration."""

    def __init__(self, h, scale, min_bound, max_bound, resolution, dtype):
        t = np.dtype(dtype).type
        hb, sc, res = t(h), t(scale), t(resolution)
        mn, mx = np.asarray(min_bound, dtype), np.asarray(max_bound, dtype)
        pad = hb * t(2)
        min_e = mn / sc - pad
        max_e = mx / sc + pad
        self.dtype = np.dtype(dtype)
        self.extent = ((max_e - min_e) / hb).astype(np.int64)              # trunc: the values are positive
        self.sample = np.floor(self.extent.astype(dtype) * res).astype(np.int64) + 1
        # node cell per axis, in the precision under test (pos / resolution, truncated)
        self.node_cell = [(np.arange(s).astype(dtype) / res).astype(np.int64) for s in self.sample]
        # float64 from here on, on the rounded inputs
        self.h, self.scale, self.res = float(hb), float(sc), float(res)
        self.min_e = _r(mn, dtype) / self.scale - 2.0 * self.h
        self.step = self.h / self.res
        self.threshold = self.h * self.scale
        self.coord = [(self.min_e[k] + np.arange(self.sample[k], dtype=np.float64) * self.step) * self.scale
                      for k in range(3)]
        self.n_nodes = int(np.prod(self.sample))

    def index(self, x, y, z):
        """utils.hpp:81 index3d(x, y, z, sx, sy, sz) = x*sy*sz + y*sz + z: z fastest."""
        return (x * self.sample[1] + y) * self.sample[2] + z

    def slots(self, axis, clamp_centre=False):
        """[3, sample] the three slot cells of every node index on one axis."""
        z = self.node_cell[axis]
        hi = self.extent[axis] - 1
        c = np.clip(z, 0, hi) if clamp_centre else z
        return np.stack([np.clip(z - 1, 0, hi), c, np.clip(z + 1, 0, hi)])

    def axis_weight(self, axis, cells, clamp_centre=False, unit=False):
        """[sample, P] how often each particle's cell coordinate occurs among the node's three slots."""
        s = self.slots(axis, clamp_centre)
        w = (s[:, :, None] == np.asarray(cells)[None, None, :]).sum(axis=0)
        return np.minimum(w, 1) if unit else w


def evaluate(pos, colour, ptype, cells, lat, size, infl, *, mutate=None, band=None):
    """All-pairs float64 field on lattice `lat`.

    pos [P,3], colour [P,4], ptype [P], cells [P,3] (predict-time).  Returns a dict of [n_nodes] arrays
    (index3d order, z fastest): v, g [.,3] (un-normalised gradient), nrm [.,3], csum [.,4], c [.,4], n (sum of weights),
    hits (pairs), sv = sum w|t_v|, sv_len = sum w|t_v|/len, sg [.,3] = sum w|t_g|, sg_len [.,3] = sum
    w|t_g|/len, sinv = sum w/len^infl, gap = min |len - threshold| over the visible non-obstacle
    candidates, wmax (largest weight among the hits), evaluated (bool).

    mutate: None or one of 'unit_weight', 'le', 'obstacles', 'drop_smallest', 'flip_sign', 'clamp_centre':
    deliberate defects, used to show that the bound bites.
    band: None, or (delta, 'in' | 'out'): pairs with |len - threshold| <= delta are all taken / all left.
    """
    pos = np.asarray(pos, np.float64)
    colour = np.asarray(colour, np.float64)
    ptype = np.asarray(ptype)
    cells = np.asarray(cells, np.int64)
    P = len(pos)
    sx, sy, sz = (int(s) for s in lat.sample)
    N = lat.n_nodes
    thr = lat.threshold
    out = dict(v=np.zeros(N), g=np.zeros((N, 3)), csum=np.zeros((N, 4)), n=np.zeros(N),
               hits=np.zeros(N, np.int64), sv=np.zeros(N), sv_len=np.zeros(N), sg=np.zeros((N, 3)),
               sg_len=np.zeros((N, 3)), sinv=np.zeros(N), gap=np.full(N, np.inf), wmax=np.zeros(N),
               evaluated=np.zeros(N, bool))
    cc = mutate == "clamp_centre"
    uw = mutate == "unit_weight"
    W = [lat.axis_weight(k, cells[:, k], cc, uw).astype(np.float64) for k in range(3)] if P else None
    visible = np.ones(P, bool) if mutate == "obstacles" else (ptype != OBSTACLE)
    sign = +1.0 if mutate == "flip_sign" else -1.0
    if P:
        lo, hi = pos.min(axis=0) - thr, pos.max(axis=0) + thr
        near = [(lat.coord[k] >= lo[k]) & (lat.coord[k] <= hi[k]) for k in range(3)]
    for iz in range(sz):
        for iy in range(sy):
            if not P or not (near[1][iy] and near[2][iz]):
                continue
            xs = np.nonzero(near[0])[0]
            if len(xs) == 0:
                continue
            idx = lat.index(xs, iy, iz)
            out["evaluated"][idx] = True
            wyz = W[1][iy] * W[2][iz]
            sub = np.nonzero((wyz > 0) & visible)[0]
            if len(sub) == 0:
                continue
            w = W[0][xs][:, sub] * wyz[sub][None, :]                     # [X, S]
            lx = pos[sub, 0][None, :] - lat.coord[0][xs][:, None]
            ly = (pos[sub, 1] - lat.coord[1][iy])[None, :]
            lz = (pos[sub, 2] - lat.coord[2][iz])[None, :]
            ln = np.sqrt(lx * lx + ly * ly + lz * lz)
            cand = w > 0
            if band is not None:
                inb = np.abs(ln - thr) <= band[0]
                hit = cand & ((ln < thr) | inb if band[1] == "in" else (ln < thr) & ~inb)
            elif mutate == "le":
                hit = cand & (ln <= thr)
            else:
                hit = cand & (ln < thr)
            gap = np.where(cand, np.abs(ln - thr), np.inf).min(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = np.where(hit, 1.0 / ln ** infl, 0.0)               # 1/len^infl; +inf on a node
                wt = np.where(hit, w, 0.0)
                tv = np.where(hit, wt * size * inv, 0.0)
                if mutate == "drop_smallest":
                    big = np.where(hit, tv, np.inf)
                    j = big.argmin(axis=1)
                    rows = np.nonzero(hit.any(axis=1))[0]
                    keep = np.ones_like(hit)
                    keep[rows, j[rows]] = False
                    hit = hit & keep
                    inv, wt, tv = inv * keep, wt * keep, np.where(keep, tv, 0.0)
                L = np.stack([np.broadcast_to(lx, ln.shape), np.broadcast_to(ly, ln.shape),
                              np.broadcast_to(lz, ln.shape)], axis=-1)  # [X, S, 3]
                tg = np.where(hit[..., None], (sign * infl * size) * wt[..., None] * (L * inv[..., None]), 0.0)
                rl = np.where(hit, 1.0 / ln, 0.0)
                out["v"][idx] = tv.sum(axis=1)
                out["g"][idx] = tg.sum(axis=1)
                out["csum"][idx] = (wt[..., None] * colour[sub][None, :, :]).sum(axis=1)
                out["n"][idx] = wt.sum(axis=1)
                out["hits"][idx] = hit.sum(axis=1)
                out["sv"][idx] = np.abs(tv).sum(axis=1)
                out["sv_len"][idx] = np.where(hit, np.abs(tv) * rl, 0.0).sum(axis=1)
                out["sg"][idx] = np.abs(tg).sum(axis=1)
                out["sg_len"][idx] = np.where(hit[..., None], np.abs(tg) * rl[..., None], 0.0).sum(axis=1)
                out["sinv"][idx] = (wt * inv).sum(axis=1)
                out["gap"][idx] = gap
                out["wmax"][idx] = wt.max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = out["g"]
        inv_len = 1.0 / np.sqrt((g * g).sum(axis=1))                     # 1/0 = inf => 0 * inf = NaN
        out["nrm"] = g * inv_len[:, None]
        out["c"] = out["csum"] / out["n"][:, None]                       # 0/0 = NaN
    # ompsph.hpp:301-304: the one node whose cell is the extent on all three axes keeps its zeros
    corner = [np.nonzero(lat.node_cell[k] == lat.extent[k])[0] for k in range(3)]
    for x in corner[0]:
        for y in corner[1]:
            for z in corner[2]:
                i = lat.index(x, y, z)
                for key in ("v", "n", "sv", "sv_len", "sinv", "wmax"):
                    out[key][i] = 0
                out["hits"][i] = 0
                for key in ("g", "nrm", "csum", "c", "sg", "sg_len"):
                    out[key][i] = 0
                out["gap"][i] = np.inf
                out["early"] = int(i)
    return out


def bounds(ev, lat, pos, size, infl, dtype):
    """Per-node error bounds for an implementation in `dtype`, from the evaluation's own quantities.

    One term t = size/len^infl evaluated in precision u:
        |dt| <= t * (infl * dlen/len + (c_pow + C_V_OPS) * u)
        dlen <= sqrt(3) * C_COORD * u * max|coordinate|  +  C_LEN * u * len
    (the node coordinate's roundings are absolute at the coordinate's magnitude and the subtraction loses
    them against len; the second part is relative to len).  A sum of n additions adds (n - 1) * u * sum|t|;
    a term of weight w is added w times, so n is the sum of weights.
    A gradient term t_i = -infl*size * l_i/len^infl also carries the absolute error of l_i itself:
        |dt_i| <= infl*size/len^infl * da  +  |t_i| * (infl * dlen/len + (c_pow + C_G_OPS + 1) * u)
    with da = C_COORD * u * max|coordinate| and the +1 for the subtraction's own rounding.
    Returns dict: u, da, dlen0 (the absolute part of dlen), bv [N], bg [N,3], c_pow.
    """
    u = unit_roundoff(dtype)
    c_pow = C_POW_SQRT if infl == 0.5 else C_POW
    cmax = max(float(np.abs(np.asarray(pos, np.float64)).max()) if len(pos) else 0.0,
               max(float(np.abs(c).max()) for c in lat.coord))
    da = C_COORD * u * cmax
    dlen0 = np.sqrt(3.0) * da
    n = np.maximum(ev["n"] - 1, 0)
    bv = (infl * dlen0 * ev["sv_len"] + (infl * C_LEN + c_pow + C_V_OPS) * u * ev["sv"] + n * u * ev["sv"])
    bg = (infl * abs(size) * da * ev["sinv"][:, None]
          + infl * dlen0 * ev["sg_len"] + (infl * C_LEN + c_pow + C_G_OPS + 1) * u * ev["sg"]
          + n[:, None] * u * ev["sg"])
    return dict(u=u, da=da, dlen0=dlen0, bv=bv, bg=bg, c_pow=c_pow, cmax=cmax)


# Normalisation of the gradient: three squares and two sums under a square root (2.5), the root (1), one
# division or a reciprocal root and a product per component (2), rounded up.
C_NORM = 6
# The project's bar for two independent float64 evaluations (tests/test_nversion_cpu.py::REL).
REL64 = 1e-12


def _ratio(err, bound):
    """err / bound per element; 0 where both are 0, inf where only the bound is."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = err / bound
    r = np.where((err == 0) & ~(bound > 0), 0.0, r)
    return np.where(np.isnan(r), np.inf, r)


def _node_ratios(pn, c, ev, b, lat):
    """Per node: the largest error / bound over v, the three scaled normals and the four colours."""
    u = b["u"]
    pn = np.asarray(pn, np.float64)
    c = np.asarray(c, np.float64)
    with np.errstate(invalid="ignore"):                     # inf - inf at a node that carries a particle
        return _node_ratios_(pn, c, ev, b, u)


def _node_ratios_(pn, c, ev, b, u):
    rv = _ratio(np.abs(pn[:, 0] - ev["v"]), b["bv"])
    g = ev["g"]
    gl = np.sqrt((g * g).sum(axis=1))
    bgn = np.sqrt((b["bg"] ** 2).sum(axis=1))
    # n_dev*|g| - g = (g_dev - g) |g|/|g_dev| + g (|g|/|g_dev| - 1) and ||g| - |g_dev|| <= |g_dev - g|:
    # a component errs by at most bg_i + |bg|, plus the normalisation's own roundings on |g|
    bn = b["bg"] + bgn[:, None] + C_NORM * u * gl[:, None]
    rn = _ratio(np.abs(pn[:, 1:4] * gl[:, None] - g), bn).max(axis=1)
    # colour mean: n - 1 additions of non-negative terms and one division
    bc = (ev["n"][:, None] + 1) * u * np.abs(ev["c"])
    rc = _ratio(np.abs(c - ev["c"]), bc).max(axis=1)
    return rv, rn, rc


def compare(pn, c, pos, colour, ptype, cells, lat, size, infl, dtype, mutate=None, exact_nodes=()):
    """Hold a lattice (pn [N,4] = v, normal; c [N,4]) to the float64 evaluation.  Returns a report dict; the caller
    asserts report['worst'] <= 1, report['pattern_bad'] == 0 and report['left_out'] <= 0.01 * report['with_hits'].

    Nodes are sorted into: early (the zero node), empty (no hit: v == 0 exactly, NaN normals, NaN colours), infinite
    (a particle on the node: v == +inf, NaN normals), band (a candidate within dlen of the threshold: must agree with
    the evaluation taking the band pairs all in or all out) and plain (everything else: inside the bound).
    exact_nodes: nodes whose only near-threshold pairs are constructed so that len is computed without rounding in
    the precision under test; they are never left out.
    """
    pn = np.asarray(pn)
    c = np.asarray(c)
    ev = evaluate(pos, colour, ptype, cells, lat, size, infl, mutate=mutate)
    b = bounds(ev, lat, pos, size, infl, dtype)
    N = lat.n_nodes
    assert pn.shape == (N, 4) and c.shape == (N, 4), (pn.shape, c.shape, N)
    dlen = b["dlen0"] + C_LEN * b["u"] * lat.threshold
    band = ev["gap"] <= dlen
    band[list(exact_nodes)] = False                         # pairs constructed so that len is exact: `<` is decided
    early = np.zeros(N, bool)
    if "early" in ev:
        early[ev["early"]] = True
    infinite = np.isinf(ev["v"]) & ~early
    empty = (ev["hits"] == 0) & ~band & ~early
    plain = (ev["hits"] > 0) & ~band & ~infinite & ~early
    bad = 0
    bad += int((pn[early] != 0).sum() + (c[early] != 0).sum())
    bad += int((pn[empty, 0] != 0).sum() + (~np.isnan(pn[empty, 1:])).sum() + (~np.isnan(c[empty])).sum())
    bad += int((pn[infinite, 0] != np.inf).sum() + (~np.isnan(pn[infinite, 1:])).sum())
    rv, rn, rc = _node_ratios(pn, c, ev, b, lat)
    rep = dict(ev=ev, bounds=b, band=band, plain=plain, empty=empty, infinite=infinite, pattern_bad=bad,
               with_hits=int((ev["hits"] > 0).sum()), left_out=int((band & (ev["hits"] > 0)).sum()),
               rv=float(rv[plain].max(initial=0)), rn=float(rn[plain].max(initial=0)),
               rc=float(np.maximum(rc[plain], 0).max(initial=0)), node_rv=rv, node_rn=rn, node_rc=rc)
    if infinite.any():                                      # colours of an infinite node are ordinary means
        rep["rc"] = max(rep["rc"], float(rc[infinite].max()))
    if dtype == np.float64 or np.dtype(dtype) == np.float64:
        # the project's bar for independent float64 evaluations: rv_bar = error / (1e-12 * sum |t|), asserted <= 1 by
        # the callers next to the derived bound
        sel = plain & (ev["sv"] > 0)
        dv = np.zeros(N)
        dv[sel] = np.abs(np.asarray(pn[:, 0], np.float64)[sel] - ev["v"][sel])
        rep["rv_bar"] = float((dv[sel] / (REL64 * ev["sv"][sel])).max(initial=0))
    rep["band_worst"] = 0.0
    rep["ok_out"] = np.ones(N, bool)
    if band.any():
        worst = []
        for side in ("in", "out"):
            e2 = evaluate(pos, colour, ptype, cells, lat, size, infl, mutate=mutate, band=(dlen, side))
            b2 = bounds(e2, lat, pos, size, infl, dtype)
            r = list(_node_ratios(pn, c, e2, b2, lat))
            nohit = e2["hits"] == 0                          # all out and nothing left: the empty pattern
            pat = (pn[:, 0] == 0) & np.isnan(pn[:, 1:]).all(axis=1) & np.isnan(c).all(axis=1)
            inf2 = np.isinf(e2["v"])
            patinf = (pn[:, 0] == np.inf) & np.isnan(pn[:, 1:]).all(axis=1)
            w = np.maximum(np.maximum(r[0], r[1]), r[2])
            w = np.where(nohit, np.where(pat, 0.0, np.inf), w)
            w = np.where(inf2, np.where(patinf, 0.0, np.inf), w)
            worst.append(w)
            if side == "out":
                rep["ok_out"] = w <= 1
        rep["band_worst"] = float(np.minimum(worst[0], worst[1])[band].max())
    rep["worst"] = max(rep["rv"], rep["rn"], rep["rc"], rep["band_worst"])
    return rep


def summary(rep):
    return (f"v {rep['rv']:.3g} n {rep['rn']:.3g} c {rep['rc']:.3g} band {rep['band_worst']:.3g} "
            f"left_out {rep['left_out']}/{rep['with_hits']} pattern_bad {rep['pattern_bad']}"
            + (f" v/1e-12 {rep['rv_bar']:.3g}" if "rv_bar" in rep else ""))
