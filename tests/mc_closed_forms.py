"""Closed forms and invariants of the marching-cubes surface that share no reading with any restatement
(test infrastructure).  Each check takes an `engine`: run(scene dict, fp64) -> (state, surface(mc tuple) -> dict, predict-time cells),
bound to the oracle on the CPU (tests/test_mc_nversion_cpu.py) and to the device on the GPU
(tests/test_mc_field_gpu.py).
"""
import os

import numpy as np

import nversion_mc as NM
from test_mc import mesh_is_closed_and_oriented

HERE = os.path.dirname(os.path.abspath(__file__))

# one particle: h * scale = 100, resolution 3 => step 33.3; size 25, influence 0.5, isolevel 3.125 => R = 64 = 1.92 steps
ONE = dict(h=0.1, scale=1000.0, min_bound=(0.0,) * 3, max_bound=(1050.0,) * 3, iteration=0, force=(0.0,) * 3, frames=1)
ONE_MC = (3.0, 3.125, 25.0, 0.5)
ONE_POS = (503.7, 489.1, 521.3)
R_ISO = (ONE_MC[2] / ONE_MC[1]) ** (1.0 / ONE_MC[3])


def reference_winding():
    """+1 / -1: the sign the reference's TriTable gives (tests/golden/ref_mc_winding.npz, make_golden.py)."""
    return int(np.load(os.path.join(HERE, "golden", "ref_mc_winding.npz"))["sign"])


def _particle(pos, colour=(0.5, 0.25, 0.125, 1.0)):
    return dict(id=np.zeros(1, np.uint64), type=np.zeros(1, np.uint8), mass=np.ones(1), pos=np.array([pos], np.float64),
                vel=np.zeros((1, 3)), colour=np.array([colour], np.float64))


def _nodes(s, res, dtype):
    """Node coordinates [sx, sy, sz, 3] in float64 from ompsph.hpp:288-291 (index3d order when flattened)."""
    lat = NM.Lattice(s["h"], s["scale"], s["min_bound"], s["max_bound"], res, dtype)
    a = np.stack(np.meshgrid(*lat.coord, indexing="ij"), -1)
    return lat, a


def _dlen(lat, p, u):
    cmax = max(np.abs(p).max(), max(np.abs(c).max() for c in lat.coord))
    return np.sqrt(3.0) * NM.C_COORD * u * cmax, cmax


def check_one_particle(engine, fp64):
    dtype = np.float64 if fp64 else np.float32
    u = NM.unit_roundoff(dtype)
    s = dict(ONE, sc=_particle(ONE_POS))
    st, surface, cells = engine(s, fp64)
    p = st["pos"][0].astype(np.float64)
    res, iso, size, infl = ONE_MC
    m = surface(ONE_MC)
    lat, a = _nodes(s, res, dtype)
    assert list(m["sample"]) == list(lat.sample)
    thr = lat.threshold
    assert 1.5 * lat.step * lat.scale <= R_ISO < thr
    d = a - p
    r = np.sqrt((d * d).sum(-1)).reshape(-1)
    d = d.reshape(-1, 3)
    dl0, cmax = _dlen(lat, p, u)
    dl = dl0 + NM.C_LEN * u * r
    inside, outside = r < thr - dl, r > thr + dl
    v = m["pn"][:, 0].astype(np.float64)
    nrm = m["pn"][:, 1:].astype(np.float64)
    if all(lat.node_cell[k][-1] == lat.extent[k] for k in range(3)):
        # the last node's cell is the extent on every axis: it keeps its zeros (ompsph.hpp:301-304)
        assert (m["pn"][-1] == 0).all() and (m["c"][-1] == 0).all()
        outside[-1] = False
    # v = size / r^infl within the term's bound (one square root, one division), exactly 0 beyond the threshold
    f = size / r ** infl
    assert inside.sum() > 100
    assert (np.abs(v - f)[inside] <= (f * (infl * dl / r + (infl * NM.C_LEN + NM.C_POW_SQRT + NM.C_V_OPS) * u))[inside]).all()
    assert (v[outside] == 0).all() and np.isnan(nrm[outside]).all()
    # the normal of a node with a hit is (a - p) / |a - p|: away from the particle.  Each component of a - p carries
    # the coordinate's absolute error, the normalisation its own roundings
    want = d / r[:, None]
    tol = (2 * dl0 / r + (NM.C_NORM + NM.C_G_OPS) * u)[:, None]
    assert (np.abs(nrm - want)[inside] <= np.broadcast_to(tol, want.shape)[inside]).all()
    assert ((nrm * d).sum(-1)[inside] > 0).all()
    # the mesh: every vertex within the linear interpolation's error of the sphere |x - p| = R.  The error is taken
    # from the closed-form field along every lattice edge that crosses R (float64, nothing from the output)
    shape = tuple(int(x) for x in lat.sample)
    F = np.where(r < thr, f, 0.0).reshape(shape)
    A = a
    err, slope = [0.0], []
    for ax in range(3):
        sl0 = [slice(None)] * 3
        sl1 = [slice(None)] * 3
        sl0[ax], sl1[ax] = slice(0, -1), slice(1, None)
        f0, f1 = F[tuple(sl0)], F[tuple(sl1)]
        cross = (f0 < iso) != (f1 < iso)
        t = (iso - f0[cross]) / (f1[cross] - f0[cross])
        x = A[tuple(sl0)][cross] + t[:, None] * (A[tuple(sl1)][cross] - A[tuple(sl0)][cross])
        err.append(np.abs(np.sqrt(((x - p) ** 2).sum(-1)) - R_ISO).max())
        slope.append(np.abs(f1[cross] - f0[cross]).min())
    e_interp = max(err)
    step_w = lat.step * lat.scale
    # roundings of the interpolation itself: t from three field values (each within its term bound), the mix, the
    # coordinates (16 roundings, counted generously) -- against the smallest field difference across a crossed edge
    slack = 16 * u * (cmax + step_w * F.max() / min(slope)) + step_w * (infl * dl0 / R_ISO) * iso / min(slope)
    vs = m["vs"].astype(np.float64)
    assert len(vs) >= 3 * 20
    rad = np.sqrt(((vs - p) ** 2).sum(-1))
    assert np.abs(rad - R_ISO).max() <= e_interp + slack, (np.abs(rad - R_ISO).max(), e_interp, slack)
    bad, total = mesh_is_closed_and_oriented(m["vs"], step_w * 1e-4)
    assert bad == 0 and total > 0, (bad, total)
    # enclosed volume (divergence theorem).  A chord of a triangle no wider than a cell's diagonal lies at most one
    # sagitta inside the sphere, a vertex at most e_interp off it
    tri = vs.reshape(-1, 3, 3) - p
    vol = (tri[:, 0] * np.cross(tri[:, 1], tri[:, 2])).sum() / 6.0
    half = np.sqrt(3.0) * step_w / 2
    sag = R_ISO + e_interp - np.sqrt((R_ISO - e_interp) ** 2 - half ** 2)
    exact = 4.0 / 3.0 * np.pi * R_ISO ** 3
    sign = reference_winding()
    assert abs(sign * vol - exact) <= 4 * np.pi * (R_ISO + e_interp) ** 2 * (e_interp + sag + slack), (vol, exact, e_interp, sag)
    assert np.sign(vol) == sign, "the mesh winds against the reference's TriTable"
    wrong, n = check_winding(m, min_tris=20)
    assert wrong == 0, ("a triangle winds against its normals", wrong, n)
    return dict(e_interp=e_interp, worst=np.abs(rad - R_ISO).max(), vol=vol / exact)


def check_corner_particle(engine, fp64, faces_scene):
    """The same particle in the corner cell (0, 0, 0) of the `faces` frame, iteration 0: the clamp folds name its cell
    2 x 2 x 2 times at the nodes of the corner cell, 4 and 2 times along the edge and the face."""
    dtype = np.float64 if fp64 else np.float32
    u = NM.unit_roundoff(dtype)
    s = dict(faces_scene)
    lo = np.asarray(s["min_bound"]) / s["scale"] - 2 * s["h"]
    s["sc"] = _particle((lo + np.array([0.55, 0.45, 0.6]) * s["h"]) * s["scale"])
    st, surface, cells = engine(s, fp64)
    p = st["pos"][0].astype(np.float64)
    seen = set()
    for mc in ((2.0, 10.0, 25.0, 0.5), (3.0, 10.0, 25.0, 1.0)):
        res, _, size, infl = mc
        m = surface(mc)
        lat, a = _nodes(s, res, dtype)
        d = (a - p).reshape(-1, 3)
        r = np.sqrt((d * d).sum(-1))
        dl0, _ = _dlen(lat, p, u)
        dl = dl0 + NM.C_LEN * u * r
        # per axis: the particle's cell 0 is named twice by a node of cell 0 ({0, 0, 1}), once by a node of cell 1
        # ({0, 1, 2}), never from cell 2 on
        wa = [np.where(lat.node_cell[k] == 0, 2, np.where(lat.node_cell[k] == 1, 1, 0)) for k in range(3)]
        w = (wa[0][:, None, None] * wa[1][None, :, None] * wa[2][None, None, :]).reshape(-1).astype(np.float64)
        sel = (r < lat.threshold - dl) & (w > 0)
        f = w * size / r ** infl
        c_pow = NM.C_POW_SQRT if infl == 0.5 else NM.C_POW
        # w equal terms summed: w - 1 additions (exact doublings in binary, counted all the same)
        bound = f * (infl * dl / r + (infl * NM.C_LEN + c_pow + NM.C_V_OPS + w) * u)
        v = m["pn"][:, 0].astype(np.float64)
        assert (np.abs(v - f)[sel] <= bound[sel]).all(), (mc, np.abs(v - f)[sel].max())
        assert (v[(r > lat.threshold + dl) | (w == 0)] == 0).all()
        seen |= set(np.unique(w[sel]).astype(int))
        cc = m["c"].astype(np.float64)[sel]
        assert (np.abs(cc - st["colour"][0].astype(np.float64)) <= (w[sel][:, None] + 1) * u).all()
    assert {1, 2, 4, 8} <= seen, seen


def check_volume_sign(m):
    """A mesh that encloses the fluid: the signed volume (divergence theorem) has the sign of the reference's winding."""
    vs = m["vs"].astype(np.float64).reshape(-1, 3, 3)
    vs = vs - vs.reshape(-1, 3).mean(axis=0)
    vol = (vs[:, 0] * np.cross(vs[:, 1], vs[:, 2])).sum() / 6.0
    return int(np.sign(vol)) == reference_winding(), vol


def check_winding(m, min_tris=1000):
    """Every non-degenerate triangle winds the way the reference's TriTable does against the interpolated normals.

    Held on the one-particle sphere only, where it is a theorem: there the accumulated normal is radial, parallel to
    the field's gradient.  With several particles it is not one: the reference accumulates l / len^infl, the field's
    gradient is the sum of l / len^(infl + 2), the two weight near and far particles differently, and on the settled
    blob at the stock isolevel 962 of the oracle's 4680 triangles (cavities inside the fluid) have a normal sum on
    the other side of their plane although the mesh is closed and consistently oriented.  That is the reference's
    field, not a table defect; the blob is held to the sign of its enclosed volume instead (check_volume_sign)."""
    vs = m["vs"].astype(np.float64).reshape(-1, 3, 3)
    ns = m["ns"].astype(np.float64).reshape(-1, 3, 3)
    cr = np.cross(vs[:, 1] - vs[:, 0], vs[:, 2] - vs[:, 0])
    area = np.sqrt((cr * cr).sum(-1))
    edge = np.sqrt(((vs[:, 1] - vs[:, 0]) ** 2).sum(-1)).max()
    ok = (area > 1e-6 * edge * edge) & np.isfinite(ns).all(axis=(1, 2))
    s = np.sign((cr * ns.sum(axis=1)).sum(-1))[ok]
    assert ok.sum() >= min_tris
    return int((s != reference_winding()).sum()), int(ok.sum())


def check_one_colour(engine, fp64, scene):
    """All particles of one colour (binary fractions: every mean and the diffusion are exact, so the particles still
    share one colour after the step): every lattice colour with hits is that colour within (m + 1) u, every mesh
    colour within two more roundings."""
    dtype = np.float64 if fp64 else np.float32
    u = NM.unit_roundoff(dtype)
    s = dict(scene)
    s["sc"] = dict(scene["sc"])
    n = len(s["sc"]["id"])
    s["sc"]["colour"] = np.tile(np.array([0.5, 0.25, 0.125, 1.0]), (n, 1))
    st, surface, cells = engine(s, fp64)
    col = st["colour"].astype(np.float64)
    c0 = col[0]
    assert (col == c0).all(), "the scene must keep one colour through the step"
    mc = (2.0, 60.0, 25.0, 0.5)
    m = surface(mc)
    cc = m["c"].astype(np.float64)
    hit = ~np.isnan(cc).any(axis=1) & (m["pn"][:, 0] > 0)   # not the one zero node (ompsph.hpp:301-304)
    assert hit.sum() > 1000
    # m, the number of values summed at a node (a particle of weight w is summed w times), from the evaluation
    lat, _ = _nodes(s, mc[0], dtype)
    ev = NM.evaluate(st["pos"], st["colour"], st["type"], cells, lat, mc[2], mc[3])
    hit &= ev["n"] > 0
    mm = ev["n"][hit][:, None]
    assert (np.abs(cc[hit] - c0) <= (mm + 1) * u * c0).all()
    # a crossed edge whose outer node has no hit mixes the colour with that node's 0 / 0, as in the reference
    mesh = m["cs"].astype(np.float64)
    keep = np.isfinite(mesh).all(axis=1)
    if all(lat.node_cell[k][-1] == lat.extent[k] for k in range(3)):
        # nor the cube at the one zero node (ompsph.hpp:301-304): its edges mix with colour 0
        last = np.array([c[-1] for c in lat.coord])
        keep &= ~(np.abs(m["vs"].astype(np.float64) - last) <= lat.step * lat.scale * (1 + 1e-6)).all(axis=1)
    mesh = mesh[keep]
    assert len(mesh) > 300 and (np.abs(mesh - c0) <= (mm.max() + 3) * u * c0).all(), \
        (len(mesh), (np.abs(mesh - c0) / (u * c0)).max(), mm.max())
    return float((np.abs(cc[hit] - c0) / (u * c0)).max())
