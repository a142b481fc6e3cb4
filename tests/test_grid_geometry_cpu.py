"""The geometries of tests/grid_scenes.py really exercise what they are for (no GPU: the oracle's state after predict,
sort and table).  Without these checks the bit-exact GPU tests on them (tests/test_grid_geometry_gpu.py) could pass
vacuously: a scene whose neighbour pairs never straddle a quantisation wrap, whose rows never cross a 64-cell segment,
or whose x-column-0 walkers never see column 1023 would not test the mechanism it is named after.
"""
import numpy as np
import pytest

import grid_scenes as G
import nversion as NV
import oracle_lib as O


def after_table(name, fp64=False):
    sc, _, q, h = G.make_geometry(name, fp64)
    o = O.Oracle(fp64, device_pow=True)
    o.set_particles(**sc)
    o.predict(q).sort(q).grid_table(q)
    return o, q, h


def decode(keys):
    k = np.asarray(keys, np.int64)

    def c10(v):
        v = v & 0x09249249
        v = (v | (v >> 2)) & 0x030C30C3
        v = (v | (v >> 4)) & 0x0300F00F
        v = (v | (v >> 8)) & 0x030000FF
        return (v | (v >> 16)) & 0x3FF
    return np.stack([c10(k), c10(k >> 1), c10(k >> 2)], 1)


def encode(xyz):
    def s10(v):
        v = np.asarray(v, np.int64) & 0x3FF
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        return (v | (v << 2)) & 0x09249249
    return s10(xyz[..., 0]) | s10(xyz[..., 1]) << 1 | s10(xyz[..., 2]) << 2


@pytest.mark.parametrize("name", G.NAMES)
def test_extent_table_and_row_shift(oracle, name):
    g = G.bounds(name)
    o, _, _ = after_table(name)
    e, m = o.extent()
    assert tuple(int(v) for v in e) == g["ext"]
    lo, _ = G.grid_frame(g, np.float32)
    assert np.array_equal(m, lo)
    tn = G.table_len(g["ext"])
    assert len(o.table()) == tn if tn < 10 ** 8 else o.L.pbf_oracle_table_size(o.h) == tn
    assert G.row_shift(tn) == g["pshift"]
    keys = o.keys().astype(np.int64)
    assert keys.max() < tn                           # every particle is in a cell: each one walks
    assert (np.diff(keys) >= 0).all()
    if name == "edge_x":
        assert tn > 2 ** 27 and g["pshift"] == 10    # the cube P = 1024: x + 1 at x = 1023 wraps to a code < tableN


def pairs_within(ps, h, chunk=1024):
    """(a, b) with a < b and |ps[a] - ps[b]| <= h, float64."""
    out = []
    for s in range(0, len(ps), chunk):
        d = ps[s:s + chunk, None, :] - ps[None, :, :]
        a, b = np.nonzero((d * d).sum(-1) <= h * h)
        keep = a + s < b
        out.append(np.stack([a[keep] + s, b[keep]], 1))
    return np.concatenate(out)


@pytest.mark.parametrize("name", ["long_x", "tall_y", "deep_z", "offset"])
def test_pairs_straddle_the_qpos_wrap_and_rows_cross_segments(oracle, name):
    """qpos keeps the low 16 bits of floor((p - gridMin) 2048 / h) (pbf_kernels.hpp quantise_position): it wraps every
    32 cells.  At least 100 neighbour pairs within h lie on opposite sides of a wrap.  k_diffuse_rows gives one wave to
    each 64-cell x-segment: where the grid is at least 64 cells wide in x (long_x, offset), at least 100 walkers have a
    three-cell row run that crosses a segment edge (tall_y / deep_z are 10-12 cells wide in x: rows of one segment)."""
    g = G.bounds(name)
    o, q, h = after_table(name)
    N = np.float32
    ps = o.pstar()
    lo, _ = G.grid_frame(g, N)
    k = N(N(2048) / N(h))
    f = np.floor(((ps - lo).astype(N) * k).astype(N)).astype(np.int64)
    assert f.min() >= 0 and f.max() < 2 ** 22
    pr = pairs_within(ps.astype(np.float64), float(N(h)))
    wrapped = ((f[pr[:, 0]] >> 16) != (f[pr[:, 1]] >> 16)).any(1)
    assert wrapped.sum() >= 100, (name, int(wrapped.sum()), len(pr))
    # (and the wrapped differences are the small ones the list build's threshold accepts)
    dq = (f[pr[:, 0]] - f[pr[:, 1]]) & 0xFFFF
    dq = np.where(dq >= 0x8000, dq - 0x10000, dq)
    assert np.abs(dq).max() <= 2048 + 5
    if g["ext"][0] >= 64:
        x = decode(o.keys())[:, 0]
        crossing = (x % 64 == 63) | ((x % 64 == 0) & (x > 0))
        assert crossing.sum() >= 100, (name, int(crossing.sum()))


def test_edge_x_walk_wraps_between_columns_0_and_1023(oracle):
    """P = 1024: the reference's x - 1 at x = 0 is 1023 (spread10 keeps 10 bits) and that code is inside the table, so
    the colour of a column-0 walker includes the particles of column 1023 in the same (y +- 1, z +- 1) cells, and the
    reverse.  The diffusion walk has no distance test (ompsph.hpp:188-207).  Recomputed in float64 with the wrap and
    with the walk clamped at the faces, the two colours differ by far more than an fp32 ulp, so a device that clamps
    cannot match the oracle bit for bit.  (The step weight is dt / 750 = 1.7e-5: a whole-colour difference moves the
    result by about 2e-5, some 300 ulps of fp32 at 1.)"""
    o, q, h = after_table("edge_x")
    g = G.bounds("edge_x")
    tn = G.table_len(g["ext"])
    keys = o.keys().astype(np.int64)
    st = o.get_particles()
    col = st["colour"].astype(np.float64)
    candidate = (st["type"] & 1) == 0
    xyz = decode(keys)

    def run(code):  # foreach_grid's range of one cell (the table is the exclusive scan of the sorted keys)
        if code >= tn:
            return np.zeros(0, np.int64)
        a, b = np.searchsorted(keys, [code, code + 1], "left")
        return np.arange(a, b)

    def walk(home, clamp):
        out = []
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    c = home + np.array([dx, dy, dz])
                    if clamp and (c < 0).any() | (c > 1023).any():
                        continue
                    out.append(run(int(encode(c & 0x3FF))))
        return np.concatenate(out)

    t = float(np.float32(np.float32(q.dt) / np.float32(750.0)))

    def diffuse(a, members):
        m = members[candidate[members]]
        y = col[m].sum(0) / len(m) * 1.33
        return np.clip(col[a] * (1 - t) + y * t, 0.03, 1.0)

    o.diffuse(q)
    got = o.get_particles()["colour"].astype(np.float64)
    for side, far in ((0, 1023), (1023, 0)):
        walkers = np.flatnonzero((xyz[:, 0] == side) & (st["type"] == 0))
        assert len(walkers) >= 10
        seen = 0
        for a in walkers:
            wrap, clamp = walk(xyz[a], False), walk(xyz[a], True)
            across = wrap[xyz[wrap, 0] == far]
            if len(across) == 0:
                continue
            seen += 1
            assert np.allclose(col[across], G.EDGE_HI_COLOUR if far == 1023 else G.EDGE_LO_COLOUR, atol=1e-6)
            cw, cc = diffuse(a, wrap), diffuse(a, clamp)
            assert np.abs(cw - cc).max() > 1e-6, (side, a)
            assert np.abs(got[a] - cw).max() <= 1e-6 < np.abs(got[a] - cc).max(), (side, a)  # the oracle wraps
        assert seen >= 10, (side, seen)


@pytest.mark.parametrize("name", ["long_x", "offset"])
def test_oracle_equals_all_pairs_on_long_grids(name):
    """The independent check that does not go through the oracle's grid: on the first two bundles of lines (the whole
    length of the long axis, so pairs straddle the table's long-axis Morton bits), the fp64 oracle's lambda, delta-p
    and finalise equal tests/nversion.py's all-pairs float64 evaluation to 1e-12 (as tests/test_nversion_cpu.py on the
    small scenes)."""
    REL = 1e-12
    sc, _, q, h = G.make_geometry(name, True)
    per_bundle = len(sc["id"]) // len(G.GEOMETRIES[name]["bundles"])
    keep = sc["id"] < 2 * per_bundle
    sc = {k: v[keep] for k, v in sc.items()}
    q.iteration = 1
    o = O.Oracle(True, device_pow=False)
    o.set_particles(**sc)
    o.predict(q).sort(q).grid_table(q)
    st = o.get_particles()
    ps = o.pstar().astype(np.float64)
    obstacle = st["type"] == 1
    assert o.keys().max() < len(o.table())
    cells = NV.predict_cells(ps, h, q.scale, list(q.min_bound))
    for it in range(2):
        o.lambda_(q)
        cm = None if it == 0 else cells
        lam, _ = NV.lambdas(ps, st["mass"].astype(np.float64), h, obstacle, cm)
        assert np.abs(o.lambdas() - lam).max() <= REL * np.abs(lam).max(), (name, it, "lambda")
        o.delta(q)
        ps_new, _ = NV.delta(ps, lam, h, q.scale, list(q.min_bound), list(q.max_bound), obstacle, cm)
        move_o, move_n = o.pstar() - ps, ps_new - ps
        # (+ one ulp of the largest pStar: the oracle's move is read back as a difference of two rounded positions,
        # which lie up to 15 sim units from the origin here)
        assert np.abs(move_o - move_n).max() <= REL * max(np.abs(move_n).max(), 1e-30) + np.spacing(np.abs(ps).max()), \
            (name, it, "delta-p")
        ps = o.pstar().astype(np.float64)
    pos_before, vel_before = st["pos"].astype(np.float64), st["vel"].astype(np.float64)
    o.finalise(q)
    pos, vel = NV.finalise(ps, pos_before, vel_before, q.dt, q.scale)
    g = o.get_particles()
    fl = ~obstacle
    assert np.abs(g["pos"][fl] - pos[fl]).max() <= REL * np.abs(pos).max()
    assert np.abs(g["vel"][fl] - vel[fl]).max() <= 1e-11 * max(np.abs(vel).max(), 1e-30)
    assert np.array_equal(g["pos"][obstacle], pos_before[obstacle])
