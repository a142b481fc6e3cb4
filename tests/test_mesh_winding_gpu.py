"""The winding-number sign of the mesh collider on the device (PBF_MESH_SIGN_WINDING of pbf_sdf_from_mesh / pbf_set_collider_mesh,
pbf_mesh_winding, include/pbf_hip.h):

  6. pbf_mesh_winding equals the longdouble restatement (tests/mesh_winding_ref.py) within bar_w(N);
  7. pbf_sdf_from_mesh with the flag: |phi| is the distance fold's sqrt(best) bit for bit, the sign the reference's wherever
     the bar decides it; on closed meshes the array is the one the pseudonormal sign gives, byte for byte;
  8. "sdf_launch_pairs" splits both folds over launches without changing a byte; so does "sdf_cull";
  9. an open box whose missing face lies beyond the lattice installs the closed box's collider, eager and replayed;
 10. a bowl cut open holds the fluid as a cavity; without the flag it is refused;
 11. refusals leave the ctx, its collider and the output arrays alone;
 12. the C++ shim's setColliderMesh(winding) / meshWinding() and `benchmark --collider=mesh:FILE.obj,...,winding`.

The bar, the restatement and the soups themselves: tests/test_mesh_winding_cpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import collider_ref as CR
import mesh_sdf_ref as MR
import mesh_shapes as MS
import mesh_soups as SP
import mesh_winding_ref as WR
from test_collider_gpu import BOX_LATTICE, ERR_INVALID, ERR_STATE, IDS, VARIANTS, dt_of, plane_through, set_lattice, solver, state_bytes
from test_mesh_sdf_gpu import write_obj
from test_nversion_cpu import scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pbf-sph_amd", "benchmark")
VALUE_CASES = [(n, l) for l in ("3x5x4", "A") for n in SP.ALL] + [("open1", "2x2x2"), ("ico2", "2x2x2")]
SIGN_CASES = [(n, l) for l in ("3x5x4", "A", "ties") for n in SP.ALL] + [("open1", "2x2x2"), ("ico2", "2x2x2")]


def w_long(name, lattice):
    return WR.w_of(WR.case(name, lattice, np.longdouble)[1])


# ---- 6. the field by value ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name,lattice", VALUE_CASES)
def test_winding_field_equals_the_reference(pkg, name, lattice, fp64, fast):
    v, t = SP.mesh(name, lattice)
    lat = MS.LATTICES[lattice]
    dtype = dt_of(fp64)
    best, _ = WR.case(name, lattice, dtype)
    far = WR.far_nodes(best, lat["spacing"])
    assert far.all()                                       # (tests/test_mesh_winding_cpu.py: none is left out on these lattices)
    got = solver(pkg, fp64, fast).mesh_winding(v, t, lat["origin"], lat["spacing"], lat["dims"])
    assert got.dtype == dtype and got.shape == tuple(lat["dims"])
    e = np.abs(got.reshape(-1).astype(np.longdouble) - w_long(name, lattice))[far]
    print(f"{name} on {lattice}: worst |w - w_longdouble| = {float(e.max()):.3e}, bar {WR.bar_w(dtype):.3e}")
    assert e.max() <= WR.bar_w(dtype)


# ---- 7. the signed distance under the flag --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name,lattice", SIGN_CASES)
def test_sdf_with_the_winding_sign(pkg, name, lattice, fp64, fast):
    v, t = SP.mesh(name, lattice)
    lat = MS.LATTICES[lattice]
    dtype = dt_of(fp64)
    args = (v, t, lat["origin"], lat["spacing"], lat["dims"])
    best, _ = WR.case(name, lattice, dtype)
    wl = w_long(name, lattice)
    on = best == 0
    decided = ~on & WR.far_nodes(best, lat["spacing"]) & (np.abs(wl - np.longdouble(0.5)) > WR.bar_w(dtype))
    left_out = ~on & ~decided
    print(f"{name} on {lattice}: {int(on.sum())} nodes on the mesh, {int(left_out.sum())} of {best.size} left out of the sign check")
    assert left_out.sum() <= 0.01 * best.size
    s = solver(pkg, fp64, fast)
    for negate in (False, True):
        got, stats = s.sdf_from_mesh(*args, negate, winding=True)
        assert got.dtype == dtype and got.shape == tuple(lat["dims"])
        flat = got.reshape(-1)
        assert np.abs(flat).tobytes() == np.sqrt(best).tobytes(), (negate, int((np.abs(flat) != np.sqrt(best)).sum()))
        assert np.array_equal(np.signbit(flat[on]), np.full(int(on.sum()), negate))                     # +0, or -0 under negate
        assert np.array_equal(np.signbit(flat[decided]), (wl[decided] > 0.5) != negate), (negate, int((np.signbit(flat[decided]) != ((wl[decided] > 0.5) != negate)).sum()))
        assert 0 < stats["pairs_tested"] <= stats["pairs_total"] == got.size * len(t)
        if name in SP.CLOSED:
            plain, _ = s.sdf_from_mesh(*args, negate)
            assert got.tobytes() == plain.tobytes(), (negate, int((got != plain).sum()))


# ---- 8. the launch split and the cull -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_launch_split_and_cull_give_the_same_bytes(pkg, fp64, fast):
    lat = MS.LATTICE_A
    bricks = int(np.prod([(d + 3) // 4 for d in lat["dims"]]))
    one = solver(pkg, fp64, fast)
    split = solver(pkg, fp64, fast).set_option("sdf_launch_pairs", 64 * 16 * bricks)          # 16 triangles per launch
    nocull = solver(pkg, fp64, fast).set_option("sdf_cull", 0)
    both = solver(pkg, fp64, fast).set_option("sdf_cull", 0).set_option("sdf_launch_pairs", 64 * 16 * bricks)
    for name in ("bowl", "ico2", "cap3"):
        v, t = SP.mesh(name, "A")
        assert len(t) > 3 * 16                                                                  # several launches
        args = (v, t, lat["origin"], lat["spacing"], lat["dims"])
        total = int(np.prod(lat["dims"])) * len(t)
        w = one.mesh_winding(*args)
        assert split.mesh_winding(*args).tobytes() == w.tobytes(), name
        for negate in (False, True):
            a, sa = one.sdf_from_mesh(*args, negate, winding=True)
            b, sb = split.sdf_from_mesh(*args, negate, winding=True)
            c, sc = nocull.sdf_from_mesh(*args, negate, winding=True)
            d, sd = both.sdf_from_mesh(*args, negate, winding=True)
            assert a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes(), (name, negate)
            assert sa["pairs_total"] == sb["pairs_total"] == sc["pairs_total"] == sd["pairs_total"] == total
            assert sc["pairs_tested"] == sd["pairs_tested"] == total                            # the distance fold, every pair
            assert 0 < sa["pairs_tested"] < total and 0 < sb["pairs_tested"] < total
            if name in SP.CLOSED:                                                               # the fold without the flag splits too
                e, se = one.sdf_from_mesh(*args, negate)
                f, sf = split.sdf_from_mesh(*args, negate)
                g, sg = both.sdf_from_mesh(*args, negate)
                assert e.tobytes() == f.tobytes() == g.tobytes() and sg["pairs_tested"] == total and 0 < sf["pairs_tested"] < total


# ---- 9. the install path -----------------------------------------------------------------------------------------------------
# gravity is +y: the box stands in the cloud scene's block of fluid and reaches 400 below the lattice, which ends at y = 1050
PILLAR = ((90.0, 760.0, 110.0), (260.0, 1450.0, 270.0))       # (no face on a lattice plane)


def pillar():
    """(vertices, all 12 triangles, the 10 that stay): the two removed ones are the face y = hi, last in index order"""
    v, t = MS.box(*PILLAR)
    assert (v[t[-2:].astype(np.int64)][..., 1] == PILLAR[1][1]).all() and (v[t[:-2].astype(np.int64)][..., 1] < PILLAR[1][1]).any(axis=1).all()
    return v, t, t[:-2].copy()


def test_no_node_is_nearest_to_the_pillars_missing_face():
    """on the CPU, in both precisions: every node's distance to the two removed triangles is strictly larger than to the rest,
    so the open pillar's distance fold is the closed one's"""
    v, t, kept = pillar()
    for dtype in (np.float32, np.float64):
        rec = WR.records30(WR.soup_records(v, t)).astype(dtype)
        p = MR.nodes(BOX_LATTICE["origin"], BOX_LATTICE["spacing"], BOX_LATTICE["dims"], dtype)
        d2, _ = MR._pairs(p, rec)
        assert (d2[:, -2:].min(axis=1) > d2[:, :-2].min(axis=1)).all()


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_open_pillar_installs_the_closed_pillars_collider(pkg, fp64, fast):
    v, t, kept = pillar()
    sc = scene("cloud")
    p = pkg.default_params(4, 1000.0)
    pts = np.random.default_rng(3).random((4000, 3)) * 1000.0
    closed, _ = solver(pkg, fp64, fast).sdf_from_mesh(v, t, **BOX_LATTICE)
    opened, _ = solver(pkg, fp64, fast).sdf_from_mesh(v, kept, winding=True, **BOX_LATTICE)
    assert (closed < 0).any() and opened.tobytes() == closed.tobytes(), int((opened != closed).sum())
    a, b, free = (solver(pkg, fp64, fast).upload(**sc) for _ in range(3))
    g, h = (solver(pkg, fp64, fast).set_option("graph", 1).upload(**sc) for _ in range(2))
    for s in (a, g):
        s.set_collider_mesh(v, t, margin=CR.MARGIN, **BOX_LATTICE)
    for s in (b, h):
        stats = s.set_collider_mesh(v, kept, margin=CR.MARGIN, winding=True, **BOX_LATTICE)
        assert stats["pairs_total"] == closed.size * len(kept)
    sa, sb = a.collider_sample(p, pts), b.collider_sample(p, pts)
    assert sa["hit"].any() and not sa["hit"].all()
    assert all(sa[k].tobytes() == sb[k].tobytes() for k in sa)
    for _ in range(6):
        a.step(p), b.step(p), free.step(p)
    g.steps(p, 6), h.steps(p, 6)
    assert state_bytes(a) == state_bytes(b) and state_bytes(g) == state_bytes(h)
    assert h.graph_stats()[1] > 0
    assert state_bytes(a)["pos"] != state_bytes(free)["pos"]                 # the pillar does act on this scene


# ---- 10. it holds the fluid -----------------------------------------------------------------------------------------------
def test_cut_bowl_holds_the_cloud_as_a_cavity(pkg):
    """mesh_soups' bowl — an icosphere with two subdivisions cut open above centre_z + 0.24 R — about the cloud scene's block of
    fluid, PBF_MESH_NEGATE: the solid is outside.  The opening looks along +z, away from the fluid; the block's far corners
    start up to 130 world units inside the solid, beyond margin + spacing, and the free run leaves particles there."""
    R, centre = 330.0, np.array([165.0, 835.0, 400.0])
    v, t = MS.icosphere(2, R, centre)
    t = t[v[t.astype(np.int64)].mean(axis=1)[:, 2] < centre[2] + 0.24 * R].copy()
    assert 150 < len(t) < 320
    sc = scene("cloud")
    p = pkg.default_params(4, 1000.0)
    bar = -(CR.MARGIN + BOX_LATTICE["spacing"])
    held = solver(pkg, False).upload(**sc)
    with pytest.raises(pkg.PbfError) as e:
        held.set_collider_mesh(v, t, margin=CR.MARGIN, negate=True, **BOX_LATTICE)
    assert f"({ERR_INVALID})" in str(e.value) and "open" in str(e.value)
    held.set_collider_mesh(v, t, margin=CR.MARGIN, negate=True, winding=True, **BOX_LATTICE)
    free = solver(pkg, False).upload(**sc)
    start = held.collider_sample(p, sc["pos"])["phi"]
    assert (start < bar).any()
    held.steps(p, 20), free.steps(p, 20)
    where = [held.collider_sample(p, s.pstar()[:, :3].astype(np.float64) * CR.SCALE)["phi"] for s in (held, free)]
    counts = [int((w < bar).sum()) for w in where]
    print(f"particles with phi < -(margin + spacing) after 20 steps: {counts[0]} in the cut bowl, {counts[1]} without it; lowest phi {where[0].min():.2f}")
    assert counts[0] == 0 and counts[1] > 0, counts


# ---- 11. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_alone(pkg):
    from pbf_sph_amd import capi
    W = capi.MESH_SIGN_WINDING
    sc = scene("cloud")
    lat, phi64, _ = plane_through(sc, np.float32)
    p = pkg.default_params(4, 1000.0)
    s = solver(pkg, False).upload(**sc)
    L = s.L
    set_lattice(s, lat, phi64, BOX_LATTICE["spacing"]).steps(p, 2)
    pts = np.random.default_rng(2).random((500, 3)) * 1000.0
    before, sample, gen = state_bytes(s), s.collider_sample(p, pts), s.graph_stats()
    v, t = SP.mesh("open1")
    good, keep = capi.mesh_struct(v, t)
    out = np.full(BOX_LATTICE["dims"], 777.0, np.float32)
    OUT = out.ctypes.data_as(C.c_void_p)

    def sdf(dims=BOX_LATTICE["dims"], origin=BOX_LATTICE["origin"], spacing=BOX_LATTICE["spacing"], margin=CR.MARGIN):
        d = capi.ColliderSdf()
        d.dims[:], d.origin[:] = list(dims), list(origin)
        d.spacing, d.margin, d.phi = spacing, margin, None
        return d

    def refused(code, mesh, lattice, flags=W, both=True):
        """the three entry points (pbf_mesh_winding takes no flags: only where the flags are not the point)"""
        st = capi.MeshSdfStats(5, 6)
        m = None if mesh is None else C.byref(mesh)
        d = None if lattice is None else C.byref(lattice)
        assert L.pbf_sdf_from_mesh(s.ctx, m, d, flags, OUT, C.byref(st)) == code
        assert L.pbf_set_collider_mesh(s.ctx, m, d, flags, C.byref(st)) == code
        if both:
            assert L.pbf_mesh_winding(s.ctx, m, d, OUT) == code
        assert (st.pairs_total, st.pairs_tested) == (5, 6)

    bad = {"a dim < 2": sdf(dims=(1, 23, 23)), "2^31 nodes": sdf(dims=(2048, 1024, 1024)), "origin nan": sdf(origin=(0.0, np.nan, 0.0)),
           "spacing 0": sdf(spacing=0.0), "spacing inf": sdf(spacing=np.inf)}
    for what, d in bad.items():
        refused(ERR_INVALID, good, d)
    refused(ERR_INVALID, good, None)
    assert L.pbf_set_collider_mesh(s.ctx, C.byref(good), C.byref(sdf(margin=-0.5)), W, None) == ERR_INVALID
    # unknown bits are still unknown with the flag set; bit 1 stays unknown
    for flags in (W | 2, W | (1 << 7), W | (1 << 3), 2):
        refused(ERR_INVALID, good, sdf(), flags, both=False)
        assert b"unknown flag bits" in L.pbf_last_error(s.ctx)
    # NULL outputs
    assert L.pbf_sdf_from_mesh(s.ctx, C.byref(good), C.byref(sdf()), W, None, None) == ERR_INVALID and b"phi == NULL" in L.pbf_last_error(s.ctx)
    assert L.pbf_mesh_winding(s.ctx, C.byref(good), C.byref(sdf()), None) == ERR_INVALID and b"w == NULL" in L.pbf_last_error(s.ctx)
    # meshes the kernels could not survive
    refused(ERR_INVALID, None, sdf())
    flat = t.copy()
    flat[4, 1] = flat[4, 0]
    m, keep2 = capi.mesh_struct(v, flat)
    refused(ERR_INVALID, m, sdf())
    assert L.pbf_last_error(s.ctx) == b"pbf_mesh_soup_records: a triangle has zero area"
    bad_t = t.copy()
    bad_t[9, 2] = len(v)
    m, keep3 = capi.mesh_struct(v, bad_t)
    refused(ERR_INVALID, m, sdf())
    # without the flag the open mesh is still refused, by pbf_mesh_records
    refused(ERR_INVALID, good, sdf(), 0, both=False)
    assert L.pbf_last_error(s.ctx) == b"pbf_mesh_records: the mesh is open (an edge with one triangle)"
    # everything refused: the output array, the collider, the particles and the captured-step key are what they were
    assert (out == 777.0).all()
    again = s.collider_sample(p, pts)
    assert all(again[k].tobytes() == sample[k].tobytes() for k in sample)
    assert state_bytes(s) == before and s.graph_stats() == gen
    # the observers that succeed leave the collider alone too
    s.mesh_winding(v, t, **BOX_LATTICE), s.sdf_from_mesh(v, t, winding=True, **BOX_LATTICE)
    again = s.collider_sample(p, pts)
    assert all(again[k].tobytes() == sample[k].tobytes() for k in sample) and state_bytes(s) == before

    # slab mode: pbf_set_collider's refusals
    t2 = solver(pkg, False).upload(**sc)
    cut = capi.SlabCut(0, 12, 0, 0)
    assert L.pbf_slab_configure(t2.ctx, C.byref(cut), 0, 0) == 0
    assert L.pbf_set_collider_mesh(t2.ctx, C.byref(good), C.byref(sdf()), W, None) == ERR_STATE and b"slab" in L.pbf_last_error(t2.ctx)
    assert L.pbf_sdf_from_mesh(t2.ctx, C.byref(good), C.byref(sdf()), W, OUT, None) == ERR_STATE
    assert L.pbf_mesh_winding(t2.ctx, C.byref(good), C.byref(sdf()), OUT) == ERR_STATE and b"slab" in L.pbf_last_error(t2.ctx)
    assert (out == 777.0).all()
    s.close()
    t2.close()


# ---- 12. the shim and the CLI -----------------------------------------------------------------------------------------------
CUBE_BALL = dict(subdivisions=2, R=150.0, centre=(350.0, 100.0, 450.0))     # inside the larger of the two cubes


def test_shim(pkg, tmp_path):
    frames = 4
    v, t = MS.icosphere(**CUBE_BALL)
    t = t[:-1]                                                               # open
    with open(tmp_path / "mesh.bin", "wb") as f:
        f.write(np.array(BOX_LATTICE["dims"], np.uint32).tobytes() + np.array(BOX_LATTICE["origin"], np.float64).tobytes() +
                np.array([BOX_LATTICE["spacing"], CR.MARGIN], np.float64).tobytes() + np.array([0, len(v), len(t)], np.uint32).tobytes() +
                v.tobytes() + np.ascontiguousarray(t).tobytes())
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_collider_soup_shim"), str(tmp_path / "mesh.bin"), str(tmp_path / "dump.bin"),
                        str(frames)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    raw = open(tmp_path / "dump.bin", "rb").read()
    n = int(np.frombuffer(raw, np.uint64, 1)[0])
    at = 8

    def take(dtype, shape):
        nonlocal at
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at).reshape(shape)
        at += a.nbytes
        return a

    def particles():
        return dict(id=take(np.uint64, (n,)), type=take(np.uint8, (n,)), mass=take(np.float32, (n,)), pos=take(np.float32, (n, 3)),
                    vel=take(np.float32, (n, 3)), colour=take(np.float32, (n, 4)))

    first, last = particles(), particles()
    nodes = int(take(np.uint64, (1,))[0])
    w = take(np.float32, (nodes,))
    assert at == len(raw)
    # the same calls over the C ABI: advance() is upload -> step -> download
    s = solver(pkg, False)
    s.set_collider_mesh(v, t, margin=CR.MARGIN, winding=True, **BOX_LATTICE)
    assert s.mesh_winding(v, t, **BOX_LATTICE).tobytes() == w.tobytes()
    p = pkg.default_params(4, 1000.0)
    st = first
    for _ in range(frames):
        st = s.upload(**st).step(p).download()
    for k in last:
        assert st[k].tobytes() == last[k].tobytes(), k


def test_cli_winding(pkg, tmp_path):
    v, t = MS.icosphere(**CUBE_BALL)
    hole = tmp_path / "hole.obj"
    write_obj(hole, v, t[:-1])
    common = ["--scene", "cubes", "--particles", "8000", "-n", "5", "-w", "0", "--resident", "--no-surface"]
    r = subprocess.run([BIN, *common, f"--collider=mesh:{hole},13.5,50,0,winding", "-o", str(tmp_path / "w")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.split("\n") if l.startswith("Collider")]
    m = re.search(r"mesh .*hole\.obj \(winding sign\), (\d+) triangles, volume ([-+.e\d]+), lattice 23 x 23 x 23, spacing 50, margin 13\.5, "
                  r"pairs tested (\d+) / (\d+), boundary 3, non-manifold 0, misoriented 0$", line[0])
    assert m, line
    assert int(m.group(1)) == len(t) - 1 and int(m.group(4)) == 23 ** 3 * (len(t) - 1) and 0 < int(m.group(3)) <= int(m.group(4))
    # still refused without the field, and the four-field form is what it was
    r = subprocess.run([BIN, *common, f"--collider=mesh:{hole},13.5,50,0", "-o", str(tmp_path / "h")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "open" in r.stdout + r.stderr and "boundary 3" in r.stdout + r.stderr
    ball = tmp_path / "ball.obj"
    write_obj(ball, v, t)
    r = subprocess.run([BIN, *common, f"--collider=mesh:{ball},13.5,50,0", "-o", str(tmp_path / "b")], capture_output=True, text=True, timeout=300)
    line = [l for l in r.stdout.split("\n") if l.startswith("Collider")]
    assert r.returncode == 0 and re.search(r"ball\.obj, \d+ triangles, volume [-+.e\d]+, lattice 23 x 23 x 23, spacing 50, margin 13\.5, pairs tested \d+ / \d+$", line[0]), line
    help_ = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "[,negate[,winding]]" in help_
