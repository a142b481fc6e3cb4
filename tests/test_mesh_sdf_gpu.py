"""Mesh colliders on the device (pbf_sdf_from_mesh / pbf_set_collider_mesh, include/pbf_hip.h):

  7. the device's lattice equals tests/mesh_sdf_ref.py bit for bit, fed the records pbf_mesh_records returned;
  8. "sdf_cull" 0 and 1 give the same bytes; the pair counts;
  9. pbf_set_collider_mesh ends in pbf_set_collider's install path: the same samples and steps, eager and replayed;
 10. it holds the fluid: the bowl of tests/test_collider_gpu.py built from an icosphere with PBF_MESH_NEGATE;
 11. refusals leave the ctx, its collider and the output array alone;
 12. the C++ shim's setColliderMesh() and `benchmark --collider=mesh:FILE.obj`.

The restatement itself, the record builder and the host program: tests/test_mesh_sdf_cpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import collider_ref as CR
import mesh_sdf_ref as MR
import mesh_shapes as MS
from test_collider_gpu import BOX_LATTICE, ERR_INVALID, ERR_STATE, IDS, VARIANTS, dt_of, plane_through, set_lattice, solver, state_bytes
from test_nversion_cpu import scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pbf-sph_amd", "benchmark")
MESHES = ["box", "tetra", "torus", "ico2", "ico3"]
_ref = {}


def mesh_of(name, lattice):
    return MS.box(*MS.TIE_BOX) if (name == "box" and lattice == "ties") else MS.shape(name)


def reference(pkg, name, lattice, fp64):
    """(best, neg) of the restatement on the library's records, computed once per (mesh, lattice, precision)"""
    key = (name, lattice, fp64)
    if key not in _ref:
        v, t = mesh_of(name, lattice)
        rec, _ = pkg.mesh_records(v, t, fp64)
        lat = MS.LATTICES[lattice]
        best, neg = MR.field(rec, lat["origin"], lat["spacing"], lat["dims"], dt_of(fp64))
        best.setflags(write=False), neg.setflags(write=False)
        _ref[key] = (best, neg)
    return _ref[key]


# ---- 7. device == restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("lattice", list(MS.LATTICES))
@pytest.mark.parametrize("name", MESHES)
def test_device_equals_the_restatement(pkg, name, lattice, fp64, fast):
    """on the tie lattice the box is the one whose faces pass through nodes (tests/test_mesh_sdf_cpu.py, ties)"""
    v, t = mesh_of(name, lattice)
    lat = MS.LATTICES[lattice]
    best, neg = reference(pkg, name, lattice, fp64)
    s = solver(pkg, fp64, fast)
    for negate in (False, True):
        want = MR.phi(best, neg, lat["dims"], negate)
        got, stats = s.sdf_from_mesh(v, t, lat["origin"], lat["spacing"], lat["dims"], negate)
        assert got.dtype == want.dtype and got.shape == tuple(lat["dims"])
        assert got.tobytes() == want.tobytes(), (negate, int((got != want).sum()), float(np.abs(got - want).max()))
        assert 0 < stats["pairs_tested"] <= stats["pairs_total"] == got.size * len(t)      # ("sdf_cull" defaults to 1)
    if lattice == "ties" and name == "box":
        assert int((got == 0).sum()) == 386 and np.signbit(got[got == 0]).all()     # -0 under PBF_MESH_NEGATE


# ---- 8. the cull -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("lattice", list(MS.LATTICES))
def test_cull_gives_the_same_bytes(pkg, lattice, fp64, fast):
    lat = MS.LATTICES[lattice]
    off, on = solver(pkg, fp64, fast).set_option("sdf_cull", 0), solver(pkg, fp64, fast).set_option("sdf_cull", 1)
    default = solver(pkg, fp64, fast)
    for name in MESHES:
        v, t = mesh_of(name, lattice)
        for negate in (False, True):
            a, sa = off.sdf_from_mesh(v, t, lat["origin"], lat["spacing"], lat["dims"], negate)
            b, sb = on.sdf_from_mesh(v, t, lat["origin"], lat["spacing"], lat["dims"], negate)
            assert a.tobytes() == b.tobytes(), (name, negate, int((a != b).sum()))
            assert sa["pairs_tested"] == sa["pairs_total"] == sb["pairs_total"] == a.size * len(t)
            assert 0 < sb["pairs_tested"] <= sb["pairs_total"]
        print(f"{name} on {lattice}: the cull tested {sb['pairs_tested']} of {sb['pairs_total']} pairs ({sb['pairs_tested'] / sb['pairs_total']:.3f})")
        if name == "ico2" and lattice == "A":
            assert sb["pairs_tested"] < sb["pairs_total"]
            assert default.sdf_from_mesh(v, t, lat["origin"], lat["spacing"], lat["dims"], True)[1] == sb     # the default is 1


# ---- 9. the install path ---------------------------------------------------------------------------------------------------
BALL = dict(subdivisions=2, R=120.0, centre=(165.0, 835.0, 165.0))       # inside the cloud scene's block of fluid


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_set_collider_mesh_is_set_collider_of_the_lattice(pkg, fp64, fast):
    v, t = MS.icosphere(**BALL)
    sc = scene("cloud")
    p = pkg.default_params(4, 1000.0)
    pts = np.random.default_rng(3).random((4000, 3)) * 1000.0
    a, b, free = (solver(pkg, fp64, fast).upload(**sc) for _ in range(3))
    phi, _ = a.sdf_from_mesh(v, t, **BOX_LATTICE)
    assert (phi < 0).any()
    a.set_collider(phi, BOX_LATTICE["origin"], BOX_LATTICE["spacing"], CR.MARGIN)
    stats = b.set_collider_mesh(v, t, margin=CR.MARGIN, **BOX_LATTICE)
    assert stats["pairs_total"] == phi.size * len(t)
    sa, sb = a.collider_sample(p, pts), b.collider_sample(p, pts)
    assert sa["hit"].any() and not sa["hit"].all()
    assert all(sa[k].tobytes() == sb[k].tobytes() for k in sa)
    for _ in range(6):
        a.step(p), b.step(p), free.step(p)
    assert state_bytes(a) == state_bytes(b)
    assert state_bytes(a)["pos"] != state_bytes(free)["pos"]                 # the ball does act on this scene


def test_graph_replay_after_the_mesh_replaced_a_plane(pkg):
    v, t = MS.icosphere(**BALL)
    sc = scene("cloud")
    lat1, phi1, _ = plane_through(sc, np.float32, 0.5)
    p = pkg.default_params(4, 1000.0)
    g = solver(pkg, False).set_option("graph", 1).upload(**sc)
    e = solver(pkg, False).upload(**sc)
    for s in (g, e):
        set_lattice(s, lat1, phi1, BOX_LATTICE["spacing"])
    g.steps(p, 6)
    for _ in range(6):
        e.step(p)
    assert state_bytes(g) == state_bytes(e) and g.graph_stats()[1] > 0
    g.set_collider_mesh(v, t, margin=CR.MARGIN, **BOX_LATTICE)
    phi, _ = e.sdf_from_mesh(v, t, **BOX_LATTICE)
    e.set_collider(phi, BOX_LATTICE["origin"], BOX_LATTICE["spacing"], CR.MARGIN)
    before = g.graph_stats()[1]
    g.steps(p, 6)
    for _ in range(6):
        e.step(p)
    assert state_bytes(g) == state_bytes(e)
    assert g.graph_stats()[1] > before and g.graph_stats()[2] and e.graph_stats()[1] == 0
    # a stale plane would have shown: the plane alone gives another run
    x = solver(pkg, False).upload(**sc)
    set_lattice(x, lat1, phi1, BOX_LATTICE["spacing"])
    for _ in range(12):
        x.step(p)
    assert state_bytes(x)["pos"] != state_bytes(e)["pos"]


# ---- 10. it holds the fluid ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_block_falls_into_the_mesh_bowl(pkg, fp64):
    """test_collider_gpu.test_block_falls_into_the_bowl with the bowl built from an icosphere whose vertices lie on that
    sphere, PBF_MESH_NEGATE: the mesh lies inside the sphere, so the same assertion holds.  The sphere, lattice and step count
    are locals of that test (restated here); the scene, margin and scale are its imports."""
    r, spacing, centre = 400.0, 25.0, np.array([500.0, 500.0, 500.0])
    origin, dims = (-spacing,) * 3, (43, 43, 43)
    v, t = MS.icosphere(3, r, centre)
    assert np.abs(np.linalg.norm(v - centre, axis=1) - r).max() < 1e-9
    sc = CR.block_scene()
    p = pkg.default_params(4, 1000.0)
    counts = []
    for on in (True, False):
        s = solver(pkg, fp64).upload(**sc)
        if on:
            s.set_collider_mesh(v, t, origin, spacing, dims, CR.MARGIN, negate=True)
        w = s.steps(p, 60).pstar()[:, :3].astype(np.float64) * CR.SCALE
        counts.append(int((np.linalg.norm(w - centre, axis=1) > r - CR.MARGIN + spacing).sum()))
    print(f"particles beyond r - margin + spacing: {counts[0]} with the mesh bowl, {counts[1]} without")
    assert counts[0] == 0 and counts[1] > 0, counts


# ---- 11. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_alone(pkg):
    from pbf_sph_amd import capi
    sc = scene("cloud")
    lat, phi64, _ = plane_through(sc, np.float32)
    p = pkg.default_params(4, 1000.0)
    s = solver(pkg, False).upload(**sc)
    L = s.L
    set_lattice(s, lat, phi64, BOX_LATTICE["spacing"]).steps(p, 2)
    pts = np.random.default_rng(2).random((500, 3)) * 1000.0
    before, sample, gen = state_bytes(s), s.collider_sample(p, pts), s.graph_stats()
    v, t = MS.shape("ico2")
    good, keep = capi.mesh_struct(v, t)
    out = np.full(BOX_LATTICE["dims"], 777.0, np.float32)
    OUT = out.ctypes.data_as(C.c_void_p)

    def sdf(dims=BOX_LATTICE["dims"], origin=BOX_LATTICE["origin"], spacing=BOX_LATTICE["spacing"], margin=CR.MARGIN):
        d = capi.ColliderSdf()
        d.dims[:], d.origin[:] = list(dims), list(origin)
        d.spacing, d.margin, d.phi = spacing, margin, None
        return d

    # every invalid lattice of test_collider_gpu's refusal test (phi is ignored here; margin is the installing call's)
    bad = {"a dim < 2": sdf(dims=(1, 23, 23)), "2^31 nodes": sdf(dims=(2048, 1024, 1024)), "dim 0": sdf(dims=(23, 0, 23)),
           "origin nan": sdf(origin=(0.0, np.nan, 0.0)), "origin inf": sdf(origin=(np.inf, 0.0, 0.0)),
           "spacing 0": sdf(spacing=0.0), "spacing < 0": sdf(spacing=-1.0), "spacing nan": sdf(spacing=np.nan), "spacing inf": sdf(spacing=np.inf)}
    margins = {"margin < 0": sdf(margin=-0.5), "margin nan": sdf(margin=np.nan), "margin inf": sdf(margin=np.inf)}
    for what, d in bad.items():
        assert L.pbf_sdf_from_mesh(s.ctx, C.byref(good), C.byref(d), 0, OUT, None) == ERR_INVALID, what
        assert L.pbf_set_collider_mesh(s.ctx, C.byref(good), C.byref(d), 0, None) == ERR_INVALID, what
    for what, d in margins.items():
        assert L.pbf_set_collider_mesh(s.ctx, C.byref(good), C.byref(d), 0, None) == ERR_INVALID, what
    assert L.pbf_sdf_from_mesh(s.ctx, C.byref(good), None, 0, OUT, None) == ERR_INVALID
    assert L.pbf_set_collider_mesh(s.ctx, C.byref(good), None, 0, None) == ERR_INVALID
    assert L.pbf_sdf_from_mesh(s.ctx, C.byref(good), C.byref(sdf()), 0, None, None) == ERR_INVALID          # phi == NULL
    assert L.pbf_sdf_from_mesh(s.ctx, C.byref(good), C.byref(sdf()), 2, OUT, None) == ERR_INVALID           # unknown flag
    assert L.pbf_set_collider_mesh(s.ctx, C.byref(good), C.byref(sdf()), 1 << 7, None) == ERR_INVALID
    # broken meshes
    assert L.pbf_sdf_from_mesh(s.ctx, None, C.byref(sdf()), 0, OUT, None) == ERR_INVALID
    for name in ("open", "flipped", "duplicate"):
        bv, bt, _, _ = MS.broken(name)
        m, keep2 = capi.mesh_struct(bv, bt)
        st = capi.MeshSdfStats(5, 6)
        assert L.pbf_sdf_from_mesh(s.ctx, C.byref(m), C.byref(sdf()), 0, OUT, C.byref(st)) == ERR_INVALID, name
        assert b"pbf_mesh_records" in L.pbf_last_error(s.ctx)
        assert L.pbf_set_collider_mesh(s.ctx, C.byref(m), C.byref(sdf()), 0, C.byref(st)) == ERR_INVALID, name
        assert (st.pairs_total, st.pairs_tested) == (5, 6)
    # everything refused: the output array, the collider, the particles and the captured-step key are what they were
    assert (out == 777.0).all()
    again = s.collider_sample(p, pts)
    assert all(again[k].tobytes() == sample[k].tobytes() for k in sample)
    assert state_bytes(s) == before and s.graph_stats() == gen
    # pbf_sdf_from_mesh that succeeds leaves the collider alone too
    phi, _ = s.sdf_from_mesh(v, t, **BOX_LATTICE)
    again = s.collider_sample(p, pts)
    assert all(again[k].tobytes() == sample[k].tobytes() for k in sample) and state_bytes(s) == before
    # a margin that pbf_set_collider_mesh refuses is ignored by pbf_sdf_from_mesh
    assert L.pbf_sdf_from_mesh(s.ctx, C.byref(good), C.byref(sdf(margin=-1.0)), 0, OUT, None) == 0
    assert out.tobytes() == phi.tobytes()

    # slab mode: pbf_set_collider's refusals
    t2 = solver(pkg, False).upload(**sc)
    cut = capi.SlabCut(0, 12, 0, 0)
    assert L.pbf_slab_configure(t2.ctx, C.byref(cut), 0, 0) == 0
    out[:] = 777.0
    assert L.pbf_set_collider_mesh(t2.ctx, C.byref(good), C.byref(sdf()), 0, None) == ERR_STATE and b"slab" in L.pbf_last_error(t2.ctx)
    assert L.pbf_sdf_from_mesh(t2.ctx, C.byref(good), C.byref(sdf()), 0, OUT, None) == ERR_STATE and (out == 777.0).all()
    noop = capi.EXCHANGE_FN(lambda *a: 0)
    comm = C.c_void_p()
    assert L.pbf_comm_create_host_callback(noop, None, 1, 0, C.byref(comm)) == 0
    cuts = np.array([0, 1024], np.uint32)
    u = solver(pkg, False).reserve(8192).upload(**sc)
    assert L.pbf_slab_attach(u.ctx, comm, cuts.ctypes.data_as(C.c_void_p), 256, 256) == 0
    assert L.pbf_set_collider_mesh(u.ctx, C.byref(good), C.byref(sdf()), 0, None) == ERR_STATE
    u.close()
    L.pbf_comm_destroy(comm)
    s.close()
    t2.close()


# ---- 12. the shim and the CLI -----------------------------------------------------------------------------------------------
CUBE_BALL = dict(subdivisions=2, R=150.0, centre=(350.0, 100.0, 450.0))     # inside the larger of the two cubes


def test_shim(pkg, tmp_path):
    frames = 4
    v, t = MS.icosphere(**CUBE_BALL)
    with open(tmp_path / "mesh.bin", "wb") as f:
        f.write(np.array(BOX_LATTICE["dims"], np.uint32).tobytes() + np.array(BOX_LATTICE["origin"], np.float64).tobytes() +
                np.array([BOX_LATTICE["spacing"], CR.MARGIN], np.float64).tobytes() + np.array([0, len(v), len(t)], np.uint32).tobytes() +
                v.tobytes() + t.tobytes())
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_collider_mesh_shim"), str(tmp_path / "mesh.bin"), str(tmp_path / "dump.bin"),
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
    assert at == len(raw)
    # the same frames over the C ABI: advance() is upload -> step -> download
    s = solver(pkg, False)
    s.set_collider_mesh(v, t, margin=CR.MARGIN, **BOX_LATTICE)
    p = pkg.default_params(4, 1000.0)
    st = first
    for _ in range(frames):
        st = s.upload(**st).step(p).download()
    for k in last:
        assert st[k].tobytes() == last[k].tobytes(), k


def write_obj(path, v, t):
    """every index form the reader takes: a, a/b, a//c, a/b/c, and negative indices (counted back from the last vertex)"""
    with open(path, "w") as f:
        f.write("# an icosphere\no ball\n")
        for x in v:
            f.write("v {!r} {!r} {!r}\n".format(*[float(c) for c in x]))
        f.write("vt 0 0\nvn 0 0 1\ns off\n")
        for k, tri in enumerate(t):
            i = [int(x) + 1 for x in tri]
            form = k % 5
            if form == 0:
                f.write("f {} {} {}\n".format(*i))
            elif form == 1:
                f.write("f {}/1 {}/1 {}/1\n".format(*i))
            elif form == 2:
                f.write("f {}//1 {}//1 {}//1\n".format(*i))
            elif form == 3:
                f.write("f {}/1/1 {}/1/1 {}/1/1\n".format(*i))
            else:
                f.write("f {} {} {}\n".format(*[x - 1 - len(v) for x in i]))


def test_cli_mesh_collider(pkg, tmp_path):
    from test_cli_gpu import read_ply
    v, t = MS.icosphere(**CUBE_BALL)
    obj = tmp_path / "ball.obj"
    write_obj(obj, v, t)
    common = ["--scene", "cubes", "--particles", "8000", "-n", "5", "-w", "0", "--resident", "--no-surface"]
    clouds = []
    for extra, d in [([], "off"), ([f"--collider=mesh:{obj},13.5,50"], "on")]:
        r = subprocess.run([BIN, *common, *extra, "-o", str(tmp_path / d)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        clouds.append(read_ply(os.path.join(str(tmp_path), d, "cloud.ply")))
        line = [l for l in r.stdout.split("\n") if l.startswith("Collider")]
        assert bool(line) == bool(extra)
    m = re.search(r"mesh .*ball\.obj, (\d+) triangles, volume ([-+.e\d]+), lattice 23 x 23 x 23, spacing 50, margin 13\.5, pairs tested (\d+) / (\d+)", line[0])
    assert m, line
    assert int(m.group(1)) == len(t) and int(m.group(4)) == 23 ** 3 * len(t) and 0 < int(m.group(3)) <= int(m.group(4))
    assert abs(float(m.group(2)) - MR.info(v, t)["volume"]) <= 1e-4 * MR.info(v, t)["volume"]
    assert clouds[0].shape == clouds[1].shape and np.isfinite(clouds[1]).all()
    assert not np.array_equal(clouds[0], clouds[1])
    # a file the reader refuses, and a mesh the library refuses
    quad = tmp_path / "quad.obj"
    quad.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3 4\n")
    r = subprocess.run([BIN, *common, f"--collider=mesh:{quad}", "-o", str(tmp_path / "q")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "triangular" in r.stdout + r.stderr
    hole = tmp_path / "hole.obj"
    write_obj(hole, v, t[:-1])
    r = subprocess.run([BIN, *common, f"--collider=mesh:{hole}", "-o", str(tmp_path / "h")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "open" in r.stdout + r.stderr and "boundary 3" in r.stdout + r.stderr
    assert "--collider=mesh:" in subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
