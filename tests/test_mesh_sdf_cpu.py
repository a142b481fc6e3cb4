"""The mesh collider without a GPU (pbf_mesh_records / pbf_sdf_from_mesh, include/pbf_hip.h):

  1. the restatement (tests/mesh_sdf_ref.py) in float64 against closed forms: box, icosphere, torus;
  2. its sign against the generalised winding number, on every node;
  3. ties: a box whose faces pass through lattice nodes, and a permutation of the triangles;
  4. the float32 restatement against the float64 one;
  5. pbf_mesh_records through the library: records, info, every refusal;
  6. the host program test_mesh_records.

The device side: tests/test_mesh_sdf_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mesh_sdf_ref as MR
import mesh_shapes as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1
A = MS.LATTICE_A
NAMES = ["box", "tetra", "torus", "ico2"]
_cache = {}


def phi_on_a(name, dtype=np.float64):
    """the restatement's field of a shape on lattice A, computed once per (shape, dtype)"""
    key = (name, np.dtype(dtype).name)
    if key not in _cache:
        v, t = MS.shape(name)
        _cache[key] = MR.sdf(v, t, A["origin"], A["spacing"], A["dims"], dtype)
        _cache[key].setflags(write=False)
    return _cache[key]


def nodes_a():
    return MR.nodes(A["origin"], A["spacing"], A["dims"], np.float64)


# ---- 1. closed forms ---------------------------------------------------------------------------------------------------
def box_phi(lo, hi, x):
    """the box's distance with ONE rounding per axis, q = max(lo - x, x - hi); pkg.sdf_box forms |x - centre| - half, which
    is the same number in exact arithmetic but rounds x - centre first (an error of up to an ulp of that difference)"""
    q = np.maximum(np.asarray(lo, np.float64) - x, x - np.asarray(hi, np.float64))
    out = np.maximum(q, 0)
    return np.sqrt((out[..., 0] * out[..., 0] + out[..., 1] * out[..., 1]) + out[..., 2] * out[..., 2]) + np.minimum(q.max(axis=-1), 0)


def test_box_equals_the_closed_form_exactly(pkg):
    """Exactly: on a face, an edge or a corner of an axis-aligned box the components of r = p - q along the feature are
    rounding dust whose squares vanish against the others, which are single exact differences.  Against pkg.sdf_box the
    difference is sdf_box's own rounding of x - centre: at most two ulps of the largest |x - centre| (< 512)."""
    got = phi_on_a("box")
    want = box_phi(*MS.BOX, nodes_a()).reshape(got.shape)
    lib = pkg.sdf_lattice(pkg.sdf_box(*MS.BOX), A["origin"], A["spacing"], A["dims"])
    print(f"box on A: largest |restatement - closed form| = {np.abs(got - want).max()}, against sdf_box {np.abs(got - lib).max():.3e}")
    assert np.array_equal(got, want)
    assert np.abs(got - lib).max() <= 2 * np.spacing(512.0)


def test_icosphere_lies_between_the_sphere_and_its_inscribed_sphere():
    v, t = MS.shape("ico2")
    c = np.asarray(MS.CENTRE)
    rec = MR.records(v, t)
    plane = np.einsum("ij,ij->i", rec[:, 0:3] - c, rec[:, 9:12])          # face-plane distance from the centre
    gap = MS.ICO_R - plane.min()
    d = phi_on_a("ico2").reshape(-1) - (np.linalg.norm(nodes_a() - c, axis=1) - MS.ICO_R)
    print(f"ico2 on A: phi - (|x - c| - R) in [{d.min():.4f}, {d.max():.4f}], bound R - min face distance = {gap:.4f}")
    assert d.min() >= 0.0 and d.max() <= gap


def test_torus_is_within_the_meshs_deviation_of_the_closed_form():
    """every mesh point is within `dev` of the torus and every torus point within `dev` of the mesh (dev = the largest
    |closed form| over the mesh, sampled on a fine barycentric grid: the mesh is inscribed, its farthest points are face
    interiors), so the two distance fields differ by at most dev, up to the sampling's own error"""
    v, t = MS.shape("torus")
    g = np.array([(i, j, 16 - i - j) for i in range(17) for j in range(17 - i)], np.float64) / 16
    pts = np.einsum("gs,tsa->tga", g, v[t.astype(np.int64)]).reshape(-1, 3)
    dev = np.abs(MS.torus_phi(pts)).max()
    # the sampling error: between samples the closed form (1-Lipschitz) moves by at most half a sample spacing
    edge = np.linalg.norm(v[t[:, 1]] - v[t[:, 0]], axis=1).max()
    dev += edge / 16
    d = np.abs(phi_on_a("torus").reshape(-1) - MS.torus_phi(nodes_a()))
    print(f"torus on A: largest |phi - closed form| = {d.max():.4f}, mesh deviation bound {dev:.4f}")
    assert d.max() <= dev


# ---- 2. the sign, independently ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_sign_equals_the_winding_number(name):
    v, t = MS.shape(name)
    phi = phi_on_a(name).reshape(-1)
    print(f"{name} on A: smallest |phi| = {np.abs(phi).min():.4f}, {int((phi < 0).sum())} nodes inside")
    # the precondition: no node sits on a surface, by more than float32 could blur it (box 1.10, tetra 4.30, torus 0.50;
    # this icosphere 0.042)
    assert np.abs(phi).min() > 8 * MR.F32_WORST
    assert (phi < 0).any() and (phi > 0).any()
    w = MR.winding_number(v, t, nodes_a())
    assert np.array_equal(phi < 0, w > 0.5), int(((phi < 0) != (w > 0.5)).sum())


# ---- 3. ties ------------------------------------------------------------------------------------------------------------
def test_ties_on_the_box_through_lattice_nodes(pkg):
    T = MS.LATTICE_TIES
    v, t = MS.box(*MS.TIE_BOX)
    phi = MR.sdf(v, t, T["origin"], T["spacing"], T["dims"])
    want = pkg.sdf_lattice(pkg.sdf_box(*MS.TIE_BOX), T["origin"], T["spacing"], T["dims"])
    assert int((phi == 0).sum()) == 386
    assert np.array_equal(np.signbit(phi), np.signbit(want)) and np.array_equal(phi < 0, want < 0)
    assert np.array_equal(phi, want)
    perm = np.random.default_rng(5).permutation(len(t))
    assert np.array_equal(MR.sdf(v, t[perm], T["origin"], T["spacing"], T["dims"]), phi)


# ---- 4. float32 against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_float32_restatement_against_float64(name):
    p32, p64 = phi_on_a(name, np.float32), phi_on_a(name)
    assert p32.dtype == np.float32
    worst = np.abs(p32.astype(np.float64) - p64).max()
    print(f"{name} on A: largest |phi32 - phi64| = {worst:.3e} (recorded worst {MR.F32_WORST:.1e})")
    assert np.array_equal(p32 < 0, p64 < 0)
    assert worst <= 8 * MR.F32_WORST


# ---- 5. pbf_mesh_records through the library ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES + ["ico3"])
def test_library_records_equal_the_restatement(pkg, name):
    v, t = MS.shape(name)
    want, winfo = MR.records(v, t), MR.info(v, t)
    got, info = pkg.mesh_records(v, t, fp64=True)
    assert got.shape == (MS.TRIANGLES[name], 30)
    assert np.array_equal(got[:, :9], want[:, :9])
    scale = np.abs(want).max(axis=1, keepdims=True)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max() and (np.abs(got - want) <= 1e-12 * scale + 1e-300).all()
    for k in ("n_edges", "boundary_edges", "nonmanifold_edges", "misoriented_edges", "degenerate_triangles", "aabb_min", "aabb_max"):
        assert info[k] == winfo[k], k
    assert info["n_edges"] == 3 * len(t) // 2 and info["boundary_edges"] == 0
    assert abs(info["volume"] - winfo["volume"]) <= 1e-12 * abs(winfo["volume"])
    if name == "box":
        assert info["volume"] == 66_000_000.0
    if name == "tetra":
        assert info["volume"] == 4_500_000.0
    f32, _ = pkg.mesh_records(v, t, fp64=False)
    assert f32.dtype == np.float32 and np.array_equal(f32, got.astype(np.float32))
    # an inside-out mesh is legal: the volume changes sign
    _, flipped = pkg.mesh_records(v, t[:, ::-1], fp64=True)
    assert flipped["volume"] == -info["volume"] or abs(flipped["volume"] + info["volume"]) <= 1e-12 * abs(info["volume"])


def call_records(pkg, mesh, fp64=True, n_records=0):
    """the raw call -> (rc, info dict, the records buffer, which was filled with a sentinel)"""
    from pbf_sph_amd import capi
    rec = np.full((max(n_records, 1), 30), 12345.0, np.float64 if fp64 else np.float32)
    info = capi.MeshInfo()
    C.memset(C.byref(info), 0xAB, C.sizeof(info))
    rc = pkg.lib().pbf_mesh_records(None if mesh is None else C.byref(mesh), int(fp64), rec.ctypes.data_as(C.c_void_p), C.byref(info))
    return rc, info.as_dict(), rec


ZERO_INFO = dict(n_edges=0, boundary_edges=0, nonmanifold_edges=0, misoriented_edges=0, degenerate_triangles=0, volume=0.0,
                 aabb_min=(0.0,) * 3, aabb_max=(0.0,) * 3)


def test_library_refusals(pkg):
    from pbf_sph_amd import capi
    L = pkg.lib()
    v, t = MS.shape("ico2")
    good, keep = capi.mesh_struct(v, t)

    def mesh(**kw):
        m = capi.Mesh(good.n_vertices, good.n_triangles, good.vertices, good.triangles)
        for k, x in kw.items():
            setattr(m, k, x)
        return m

    nan_v, inf_v = v.copy(), v.copy()
    nan_v[17, 1], inf_v[3, 2] = np.nan, np.inf
    nothing = {"mesh NULL": None, "vertices NULL": mesh(vertices=None), "triangles NULL": mesh(triangles=None),
               "no vertices": mesh(n_vertices=0), "no triangles": mesh(n_triangles=0), "2^31 vertices": mesh(n_vertices=2 ** 31),
               "2^31 triangles": mesh(n_triangles=2 ** 31), "NaN vertex": mesh(vertices=nan_v.ctypes.data),
               "inf vertex": mesh(vertices=inf_v.ctypes.data)}
    for what, m in nothing.items():
        rc, info, rec = call_records(pkg, m, n_records=len(t))
        assert rc == ERR_INVALID and info == ZERO_INFO and (rec == 12345.0).all(), (what, info)
        assert b"pbf_mesh_records" in L.pbf_last_error(None), what
    # an index out of range: the box of the vertices, nothing else
    bad_t = t.copy()
    bad_t[9, 2] = len(v)
    rc, info, rec = call_records(pkg, mesh(triangles=bad_t.ctypes.data), n_records=len(t))
    assert rc == ERR_INVALID and (rec == 12345.0).all()
    assert info == dict(ZERO_INFO, aabb_min=tuple(v.min(axis=0)), aabb_max=tuple(v.max(axis=0)))
    # a triangle of zero area (two equal corners): counted, and everything else measured
    flat = t.copy()
    flat[4, 1] = flat[4, 0]
    rc, info, rec = call_records(pkg, mesh(triangles=flat.ctypes.data), n_records=len(t))
    assert rc == ERR_INVALID and info["degenerate_triangles"] == 1 and (rec == 12345.0).all()
    assert info == MR.info(v, flat)
    # the three broken meshes
    for name in ("open", "flipped", "duplicate"):
        bv, bt, field, count = MS.broken(name)
        m, keep2 = capi.mesh_struct(bv, bt)
        for fp64 in (True, False):
            rc, info, rec = call_records(pkg, m, fp64, n_records=len(bt))
            assert rc == ERR_INVALID and info[field] == count and (rec == 12345.0).all(), (name, info)
            want = MR.info(bv, bt)
            assert {k: info[k] for k in want if k != "volume"} == {k: want[k] for k in want if k != "volume"}, name
            assert abs(info["volume"] - want["volume"]) <= 1e-12 * abs(want["volume"])
        with pytest.raises(pkg.PbfError) as e:
            pkg.mesh_records(bv, bt)
        assert e.value.info[field] == count
    # and the good mesh still passes, with records == NULL as a check only
    info = capi.MeshInfo()
    assert L.pbf_mesh_records(C.byref(good), 1, None, C.byref(info)) == 0 and info.as_dict()["n_edges"] == 480
    assert L.pbf_mesh_records(C.byref(good), 1, None, None) == 0


# ---- 6. the host program ------------------------------------------------------------------------------------------------------
def test_host_program(pkg):
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_mesh_records")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
