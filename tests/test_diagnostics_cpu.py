"""pbf_diagnostics without a GPU: the entry point and its record are declared, exported and bound with the header's layout;
the reference the GPU tests use (tests/diagnostics_ref.py) agrees with closed forms that share nothing with it; and the
scenes those tests run on contain what they are said to contain — in particular, hardly any pair sits so close to r = h
that the neighbour-count bracket [h (1 - delta), h (1 + delta)] could hide a wrong count."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import diagnostics_ref as DR
import nversion as NV
import oracle_lib as O
from test_nversion_cpu import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 0.1
SCENES = ["cubes1024", "cloud", "obstacles"]


def header():
    return open(os.path.join(ROOT, "include", "pbf_hip.h")).read()


def test_entry_point_is_declared_exported_and_bound(pkg):
    from pbf_sph_amd import capi
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"int pbf_diagnostics\(pbf_ctx \*ctx, const pbf_params \*params, uint32_t what, pbf_diag \*out\);", code)
    assert re.search(r"typedef struct pbf_diag \{.*?\} pbf_diag;", code, flags=re.S)
    assert re.search(r"PBF_DIAG_DENSITY = 1u << 0", code)
    assert hasattr(C.CDLL(pkg.LIB_PATH), "pbf_diagnostics")
    assert "pbf_diagnostics" in capi.exported_symbols()
    f = pkg.lib().pbf_diagnostics
    assert f.restype is C.c_int and f.argtypes[3]._type_ is capi.Diag
    assert callable(pkg.Solver.diagnostics) and callable(pkg.Solver.density)
    assert pkg.Diag is capi.Diag and pkg.DIAG_DENSITY == 1 and pkg.BUF_DENSITY == 6
    assert PBF_ABI_VERSION_is_one(code)


def PBF_ABI_VERSION_is_one(code):
    return re.search(r"#define PBF_ABI_VERSION 1\b", code) is not None


def test_struct_layout_matches_the_header(pkg):
    from pbf_sph_amd import capi
    assert C.sizeof(capi.Diag) == (3 + 15 + 2 + 7) * 8 == 216
    # the same members in the same order as the header's struct
    body = re.search(r"typedef struct pbf_diag \{(.*?)\} pbf_diag;", header(), flags=re.S).group(1)
    names = re.findall(r"(\w+)(?:\[3\])?\s*[,;]", body)
    assert names == [n for n, _ in capi.Diag._fields_]
    arrays = set(re.findall(r"(\w+)\[3\]", body))
    assert arrays == {n for n, t in capi.Diag._fields_ if C.sizeof(t) == 24}
    ints = re.findall(r"uint64_t ([^;]*);", body)
    assert {n.strip() for line in ints for n in line.split(",")} == {n for n, t in capi.Diag._fields_ if t is C.c_uint64}


def test_density_buffer_is_number_six():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"PBF_BUF_DENSITY = 6,", code) and re.search(r"PBF_BUF_COUNT_ = 7,", code)


# ---- the reference against closed forms ------------------------------------------------------------------------------

def test_reference_rigid_block():
    """A block moving rigidly at v: momentum = M v, kinetic = M |v|^2 / 2, centre of mass = the block's centre."""
    ax = (np.arange(6) - 2.5) * 27.0
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3) + np.array([400.0, 500.0, 600.0])
    n = len(g)
    v = np.array([0.25, -1.5, 0.75])        # (exactly representable: the closed forms are exact up to summation)
    d = dict(type=np.zeros(n, np.uint8), mass=np.full(n, 2.0), pos=g, vel=np.tile(v, (n, 1)))
    d["type"][::7] = 1                       # obstacles are counted and take no part in any sum
    fluid = d["type"] == 0
    M = 2.0 * fluid.sum()
    r = DR.stream(d)
    assert r["n_fluid"] == fluid.sum() and r["n_obstacle"] == n - fluid.sum() and r["n_nonfinite"] == 0
    assert r["mass"] == M
    assert np.allclose(r["momentum"], M * v, rtol=1e-14, atol=0)
    assert np.isclose(r["kinetic"], 0.5 * M * (v @ v), rtol=1e-14)
    assert np.isclose(r["max_speed"], np.sqrt(v @ v), rtol=1e-15)
    assert np.allclose(r["moment"] / r["mass"], g[fluid].mean(0), rtol=1e-13)
    d["type"][:] = 0                          # the whole block: its centre is the lattice's
    r = DR.stream(d)
    assert np.allclose(r["moment"] / r["mass"], [400.0, 500.0, 600.0], rtol=1e-13)
    assert np.array_equal(r["aabb_min"], g.min(0)) and np.array_equal(r["aabb_max"], g.max(0))
    # non-finite fluid particles are counted and left out of everything else
    d["vel"][3, 1] = np.inf
    d["pos"][11, 2] = np.nan
    r2 = DR.stream(d)
    assert r2["n_nonfinite"] == 2 and r2["n_fluid"] == n - 2 and r2["mass"] == 2.0 * (n - 2)
    assert np.isfinite(r2["kinetic"]) and np.isfinite(r2["moment"]).all()
    # none at all: zeros
    d["type"][:] = 1
    r3 = DR.stream(d)
    assert r3["n_fluid"] == 0 and r3["n_obstacle"] == n and r3["mass"] == 0.0 and not r3["aabb_max"].any()


def test_reference_rest_lattice_density():
    """A cubic lattice at spacing rho0^(-1/3): interior rho within 1.2 % of rho0 (tests/test_physics_gpu.py's figure)."""
    a = DR.RHO0 ** (-1.0 / 3.0)
    ax = np.arange(9) * a
    ps = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    n = len(ps)
    rho, lo, hi = DR.density(ps, np.ones(n), H, np.zeros(n, bool), None)
    inner = (np.abs(ps - 4 * a) <= 2 * a + 1e-12).all(1)     # h / a = 1.85: two lattice steps from every face
    assert inner.sum() == 125
    assert np.abs(rho[inner] / DR.RHO0 - 1.0).max() <= 0.012
    assert np.array_equal(lo, hi) and len(set(lo[inner])) == 1  # every interior particle sees the same shell
    f = DR.density_fields(rho, lo, np.zeros(n, bool))
    assert f["n_density"] == n and f["rho_max"] == rho.max() and f["nbr_max"] == lo.max()
    assert f["err_mean"] >= f["compression_mean"] >= 0 and f["err_max"] >= f["err_mean"]


def test_reference_two_particles():
    for r, want in [(0.05, 1), (0.0999, 1), (0.1001, 0), (0.2, 0), (0.0, 1)]:
        ps = np.array([[0.3, 0.3, 0.3], [0.3 + r, 0.3, 0.3]])
        rho, lo, hi = DR.density(ps, np.ones(2), H, np.zeros(2, bool), None)
        assert list(lo) == [want, want] and list(hi) == [want, want], r
        w = NV.poly6_factor(H) * H ** 6 + (NV.poly6_factor(H) * (H * H - r * r) ** 3 if r <= H else 0.0)
        assert np.allclose(rho, w, rtol=1e-14)
    # an obstacle is a candidate and has no record of its own
    rho, lo, hi = DR.density(np.array([[0.3, 0.3, 0.3], [0.35, 0.3, 0.3]]), np.ones(2), H, np.array([False, True]), None)
    assert list(lo) == [1, 0] and rho[1] == 0.0 and rho[0] > NV.poly6_factor(H) * H ** 6


# ---- the scenes -------------------------------------------------------------------------------------------------------

def test_scenes_contain_what_they_claim():
    cl, ob = scene("cloud"), scene("obstacles")
    assert (ob["type"] == 1).sum() > 100 and len(np.unique(ob["mass"])) > 100
    assert (cl["pos"][:, 0] == 0.0).sum() >= 40 and (cl["pos"][:, 1] == 1000.0).sum() >= 40   # ON the box walls
    d = cl["pos"][80:90] - cl["pos"][90:100]
    assert not d.any()                                                                          # coincident pairs
    assert (scene("cubes1024")["type"] == 0).all()


_FINAL = {}


def final_pstar(name):
    """the oracle's final pStar after the step the GPU tests take (K = 2; cubes1024 after 3 warm steps), its obstacle mask and
    predict-time cells"""
    if name not in _FINAL:
        q = O.make_params(iteration=2, mode=O.JACOBI, sort=O.SORT_STABLE)
        o = O.Oracle(True)
        o.set_particles(**scene(name))
        for _ in range(3 if name == "cubes1024" else 0):
            o.step(q)
        o.predict(q).sort(q).grid_table(q)
        cells = NV.predict_cells(o.pstar().astype(np.float64), q.h, q.scale, list(q.min_bound))
        for _ in range(2):
            o.lambda_(q).delta(q)
        o.finalise(q)
        _FINAL[name] = (o.pstar().astype(np.float64), o.get_particles()["type"] == 1, cells)
    return _FINAL[name]


@pytest.mark.parametrize("name", SCENES)
def test_hardly_any_pair_sits_on_the_kernel_radius(name):
    """delta = 16 eps_N (the fp32 one: the wider window).  At most 0.1 % of the particles may have a pair with r in
    (h (1 - delta), h (1 + delta)]: the cap that keeps the GPU tests' neighbour-count bracket from hiding a failure."""
    ps, obstacle, cells = final_pstar(name)
    delta = 16 * float(np.finfo(np.float32).eps)
    r, _ = NV.pair_tables(ps, H, cells)
    near = (r > H * (1 - delta)) & (r <= H * (1 + delta))
    touched = int(near.any(1).sum())
    print(name, "particles with a pair on the radius:", touched, "of", len(ps))
    assert touched <= 0.001 * len(ps)
    # and the state is a real test of the density part: fluid away from rest density, coincident pairs where claimed
    rho, lo, hi = DR.density(ps, np.ones(len(ps)), H, obstacle, cells, delta)
    assert (lo <= hi).all() and hi.max() >= 20
