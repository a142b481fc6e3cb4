"""The indexed marching-cubes mesh on the device (pbf_surface_indexed: k_mc_edge_mark, k_mc_emit_vertices,
k_mc_emit_indices) against the numpy checker tests/mc_indexed_ref.py run on the DEVICE lattice of the same call: vertices,
normals, colours and indices bit for bit, fp32 and fp64; against the device's own triangle soup under the bound derived
in tests/test_mc_indexed_cpu.py; watertight by index with zero exceptions; deterministic; the state rules of
include/pbf_hip.h; the CLI's --indexed-mesh.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mc_closed_forms as CF
import mc_indexed_ref as R
import mc_scenes as M
from test_mc_indexed_cpu import STOCK, run_checker, straddling_edges

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pbf-sph_amd", "benchmark")
ERR_STATE = -4
STOCK_MC = (2.0, 100.0, 25.0, 0.5)


def scene(name):
    """-> (scene dict of mc_scenes' shape, parameter sets)"""
    if name == "cubes":
        import oracle_lib as O
        return dict(sc=O.scene_cubes(2048, True), iteration=4, frames=3, force=(0.0, 9.8, 0.0), max_bound=(1000.0,) * 3, **STOCK), [STOCK_MC]
    if name == "one":
        return dict(CF.ONE, sc=CF._particle(CF.ONE_POS)), [CF.ONE_MC]
    return M.make(name), M.PARAMS[name]


def stepped(pkg, s, fp64):
    sol = pkg.Solver(h=s["h"], fp64=fp64)
    sol.upload(**M.cast(s["sc"], np.float64 if fp64 else np.float32))
    p = M.device_params(pkg, s)
    for _ in range(s["frames"]):
        sol.step(p)
    return sol, p


NAMES = ("cubes", "one") + M.NAMES
CASES = [(n, fp64) for n in NAMES for fp64 in (False, True)]
IDS = [f"{n}-{'f64' if d else 'f32'}" for n, d in CASES]


@pytest.mark.parametrize("name,fp64", CASES, ids=IDS)
def test_indexed_bit_equal_to_checker_on_device_lattice(pkg, name, fp64):
    s, params = scene(name)
    sol, p = stepped(pkg, s, fp64)
    try:
        for mc in params:
            g = sol.surface_indexed(p, pkg.McParams(*mc))
            ix, _ = run_checker(g, s, mc, fp64)
            assert len(g["tris"]) > 40 and g["tris"].dtype == np.uint32
            assert len(g["vs"]) == len(ix["vs"]) == straddling_edges(g["sample"], g["pn"][:, 0], mc[1]), mc
            assert np.array_equal(g["tris"], ix["tris"]), mc
            for k in ("vs", "ns", "cs"):
                assert g[k].dtype == ix[k].dtype and np.array_equal(g[k], ix[k], equal_nan=True), (mc, k)
            assert np.unique(g["tris"]).size == len(g["vs"])
    finally:
        sol.close()


@pytest.mark.parametrize("name,fp64", CASES, ids=IDS)
def test_indexed_against_device_soup(pkg, name, fp64):
    s, params = scene(name)
    sol, p = stepped(pkg, s, fp64)
    try:
        for mc in params:
            soup = sol.surface(p, pkg.McParams(*mc))
            g = sol.surface_indexed(p, pkg.McParams(*mc))
            assert len(soup["vs"]) == 3 * len(g["tris"])                       # the same T
            assert np.array_equal(soup["sample"], g["sample"])
            for k in ("pn", "c"):                                              # identical lattices
                assert np.array_equal(soup[k], g[k], equal_nan=True), (mc, k)
            ix, consts = run_checker(g, s, mc, fp64)
            dev = dict(ix, vs=g["vs"], ns=g["ns"], cs=g["cs"], tris=g["tris"])  # the device's arrays, the checker's edge labels
            rep = R.compare_with_soup(dev, soup, (g["sample"], g["pn"], g["c"]), consts, mc[1])
            print(f"RATIO device {name} {mc} {'f64' if fp64 else 'f32'}: V={len(g['vs'])} T={len(g['tris'])} +edges "
                  f"{rep['n_pos']} -edges {rep['n_neg']} inf {rep['n_inf']} largest error / bound {rep['worst']:.3f}")
            assert rep["n_pos"] + rep["n_neg"] + rep["n_inf"] == len(soup["vs"])
            if name in ("one", "blob", "cubes") and mc in (CF.ONE_MC, STOCK_MC):
                # closed scenes: watertight BY INDEX, no tolerance (the soup's quantised check tolerates 0.2 %)
                bad, edges = R.directed_edge_defects(g["tris"])
                assert bad == 0 and edges > 0, (bad, edges)
                v, t = len(g["vs"]), len(g["tris"])
                chi = v - edges + t
                assert v == t // 2 + chi and t % 2 == 0
                if name == "one":
                    assert chi == 2
    finally:
        sol.close()


@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
def test_indexed_is_deterministic(pkg, fp64):
    s, _ = scene("cubes")
    sol, p = stepped(pkg, s, fp64)
    try:
        a = sol.surface_indexed(p, pkg.McParams(*STOCK_MC))
        b = sol.surface_indexed(p, pkg.McParams(*STOCK_MC))
        assert len(a["tris"]) > 2000
        for k in ("vs", "ns", "cs", "tris", "pn", "c"):
            assert a[k].tobytes() == b[k].tobytes(), k
    finally:
        sol.close()


@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
def test_indexed_state_rules(pkg, fp64):
    s, _ = scene("cubes")
    sol, p = stepped(pkg, s, fp64)
    L = sol.L
    try:
        mc = pkg.McParams(*STOCK_MC)
        g = sol.surface_indexed(p, mc)
        v, t = len(g["vs"]), len(g["tris"])
        buf = np.empty((9 * t + 16, 4), sol.dtype)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        # after pbf_surface_indexed there is no soup
        assert L.pbf_download_mesh(sol.ctx, ptr(buf), None, None) == ERR_STATE
        pv, pn, pc, pt = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert L.pbf_map_mesh(sol.ctx, C.byref(pv), C.byref(pn), C.byref(pc)) == ERR_STATE
        # the page-locked view holds the same bytes as the download; NULL pointers are skipped
        assert L.pbf_map_mesh_indexed(sol.ctx, C.byref(pv), C.byref(pn), C.byref(pc), C.byref(pt)) == 0
        e = np.dtype(sol.dtype).itemsize
        assert C.string_at(pv.value, 3 * v * e) == g["vs"].tobytes() and C.string_at(pn.value, 3 * v * e) == g["ns"].tobytes()
        assert C.string_at(pc.value, 4 * v * e) == g["cs"].tobytes() and C.string_at(pt.value, 12 * t) == g["tris"].tobytes()
        only = np.empty((t, 3), np.uint32)
        assert L.pbf_download_mesh_indexed(sol.ctx, None, None, None, ptr(only)) == 0 and np.array_equal(only, g["tris"])
        # after pbf_surface there is no indexed mesh
        soup = sol.surface(p, mc)
        assert len(soup["vs"]) == 3 * t
        assert L.pbf_download_mesh_indexed(sol.ctx, ptr(buf), None, None, None) == ERR_STATE
        assert L.pbf_map_mesh_indexed(sol.ctx, C.byref(pv), C.byref(pn), C.byref(pc), C.byref(pt)) == ERR_STATE
        # ... and the soup is what it was before the indexed call existed
        again = sol.surface(p, mc)
        for k in ("vs", "ns", "cs"):
            assert soup[k].tobytes() == again[k].tobytes()
        # a slab-configured ctx is refused
        cut = pkg.SlabCut(0, int(sol.extent()[0][0]), 0, 0)
        assert L.pbf_slab_configure(sol.ctx, C.byref(cut), 0, 0) == 0
        nv, nt = C.c_uint64(7), C.c_uint64(7)
        assert L.pbf_surface_indexed(sol.ctx, C.byref(p), C.byref(mc), C.byref(nv), C.byref(nt)) == ERR_STATE
        assert b"slab" in L.pbf_last_error(sol.ctx)
    finally:
        sol.close()


@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
def test_indexed_empty_surface(pkg, fp64):
    """One particle, lattice step 400 world units: the nearest node is 170 from it, the isosurface's radius is 64 — no
    edge straddles the isolevel."""
    s, _ = scene("one")
    sol, p = stepped(pkg, s, fp64)
    try:
        mc = (0.25,) + CF.ONE_MC[1:]
        g = sol.surface_indexed(p, pkg.McParams(*mc))
        assert min(int(x) for x in g["sample"]) >= 2
        assert straddling_edges(g["sample"], g["pn"][:, 0], mc[1]) == 0
        assert len(g["vs"]) == 0 and len(g["tris"]) == 0
    finally:
        sol.close()


def run_cli(*args):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_cli_indexed_mesh(pkg, tmp_path):
    txt = run_cli("-n", "3", "-w", "2", "--indexed-mesh", "-o", str(tmp_path / "ix"))
    m = re.search(r"Indexed mesh         : (\d+) vertices, (\d+) triangles", txt)
    assert m, txt
    v, t = int(m.group(1)), int(m.group(2))
    assert "Final Vertex count   : 0" in txt and "Results flushed." in txt
    lines = open(tmp_path / "ix" / "mesh.obj").read().split("\n")
    vl = [l for l in lines if l.startswith("v ")]
    nl = [l for l in lines if l.startswith("vn ")]
    fl = [l for l in lines if l.startswith("f ")]
    assert len(vl) == len(nl) == v > 1000 and len(fl) == t > 2000
    assert all(len(l.split()) == 4 for l in vl + nl)
    idx = []
    for l in fl:
        parts = l.split()[1:]
        assert len(parts) == 3
        for q in parts:
            a, mid, b = q.split("/")
            assert mid == "" and a == b
            idx.append(int(a))
    idx = np.array(idx)
    assert idx.min() >= 1 and idx.max() <= v and np.unique(idx).size == v
    # the same frames through the C ABI (the stock scene: 20000 nominal particles, 6 iterations, the box in motion;
    # warm-up frames 0, 1, then timed frames 0, 1, 2 — the surface of the last one)
    sc = pkg.scene_cubes(20000)
    s = pkg.Solver(h=0.1)
    try:
        s.upload(**sc)
        base = pkg.default_params(6, 1000.0)
        for frame in (0, 1, 0, 1, 2):
            s.step(pkg.apply_motion(base, frame, False))
        g = s.surface_indexed(pkg.apply_motion(base, 2, False), pkg.McParams())
        assert (len(g["vs"]), len(g["tris"])) == (v, t)
        assert np.array_equal(g["tris"].reshape(-1) + 1, idx)
        got = np.array([[float(x) for x in l.split()[1:]] for l in vl])
        np.testing.assert_allclose(got, g["vs"].astype(np.float64), rtol=1e-5, atol=1e-3)   # (the OBJ prints 6 digits)
    finally:
        s.close()
    # without the flag: the soup, as before — no extra line, 3 `v` per `f`, the same triangle count
    plain = run_cli("-n", "3", "-w", "2", "-o", str(tmp_path / "soup"))
    assert "Indexed mesh" not in plain
    n = int(re.search(r"Final Vertex count   : (\d+)", plain).group(1))
    assert n == 3 * t
    obj = open(tmp_path / "soup" / "mesh.obj").read().split("\n")
    assert sum(1 for l in obj if l.startswith("v ")) == n and sum(1 for l in obj if l.startswith("f ")) == n // 3
    labels = lambda out: [l.split(":")[0] for l in out.split("\n") if ":" in l]  # noqa: E731
    assert [l for l in labels(txt) if not l.startswith("Indexed mesh")] == labels(plain)


def test_cli_indexed_mesh_refuses_slabs():
    r = subprocess.run([BIN, "--indexed-mesh", "--slabs", "2", "-n", "1", "-w", "0", "-o", ""], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--indexed-mesh is a single-device feature" in r.stderr
