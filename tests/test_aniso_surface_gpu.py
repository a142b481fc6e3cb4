"""pbf_surface_anisotropic on a GPU: the device lattice against the all-pairs float64 checker (tests/aniso_surface_ref.py)
inside its counted bound; the nodes without hits, and no NaN anywhere; count, emit and the indexed mesh bit for bit against
the oracle's emit stage and tests/mc_indexed_ref.py on the device lattice; a closed form that shares nothing with the
checker; equal bytes call after call and under every gather setting; that the call observes without changing what a step or
pbf_surface does; its refusals; the benchmark flag and the C++ shim.

Both sides start from the same bits: the records (centre, G, radii) are read back with anisotropy(), positions, colours and
types with download(), the predict-time cells as tests/test_mc_field_gpu.py obtains them.  The bound and the band of nodes
left out are the checker's (its module text counts them); the 1 % cap on the band is a condition on the scenes, shown to
hold on the oracle's states in tests/test_aniso_surface_cpu.py.  The project's 1e-12 sum|t| bar for fp64 is not asserted as
well: the coordinate error is amplified by |G''| |a|, up to about 1e4, and the counted bound is the bar.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aniso_surface_ref as AS
import mc_closed_forms as CF
import mc_indexed_ref as R
import mc_scenes as M
import nversion_mc as NM
import oracle_lib as O
from test_aniso_surface_cpu import ISO, SCENES, kernel_of, make
from test_mc_indexed_cpu import run_checker, straddling_edges

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pbf-sph_amd", "benchmark")
ERR_INVALID, ERR_STATE = -1, -4
RESOLUTIONS = (1.0, 1.5, 2.0, 3.0)       # non-integer steps, lattice sides that are no multiple of 4
CLOSED = ("obstacles", "blob", "cloud", "sparse", "pair")   # the fluid stays clear of the lattice's faces: a closed surface

_STATE = {}


def device_state(pkg, name, fp64):
    """-> (solver, params, downloaded state, predict-time cells, scene, records read back), made once and left unchanged"""
    key = (name, fp64)
    if key not in _STATE:
        s = make(name)
        dt = np.float64 if fp64 else np.float32
        sol = pkg.Solver(h=s["h"], fp64=fp64)
        sol.upload(**M.cast(s["sc"], dt))
        p = M.device_params(pkg, s)
        for _ in range(s["frames"] - 1):
            sol.step(p)
        before = sol.download()
        sol.step(p)
        st = sol.download()
        an = sol.anisotropy(p, **kernel_of(name))
        _STATE[key] = (sol, p, st, M.predict_time_cells(before, s, st["id"]), s, an)
    return _STATE[key]


def records(an, st, lat, dtype):
    return AS.records(an["centre"], an["G"], an["radii"], st["pos"], st["type"], lat.h, lat.scale, dtype)


CASES = [(n, fp64) for n in SCENES for fp64 in (False, True)]
IDS = [f"{n}-{'f64' if d else 'f32'}" for n, d in CASES]


@pytest.mark.parametrize("name,fp64", CASES, ids=IDS)
def test_device_field_within_counted_bound_and_emission_bit_for_bit(pkg, name, fp64):
    sol, p, st, cells, s, an = device_state(pkg, name, fp64)
    dtype = sol.dtype
    o = O.Oracle(fp64, device_pow=True)
    o.set_particles(**M.cast(s["sc"], dtype))
    q = M.oracle_params(s)
    for _ in range(s["frames"]):          # (the oracle's emit stage takes its grid from its last step)
        o.step(q)
    for res in RESOLUTIONS:
        lat = M.lattice_of(s, (res,), fp64)
        fluid = st["type"] != NM.OBSTACLE
        assert (cells[fluid] >= 0).all() and (cells[fluid] < lat.extent).all(), "a particle outside the grid"
        g = sol.surface_anisotropic(p, res, ISO, **kernel_of(name))
        assert list(g["sample"]) == list(lat.sample)
        rec = records(an, st, lat, dtype)
        rep = AS.compare(g["pn"], g["c"], rec, st["colour"], cells, lat, dtype)
        print("RATIO device", name, res, "f64" if fp64 else "f32", AS.summary(rep))
        assert rep["nan"] == 0 and rep["pattern_bad"] == 0, AS.summary(rep)
        assert rep["worst"] <= 1, AS.summary(rep)
        assert rep["left_out"] <= 0.01 * rep["with_hits"], AS.summary(rep)
        assert rep["pre"] >= 1.4, "the pre-test must never decide a hit"
        for k in ("vs", "ns", "cs"):
            assert np.isfinite(g[k]).all(), k
        # count + emit: the oracle's emit stage on the device lattice, bit for bit
        e = o.surface(q, O.OracleMc(res, ISO, 0.0, 0.0), lattice=(g["sample"], g["pn"], g["c"]))
        assert len(e["vs"]) == len(g["vs"]) > 0
        for k in ("vs", "ns", "cs"):
            assert np.array_equal(g[k], e[k]), (res, k)
        # the indexed mesh: the same lattice, the checker's vertices and indices bit for bit, watertight by index
        gi = sol.surface_anisotropic(p, res, ISO, indexed=True, **kernel_of(name))
        for k in ("pn", "c"):
            assert gi[k].tobytes() == g[k].tobytes(), (res, k)
        mc = (res, ISO, 0.0, 0.0)
        ix, _ = run_checker(gi, s, mc, fp64)
        assert 3 * len(gi["tris"]) == len(g["vs"])
        assert len(gi["vs"]) == len(ix["vs"]) == straddling_edges(gi["sample"], gi["pn"][:, 0], ISO)
        assert np.array_equal(gi["tris"], ix["tris"])
        for k in ("vs", "ns", "cs"):
            assert gi[k].dtype == ix[k].dtype and np.array_equal(gi[k], ix[k]), (res, k)
        sx, sy, sz = (int(v) for v in gi["sample"])
        phi = gi["pn"][:, 0].reshape(sx, sy, sz)
        shell = np.ones((sx, sy, sz), bool)
        shell[1:-1, 1:-1, 1:-1] = False
        closed = not (phi[shell] >= dtype(ISO)).any()
        assert closed or name not in CLOSED
        if closed:   # every undirected edge in exactly two triangles, in opposite directions
            bad, edges = R.directed_edge_defects(gi["tris"])
            assert bad == 0 and edges > 0, (res, bad, edges)


def test_the_scenes_hold_every_case(pkg):
    """asserted on the read-back records and cells of the fp32 states"""
    seen = set()
    for name in SCENES:
        sol, p, st, cells, s, an = device_state(pkg, name, False)
        lat = M.lattice_of(s, (2.0,), False)
        rec = records(an, st, lat, np.float32)
        fluid = st["type"] == 0
        _, per_cell = np.unique(cells, axis=0, return_counts=True)
        seen |= {f"cell of {k}" for k in (1, 4, 5) if (per_cell == k).any()}
        if ((cells[fluid] == 0) | (cells[fluid] == lat.extent - 1)).any():
            seen.add("face cell")
        if (~fluid).any():
            seen.add("obstacles")
            assert not rec["ok"][~fluid].any()
        if (fluid & (an["neighbours"] == 0)).any():
            seen.add("isolated")
            alone = fluid & (an["neighbours"] == 0)
            assert (an["radii"][alone] == np.float32(0.5)).all()                       # the isotropic branch: radii = k_n
        if (rec["f"][rec["ok"]] == 1).any():
            seen.add("f == 1")
        if (rec["f"][rec["ok"]] > 1).any():
            seen.add("f > 1")
        if name == "pair":
            bad = fluid & ~rec["ok"]
            assert bad.sum() == 2 and (an["neighbours"][bad] == 1).all() and not np.isfinite(an["G"][bad]).all()
            assert np.array_equal(st["pos"][bad][0], st["pos"][bad][1])
            seen.add("skipped non-finite record")
    assert seen == {"cell of 1", "cell of 4", "cell of 5", "face cell", "obstacles", "isolated", "f == 1", "f > 1",
                    "skipped non-finite record"}, seen


# ---- a closed form that shares nothing with the checker ----------------------------------------------------------------

@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("k_n,iso", [(0.9, 0.08), (0.7, 0.3)])
def test_one_isolated_particle(pkg, fp64, k_n, iso):
    """k_n <= 0.99 (f == 1): phi = (1 - r^2 / (H k_n)^2)^3 / k_n^3, so the surface is the sphere of radius
    H k_n sqrt(1 - (iso k_n^3)^(1/3)) around the particle"""
    s = dict(CF.ONE, sc=CF._particle(CF.ONE_POS))
    dtype = np.float64 if fp64 else np.float32
    sol = pkg.Solver(h=s["h"], fp64=fp64)
    try:
        sol.upload(**M.cast(s["sc"], dtype))
        p = M.device_params(pkg, s)
        sol.step(p)
        down = sol.download()
        centre = down["pos"][0].astype(np.float64)
        res = 3.0
        g = sol.surface_anisotropic(p, res, iso, indexed=True, k_n=k_n, min_neighbours=8)
        lat = M.lattice_of(s, (res,), fp64)
        Hk = lat.threshold * float(dtype(k_n))
        radius = Hk * np.sqrt(1 - (iso * float(dtype(k_n)) ** 3) ** (1 / 3))
        assert 1.5 * lat.step * lat.scale < radius < Hk
        a = np.stack(np.meshgrid(*lat.coord, indexing="ij"), -1).reshape(-1, 3)
        r = np.sqrt(((a - centre) ** 2).sum(1))
        want = np.where(r < Hk, (1 - (r / Hk) ** 2) ** 3 / float(dtype(k_n)) ** 3, 0.0)
        tol = 64 * NM.unit_roundoff(dtype) * (1 + np.abs(a).max() / (Hk - r.clip(max=Hk * (1 - 1e-3))))   # |a| / distance to the edge
        inside = r < Hk * (1 - 1e-3)
        assert inside.sum() > 30 and np.all(np.abs(g["pn"][inside, 0] - want[inside]) <= tol[inside] * want.max())
        assert not g["pn"][r > Hk * (1 + 1e-3)].any()
        # every vertex lies on a lattice edge whose ends straddle the radius
        ix, _ = run_checker(g, s, (res, iso, 0.0, 0.0), fp64)
        assert np.array_equal(g["tris"], ix["tris"]) and len(g["vs"]) == len(ix["vs"]) > 30
        stride = np.array([int(g["sample"][1]) * int(g["sample"][2]), int(g["sample"][2]), 1])
        lo, hi = r[ix["owner"]], r[ix["owner"] + stride[ix["axis"]]]
        assert np.all((np.minimum(lo, hi) < radius) & (radius < np.maximum(lo, hi)))
        # closed, a sphere by index: V - E + F = 2; the normals point outwards
        bad, edges = R.directed_edge_defects(g["tris"])
        assert bad == 0 and len(g["vs"]) - edges + len(g["tris"]) == 2
        out = (g["ns"].astype(np.float64) * (g["vs"].astype(np.float64) - centre)).sum(1)
        assert np.isfinite(g["ns"]).all() and (out > 0).all()
        # one colour everywhere: a far node's mean of up to three equal colours (2 roundings), then mix (4), rounded up
        # (the particle's colour as the step left it: the diffusion stage has run on it)
        assert np.abs(g["cs"] - down["colour"][0]).max() <= 4 * np.finfo(dtype).eps
    finally:
        sol.close()


# ---- the same bytes ----------------------------------------------------------------------------------------------------

KEYS = ("vs", "ns", "cs", "pn", "c")


@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
def test_the_same_bytes_call_after_call_and_under_every_gather_setting(pkg, fp64):
    s = make("obstacles")
    base = None
    for gather in (1, 0):
        for row_major in (1, 0):
            sol = pkg.Solver(h=s["h"], fp64=fp64)
            try:
                sol.set_option("gather", gather)
                sol.set_option("row_major", row_major)
                sol.upload(**M.cast(s["sc"], sol.dtype))
                p = M.device_params(pkg, s)
                for _ in range(s["frames"]):
                    sol.step(p)
                a = sol.surface_anisotropic(p, 2.0, ISO, **kernel_of("obstacles"))
                b = sol.surface_anisotropic(p, 2.0, ISO, **kernel_of("obstacles"))
                assert len(a["vs"]) > 3000
                base = base or a
                for k in KEYS:
                    assert a[k].tobytes() == b[k].tobytes() == base[k].tobytes(), (gather, row_major, k)
            finally:
                sol.close()


@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
def test_the_call_changes_nothing_a_step_or_the_stock_surface_sees(pkg, fp64):
    s = make("obstacles")
    sols = []
    for _ in range(2):
        sol = pkg.Solver(h=s["h"], fp64=fp64)
        sol.upload(**M.cast(s["sc"], sol.dtype))
        sols.append(sol)
    a, b = sols
    try:
        p = M.device_params(pkg, s)
        for _ in range(s["frames"]):
            a.step(p), b.step(p)
        before = a.surface(p, pkg.McParams())
        a.surface_anisotropic(p, 2.0, ISO, **kernel_of("obstacles"))
        a.surface_anisotropic(p, 1.5, ISO, indexed=True, **kernel_of("obstacles"))
        after = a.surface(p, pkg.McParams())
        assert len(before["vs"]) > 3000
        for k in KEYS:
            assert before[k].tobytes() == after[k].tobytes(), k
        a.step(p), b.step(p)
        da, db = a.download(), b.download()
        assert all(np.array_equal(da[k], db[k]) for k in da) and np.array_equal(a.pstar(), b.pstar())
    finally:
        a.close(), b.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_previous_mesh_readable(pkg):
    L = pkg.lib()
    s = make("obstacles")
    sol = pkg.Solver(h=s["h"])
    sol.upload(**M.cast(s["sc"], np.float32))
    p = M.device_params(pkg, s)
    good = pkg.Anisotropy(0.9, 4.0, 20 / 3, 0.5, 8)
    nv, nt = C.c_uint64(7), C.c_uint64(7)

    def call(params=p, cfg=(2.0, ISO, good), indexed=0, v=nv, t=nt):
        c = None if cfg is None else pkg.AnisoSurface(*cfg)
        return L.pbf_surface_anisotropic(sol.ctx, None if params is None else C.byref(params), None if c is None else C.byref(c),
                                         indexed, None if v is None else C.byref(v), None if t is None else C.byref(t))

    try:
        assert call() == ERR_STATE                                                # before any step
        for _ in range(s["frames"]):
            sol.step(p)
        stock = sol.surface(p, pkg.McParams())
        assert len(stock["vs"]) > 3000

        def still_readable(m, reader):
            again = reader()
            for k in m:
                assert again[k].tobytes() == m[k].tobytes(), k

        inf, nan = float("inf"), float("nan")
        invalid = [dict(params=None), dict(cfg=None), dict(t=None), dict(indexed=1, v=None)]
        invalid += [dict(cfg=(r, i, good)) for r, i in ((0.0, ISO), (-1.0, ISO), (inf, ISO), (nan, ISO), (2.0, 0.0), (2.0, -0.1),
                                                        (2.0, inf), (2.0, nan))]
        invalid += [dict(cfg=(2.0, ISO, pkg.Anisotropy(*bad, 25))) for bad in
                    ((-0.1, 4, 6, 0.5), (1.1, 4, 6, 0.5), (nan, 4, 6, 0.5), (0.9, 0.99, 6, 0.5), (0.9, inf, 6, 0.5), (0.9, 4, 0, 0.5),
                     (0.9, 4, nan, 0.5), (0.9, 4, 6, 0), (0.9, 4, 6, inf))]
        invalid += [dict(cfg=(60.0, ISO, good)), dict(cfg=(47.0, ISO, good), indexed=1)]     # 1441^3 >= 2^31; 3 * 1129^3 >= 2^32
        bad_dt = pkg.default_params(4, 1000.0)
        bad_dt.dt = 0.0
        invalid.append(dict(params=bad_dt))
        foreign = M.device_params(pkg, s)
        foreign.max_bound[0] = 700.0
        for stage, mesh, reader in (("stock", stock, lambda: sol._read_soup(len(stock["vs"]) // 3)), ("anisotropic", None, None)):
            if stage == "anisotropic":
                mesh = sol.surface_anisotropic(p, 2.0, ISO, indexed=True, **kernel_of("obstacles"))
                assert len(mesh["tris"]) > 1000
                reader = lambda: sol._read_indexed(len(mesh["vs"]), len(mesh["tris"]))   # noqa: E731
            for kw in invalid:
                assert call(**kw) == ERR_INVALID, kw
                still_readable(mesh, reader)
            assert call(params=foreign) == ERR_STATE                              # params of another grid
            still_readable(mesh, reader)
        assert nv.value == 7 and nt.value == 7                                    # (no refusal wrote a count)
        assert call() == 0 and nt.value > 1000                                    # (and the table survived the refusals)
        sol.upload(**M.cast(s["sc"], np.float32))
        assert call() == ERR_STATE                                                # after pbf_upload: the table is stale
        t = pkg.Solver(h=s["h"])
        t.upload(**M.cast(s["sc"], np.float32))
        t.step(p)
        cut = pkg.SlabCut(0, 12, 0, 0)
        assert L.pbf_slab_configure(t.ctx, C.byref(cut), 0, 0) == 0
        c = pkg.AnisoSurface(2.0, ISO, good)
        assert L.pbf_surface_anisotropic(t.ctx, C.byref(p), C.byref(c), 0, None, C.byref(nt)) == ERR_STATE   # slab-configured
        t.close()
        e = pkg.Solver(h=s["h"])
        nt.value = 7
        assert L.pbf_surface_anisotropic(e.ctx, C.byref(p), C.byref(c), 0, None, C.byref(nt)) == 0 and nt.value == 0   # empty
        e.close()
    finally:
        sol.close()


# ---- shim and CLI ------------------------------------------------------------------------------------------------------

def test_shim(pkg):
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_aniso_surface_shim")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr


def test_cli_writes_the_mesh_with_the_returned_counts(pkg, tmp_path):
    common = ["--resident", "--scene", "dam-break", "--particles", "8192", "--solver-iter", "2", "-n", "4", "-w", "2"]
    soup, indexed = tmp_path / "soup", tmp_path / "indexed"
    flag = "--anisotropic-surface=0.4,0.9,4,6.6667,0.5,25"
    r = subprocess.run([BIN, *common, "-o", str(soup), flag], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    n = int(re.search(r"Final Vertex count   : (\d+)", r.stdout).group(1))
    assert n > 3000 and n % 3 == 0
    obj = (soup / "mesh.obj").read_text().split("\n")
    assert sum(1 for l in obj if l.startswith("v ")) == n and sum(1 for l in obj if l.startswith("f ")) == n // 3
    assert "nan" not in (soup / "mesh.obj").read_text().lower()
    r = subprocess.run([BIN, *common, "-o", str(indexed), flag, "--indexed-mesh"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    v, t = (int(x) for x in re.search(r"Indexed mesh         : (\d+) vertices, (\d+) triangles", r.stdout).groups())
    assert t == n // 3 and 0 < v < n                                              # the same triangles, shared vertices
    obj = (indexed / "mesh.obj").read_text().split("\n")
    assert sum(1 for l in obj if l.startswith("v ")) == v and sum(1 for l in obj if l.startswith("f ")) == t
    r = subprocess.run([BIN, *common, "--slabs", "2", "--anisotropic-surface=0.4"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--anisotropic-surface is a single-device feature" in r.stderr
