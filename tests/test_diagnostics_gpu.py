"""pbf_diagnostics on a GPU: the stream part against exact (math.fsum) sums of the downloaded arrays, the density part against
the float64 all-pairs restatement (tests/diagnostics_ref.py), the reduction at the sizes where its shape changes, that the
call observes without changing anything a step does, its refusals, the benchmark flag and the C++ shim.

Bounds.  Sums: |got - fsum| <= (n + 8) 2^-53 sum|term| — worst-case recursive summation of n terms in any order, plus the
<= 4 roundings of a term; the terms themselves are formed in double on both sides.  Extrema and counts: exact.  max_speed:
2 ulp of the double root.  rho: the bars tests/test_surface_tension_gpu.py already holds the same sum to (1e-12 in fp64,
3e-5 in fp32, of rho.max()), C the same scaled by 1 / rho0.  Neighbour counts: between the reference at thresholds
h (1 - delta) and h (1 + delta), delta = 16 eps_N — tests/test_diagnostics_cpu.py shows that at most 0.1 % of the particles
have a pair in that window."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import diagnostics_ref as DR
import nversion as NV
from test_cli_gpu import BIN
from test_nversion_cpu import scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 0.1
VARIANTS = [(True, False), (False, False), (False, True)]   # (fp64, PBF_FLAG_FAST_MATH)
IDS = ["fp64", "fp32", "fp32-fast"]
SCENES = ["cubes1024", "cloud", "obstacles"]
ERR_INVALID, ERR_STATE = -1, -4
U = 2.0 ** -53
SUMS = ["mass", "moment", "momentum", "kinetic"]
DENSITY_FLOATS = ["rho_min", "rho_max", "rho_mean", "err_mean", "err_max", "compression_mean", "nbr_mean"]


def solver(pkg, sc, fp64, fast=False, **options):
    s = pkg.Solver(h=H, fp64=fp64, flags=pkg.FLAG_FAST_MATH if fast else 0)
    for k, v in options.items():
        s.set_option(k, v)
    return s.upload(**sc)


def as_dtype(sc, fp64):
    dt = np.float64 if fp64 else np.float32
    return {k: (v.astype(dt) if v.dtype.kind == "f" else v) for k, v in sc.items()}


def raw(d):
    return bytes(memoryview(d))


def check_stream(got, down):
    """got: Solver.diagnostics() dict; down: Solver.download() of the same state"""
    ref = DR.stream(down)
    n = ref["n_fluid"]
    for k in ("n_fluid", "n_obstacle", "n_nonfinite"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert got["n_fluid"] + got["n_obstacle"] + got["n_nonfinite"] == len(down["id"])
    for k in SUMS:
        err, bound = np.abs(got[k] - ref[k]), (n + 8) * U * ref["abs_" + k]
        print(k, "error", np.max(err), "bound", np.max(bound))
        assert np.all(err <= bound), (k, got[k], ref[k], bound)
    assert np.array_equal(got["aabb_min"], ref["aabb_min"]) and np.array_equal(got["aabb_max"], ref["aabb_max"])
    root = np.sqrt(ref["max_speed2"])
    assert abs(got["max_speed"] - root) <= 2 * np.spacing(root), (got["max_speed"], root)
    return ref


# ---- stream part ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", SCENES)
def test_stream_part_after_upload_and_after_steps(pkg, name, fp64, fast):
    s = solver(pkg, scene(name), fp64, fast)
    d0 = s.diagnostics()                       # straight after the upload, no params
    check_stream(d0, s.download())
    assert d0["n_density"] == 0 and d0["nbr_max"] == 0 and not any(d0[k] for k in DENSITY_FLOATS)
    p = pkg.default_params(2, 1000.0)
    s.steps(p, 3)
    ref = check_stream(s.diagnostics(p), s.download())
    assert ref["kinetic"] > 0


@pytest.mark.parametrize("fp64", [True, False], ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 262144 + 77])
def test_reduction_sizes(pkg, n, fp64):
    """one lane, a wave +- 1, a workgroup's round +- 1, a workgroup's tile +- 1, and more partial records (257) than the
    second launch has lanes"""
    s = solver(pkg, DR.lattice(n, fp64=fp64), fp64)
    d = s.diagnostics()
    check_stream(d, s.download())
    assert d["n_fluid"] == n
    assert raw(s.diagnostics(raw=True)) == raw(s.diagnostics(raw=True))


@pytest.mark.parametrize("fp64", [True, False], ids=["fp64", "fp32"])
def test_obstacles_only_and_nonfinite(pkg, fp64):
    sc = DR.lattice(700, fp64=fp64)
    walls = dict(sc, type=np.ones(700, np.uint8))
    d = solver(pkg, walls, fp64).diagnostics()
    assert d["n_fluid"] == 0 and d["n_obstacle"] == 700 and d["n_nonfinite"] == 0
    for k, v in d.items():
        if k not in ("n_fluid", "n_obstacle", "n_nonfinite"):
            assert not np.any(v), (k, v)
    sc["type"][::9] = 1
    sc["vel"][301, 1] = np.inf
    sc["pos"][302, 2] = np.nan
    sc["pos"][306] = np.nan                    # (an obstacle: its values are never looked at)
    assert sc["type"][306] == 1 and sc["type"][301] == 0 and sc["type"][302] == 0
    s = solver(pkg, sc, fp64)
    d = s.diagnostics()
    check_stream(d, s.download())
    assert d["n_nonfinite"] == 2 and np.isfinite(d["kinetic"]) and np.isfinite(d["aabb_max"]).all()


# ---- density part -----------------------------------------------------------------------------------------------------

def stepped(pkg, name, fp64, fast, p, **options):
    s = solver(pkg, scene(name), fp64, fast, **options)
    if name == "cubes1024":
        s.steps(p, 3)                          # leave the lattice first (as test_physics_gpu does)
    return s


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", SCENES)
def test_density_part_equals_all_pairs_restatement(pkg, name, fp64, fast):
    p = pkg.default_params(2, 1000.0)
    s, cut = stepped(pkg, name, fp64, fast, p), stepped(pkg, name, fp64, fast, p)
    s.step(p)
    # the neighbour set is fixed at predict time: the cells from a second run stopped after this step's sort
    cut.stage("predict", p).stage("sort", p)
    b = s.download()
    assert np.array_equal(cut.download()["id"], b["id"])
    cells = NV.predict_cells(cut.pstar()[:, :3].astype(np.float64), H, p.scale, list(p.min_bound))
    d = s.diagnostics(p, density=True, raw=True)
    got, rho_gpu = d.as_dict(), s.density().astype(np.float64)
    check_stream(got, b)
    ps = s.pstar()[:, :3].astype(np.float64)
    mass, obstacle = b["mass"].astype(np.float64), b["type"] == 1
    delta = 16 * float(np.finfo(np.float64 if fp64 else np.float32).eps)
    rho, lo, hi = DR.density(ps, mass, H, obstacle, cells, delta)
    tol = (1e-12 if fp64 else 3e-5) * rho.max()
    print("rho error", np.abs(rho_gpu - rho).max(), "bar", tol, "pairs in the window", int((hi - lo).sum()))
    assert np.abs(rho_gpu - rho).max() <= tol
    assert not rho_gpu[obstacle].any()
    ref = DR.density_fields(rho, lo, obstacle)
    assert got["n_density"] == ref["n_density"] == int((~obstacle).sum())
    for k in ("rho_min", "rho_max", "rho_mean"):
        assert abs(got[k] - ref[k]) <= tol, (k, got[k], ref[k])
    for k in ("err_mean", "err_max", "compression_mean"):
        assert abs(got[k] - ref[k]) <= tol / DR.RHO0, (k, got[k], ref[k])
    f = ~obstacle
    assert lo[f].max() <= got["nbr_max"] <= hi[f].max()
    assert lo[f].mean() - 1e-12 <= got["nbr_mean"] <= hi[f].mean() + 1e-12
    # the record's own arithmetic: the fields are the device's per-particle values, reduced
    assert got["rho_min"] == rho_gpu[f].min() and got["rho_max"] == rho_gpu[f].max()
    assert abs(got["rho_mean"] - DR.fsum(rho_gpu[f]) / f.sum()) <= (f.sum() + 8) * U * got["rho_mean"]
    # every gather kernel: the same bits
    for kind in (0, 1):
        s.set_option("gather", kind)
        again = s.diagnostics(p, density=True, raw=True)
        assert raw(again) == raw(d), kind
        assert np.array_equal(s.density().astype(np.float64), rho_gpu), kind


# ---- observer ---------------------------------------------------------------------------------------------------------

def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("fp64", [True, False], ids=["fp64", "fp32"])
def test_a_call_between_steps_changes_nothing(pkg, fp64, graph):
    p = pkg.default_params(2, 1000.0)
    plain, watched, batch = (solver(pkg, scene("cubes1024"), fp64, graph=graph) for _ in range(3))
    for _ in range(6):
        plain.steps(p, 1)
        watched.steps(p, 1)
        d = watched.diagnostics(p, density=True, raw=True)
        assert raw(watched.diagnostics(p, density=True, raw=True)) == raw(d)      # two calls, identical bytes
    batch.steps(p, 6)
    one = batch.diagnostics(p, density=True, raw=True)
    a = plain.download()
    assert same_bits(a, watched.download()) and same_bits(a, batch.download())
    assert plain.graph_stats() == watched.graph_stats()
    print("graph stats", plain.graph_stats())
    if graph:
        assert plain.graph_stats()[0] > 0, "the graph path was not exercised"
    assert raw(one) == raw(d)                  # the same state, however it was reached and however often it was asked


@pytest.mark.parametrize("fp64", [True, False], ids=["fp64", "fp32"])
def test_extras_records_survive_the_call(pkg, fp64):
    p = pkg.default_params(2, 1000.0)
    p.vorticity = 1
    plain, watched = (solver(pkg, scene("obstacles"), fp64).set_surface_tension(0.05, 0.5) for _ in range(2))
    for _ in range(3):
        plain.step(p)
        watched.step(p)
        w, st, ps = watched.omega(), watched.surface_state(), watched.pstar()
        watched.diagnostics(p, density=True)
        assert np.array_equal(watched.omega(), w) and np.array_equal(watched.surface_state(), st)
        assert np.array_equal(watched.pstar(), ps)
        # the surface pass's own density is the sum with the NEIGHBOUR's mass; with equal masses the two would agree
        assert watched.density().shape == (watched.n,)
    assert same_bits(plain.download(), watched.download())
    assert np.array_equal(plain.omega(), watched.omega()) and np.array_equal(plain.surface_state(), watched.surface_state())


# ---- refusals ---------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_record_untouched(pkg):
    from pbf_sph_amd import capi
    L = pkg.lib()
    p = pkg.default_params(2, 1000.0)
    s = solver(pkg, scene("cubes1024"), False)
    d = capi.Diag()
    C.memset(C.byref(d), 0xAB, C.sizeof(d))
    before = raw(d)

    def refused(rc, code, *args):
        assert L.pbf_diagnostics(*args) == code, (rc, args)
        assert raw(d) == before, rc

    refused("density before any step", ERR_STATE, s.ctx, C.byref(p), capi.DIAG_DENSITY, C.byref(d))
    with pytest.raises(pkg.PbfError):
        s.density()
    refused("unknown flag", ERR_INVALID, s.ctx, C.byref(p), 2, C.byref(d))
    refused("unknown flag beside a known one", ERR_INVALID, s.ctx, C.byref(p), 1 | 1 << 31, C.byref(d))
    assert L.pbf_diagnostics(s.ctx, C.byref(p), 0, None) == ERR_INVALID
    refused("density without params", ERR_INVALID, s.ctx, None, capi.DIAG_DENSITY, C.byref(d))
    s.step(p)
    q = pkg.default_params(2, 1000.0)
    q.max_bound[0] = 1400.0
    refused("density with foreign bounds", ERR_STATE, s.ctx, C.byref(q), capi.DIAG_DENSITY, C.byref(d))
    assert b"differ" in L.pbf_last_error(s.ctx)
    assert s.diagnostics(p, density=True)["n_density"] == 1024        # the refusal left the grid alone
    assert s.density().shape == (1024,)
    s.step(p)
    with pytest.raises(pkg.PbfError):
        s.density()                                                   # the arrays have changed since
    s.diagnostics(p, density=True)
    s.upload(**as_dtype(scene("cubes1024"), False))
    refused("density after an upload that follows a step", ERR_STATE, s.ctx, C.byref(p), capi.DIAG_DENSITY, C.byref(d))
    with pytest.raises(pkg.PbfError):
        s.density()
    assert s.diagnostics()["n_fluid"] == 1024                         # the stream part is valid whenever download is
    cut = capi.SlabCut(0, 12, 0, 0)
    assert L.pbf_slab_configure(s.ctx, C.byref(cut), 0, 0) == 0
    refused("slab mode, stream part", ERR_STATE, s.ctx, None, 0, C.byref(d))
    refused("slab mode, density part", ERR_STATE, s.ctx, C.byref(p), capi.DIAG_DENSITY, C.byref(d))
    assert b"slab" in L.pbf_last_error(s.ctx)


def test_records_go_stale_on_a_replayed_step(pkg):
    """What the density pass and a whitewater step leave for pbf_read_buffer describes one sorted order.  A step replayed
    from a captured graph launches its sort without running the host code of the sort stage: the records must go stale
    there as well.  At least one of the single steps below has to be a replay, or the test has not reached that path."""
    p = pkg.default_params(4, 1000.0)
    s = solver(pkg, pkg.scene_cubes(2048, False), False, graph=1)
    s.whitewater_configure(capacity=4096, k_ta=50.0, k_wc=50.0, tau_ta=(0.0, 0.5), tau_wc=(0.0, 0.5), tau_k=(0.0, 0.01))
    for _ in range(4):
        s.steps(p, 4)
    rho, pot = np.empty(s.n, np.float32), np.empty((s.n, 4), np.float32)

    def read():
        return (s.L.pbf_read_buffer(s.ctx, pkg.BUF_DENSITY, rho.ctypes.data_as(C.c_void_p), rho.nbytes),
                s.L.pbf_read_buffer(s.ctx, pkg.BUF_WHITEWATER, pot.ctypes.data_as(C.c_void_p), pot.nbytes))

    replays = 0
    for _ in range(4):
        s.diagnostics(p, density=True)
        s.whitewater_step(p)
        assert read() == (0, 0)
        before = s.graph_stats()
        s.steps(p, 1)
        after = s.graph_stats()
        print("graph stats", before, "->", after)
        assert read() == (ERR_STATE, ERR_STATE)
        replays += after[1] == before[1] + 1
    assert replays >= 1, "no single step was a replay: restore() was not reached"


def touch_every_owner(pkg):
    """One context that makes every lazily allocated owner allocate — the drain's, the diagnostics' and the whitewater
    step's pinned records, the pinned mesh staging (mapped as a soup and as an indexed mesh), the observers' scratch — and
    is then destroyed -> everything it handed out, as bytes."""
    p = pkg.default_params(2, 1000.0)
    sc = pkg.scene_cubes(2048, False)
    s = solver(pkg, sc, False)
    s.set_drains([(sc["pos"][7], 60.0)])
    s.whitewater_configure(capacity=4096, k_ta=50.0, k_wc=50.0, tau_ta=(0.0, 0.5), tau_wc=(0.0, 0.5), tau_k=(0.0, 0.01))
    s.steps(p, 2)
    assert s.scene_host_syncs() == 2 and s.n > 0
    out = {"diag": raw(s.diagnostics(p, density=True, raw=True)), "rho": s.density().tobytes()}
    out["ww"] = repr(s.whitewater_step(p))
    out.update(("ww_" + k, v.tobytes()) for k, v in s.whitewater_download().items())
    out["pot"] = s.whitewater_potentials().tobytes()
    for indexed in (False, True):
        mesh = s.surface_indexed(p) if indexed else s.surface(p)
        sizes = [a.nbytes for a in (mesh["vs"], mesh["ns"], mesh["cs"])] + ([mesh["tris"].nbytes] if indexed else [])
        assert min(sizes) > 0
        at = [C.c_void_p() for _ in sizes]
        fn = s.L.pbf_map_mesh_indexed if indexed else s.L.pbf_map_mesh
        assert fn(s.ctx, *[C.byref(a) for a in at]) == 0
        for k, (a, n) in enumerate(zip(at, sizes)):
            out["map%d_%d" % (indexed, k)] = C.string_at(a.value, n)
        assert [out["map%d_%d" % (indexed, k)] for k in range(3)] == [mesh[k].tobytes() for k in ("vs", "ns", "cs")]
    pts = sc["pos"][::97].astype(np.float64)
    out["query"] = b"".join(ids.tobytes() for ids in s.query(p, pts))
    out.update(("sample_" + k, v.tobytes()) for k, v in s.sample(p, pts, velocity=True, colour=True).items())
    out.update(("aniso_" + k, np.ascontiguousarray(v).tobytes()) for k, v in s.anisotropy(p).items())
    s.step(p)
    out.update(("down_" + k, v.tobytes()) for k, v in s.download().items())
    s.close()
    return out


def test_a_second_context_after_a_destroyed_one(pkg):
    """every owner allocated, the context destroyed, and the same again in the same process: the same bytes"""
    first, second = touch_every_owner(pkg), touch_every_owner(pkg)
    print("bytes compared", {k: len(v) for k, v in first.items()})
    assert first.keys() == second.keys()
    assert [k for k in first if first[k] != second[k]] == []


# ---- CLI and shim -----------------------------------------------------------------------------------------------------

def test_benchmark_flag(pkg, tmp_path):
    r = subprocess.run([BIN, "--resident", "--diagnostics=2", "-n", "6", "--particles", "4096", "-w", "2", "-o", str(tmp_path / "out"),
                        "--json"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.split("\n") if l.startswith('{"frame"')]
    assert [l["frame"] for l in lines] == [1, 3, 5]
    n = len(pkg.scene_cubes(4096)["id"])
    for l in lines:
        assert l["diag"]["n_fluid"] == n and l["diag"]["kinetic"] > 0 and l["diag"]["n_density"] == n
        assert l["diag"]["rho_max"] >= l["diag"]["rho_mean"] > 0 and l["diag"]["nbr_mean"] > 0
    summary = [json.loads(l) for l in r.stdout.split("\n") if l.startswith('{"impl"')]
    assert len(summary) == 1 and summary[0]["frames"] == 6


def test_shim(pkg):
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_diag_shim")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
