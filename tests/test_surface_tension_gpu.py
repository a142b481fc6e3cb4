"""GPU checks of the opt-in surface tension and adhesion (Akinci et al. 2013; pbf_set_surface_tension): off costs
nothing and changes no bit; the three passes against the float64 all-pairs restatement (tests/surface_tension_ref.py);
a two-particle closed form; momentum conservation and adhesion; that cohesion rounds an elongated block; hipGraph replay
with the coefficients toggled; determinism; the benchmark flag.  Small scenes only.

Calibration.  The test scenes sit at rest spacing 27 world units = 0.054 solver units (scale 500); with h = 0.1 nearest
neighbours sit just beyond h/2, where C peaks at ~160 (32 / (pi h^9) (h - r)^3 r^3).  One neighbour then changes a
velocity by dt K gamma m C ~ 0.0125 * 1 * gamma * 160 = 2 gamma per step (solver units / time; K = 2 rho0 / (rho_i + rho_j)
~ 1 in the bulk, up to ~3 at a sparse surface), while finalise damps velocities by VD = 0.49 every step.  GAMMA = 0.05
changes a surface velocity by ~0.1 per step: large against fp32 rounding of the velocities it is added to (the stage
checks subtract two runs) and far below anything that makes a step unstable.
"""
import os
import subprocess

import numpy as np
import pytest

import nversion as NV
import surface_tension_ref as ST
from test_cli_gpu import BIN, read_ply
from test_nversion_cpu import scene

pytestmark = pytest.mark.gpu

H = 0.1
GAMMA = 0.05
BETA = 0.5
VARIANTS = [(True, False), (False, False), (False, True)]   # (fp64, PBF_FLAG_FAST_MATH): fp64, fp32, fp32 fast math
IDS = ["fp64", "fp32", "fp32-fast"]


def tol(fp64):
    return 1e-12 if fp64 else 2e-4


def solver(pkg, sc, fp64, flags=0):
    return pkg.Solver(h=H, fp64=fp64, flags=flags).upload(**sc)


def zero_g(pkg, iteration):
    p = pkg.default_params(iteration, 1000.0)
    p.constant_force[0] = p.constant_force[1] = p.constant_force[2] = 0.0
    return p


def block(nx, ny, nz, spacing=27.0, centre=(500.0, 500.0, 500.0), fp64=True, type_=0):
    dt = np.float64 if fp64 else np.float32
    ax = [(np.arange(k) - (k - 1) / 2.0) * spacing for k in (nx, ny, nz)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3) + np.asarray(centre)
    n = len(g)
    return dict(id=np.arange(n, dtype=np.uint64), type=np.full(n, type_, np.uint8), mass=np.ones(n, dt),
                pos=g.astype(dt), vel=np.zeros((n, 3), dt), colour=np.full((n, 4), 0.5, dt))


def concat(a, b):
    out = {k: np.concatenate([a[k], b[k]]) for k in a}
    out["id"] = np.arange(len(out["id"]), dtype=np.uint64)
    return out


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("fp64", [True, False])
def test_off_is_free(pkg, fp64, graph):
    sc = scene("cubes1024")
    p = pkg.default_params(2, 1000.0)
    out = []
    for mode in range(3):
        s = solver(pkg, sc, fp64)
        s.set_option("graph", graph)
        if mode == 1:
            s.set_surface_tension(0.0, 0.0)
        elif mode == 2:
            s.set_surface_tension(GAMMA, BETA).set_surface_tension(0.0)
        s.steps(p, 10)
        out.append(s.download())
        with pytest.raises(pkg.PbfError):
            s.surface_state()                                # never ran: no record
    assert same_bits(out[0], out[1]) and same_bits(out[0], out[2])


def test_invalid_coefficients_are_refused(pkg):
    s = solver(pkg, scene("cubes1024"), False)
    for bad in [(-1.0, 0.0), (0.0, -0.5), (float("nan"), 0.0), (0.0, float("inf"))]:
        with pytest.raises(pkg.PbfError):
            s.set_surface_tension(*bad)


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", ["cubes1024", "cloud", "obstacles"])
def test_passes_equal_all_pairs_restatement(pkg, name, fp64, fast):
    flags = pkg.FLAG_FAST_MATH if fast else 0
    sc = scene(name)
    p = pkg.default_params(2, 1000.0)
    warm = 3 if name == "cubes1024" else 0             # leave the lattice first (as test_physics_gpu does)
    beta = BETA if name == "obstacles" else 0.0
    off, on, cut = (solver(pkg, sc, fp64, flags) for _ in range(3))
    for s in (off, on, cut):
        if warm:
            s.steps(p, warm)
    on.set_surface_tension(GAMMA, beta)
    off.step(p)
    on.step(p)
    a, b = off.download(), on.download()
    assert np.array_equal(a["id"], b["id"]) and np.array_equal(a["pos"], b["pos"])   # the pass runs after the solve
    assert not np.array_equal(a["vel"], b["vel"])
    # the neighbour set is fixed at predict time: the cells from a third run stopped after this step's sort
    cut.stage("predict", p).stage("sort", p)
    assert np.array_equal(cut.download()["id"], b["id"])
    cells = NV.predict_cells(cut.pstar()[:, :3].astype(np.float64), H, p.scale, list(p.min_bound))
    ps = on.pstar()[:, :3].astype(np.float64)
    mass, obstacle = b["mass"].astype(np.float64), b["type"] == 1
    dv, rho, nrm = ST.delta_v(ps, mass, H, p.dt, GAMMA, beta, obstacle, cells)
    st = on.surface_state().astype(np.float64)
    t = tol(fp64)
    assert np.abs(st[:, 3] - rho).max() <= (1e-12 if fp64 else 3e-5) * rho.max()
    assert np.abs(st[:, :3] - nrm).max() <= t * np.abs(nrm).max()
    got = b["vel"].astype(np.float64) - a["vel"].astype(np.float64)
    assert np.abs(got - dv).max() <= t * np.abs(dv).max()
    if name == "obstacles":
        assert np.array_equal(a["vel"][obstacle], b["vel"][obstacle])


@pytest.mark.parametrize("fp64", [True, False])
def test_two_particles_closed_form(pkg, fp64):
    """Zero gravity, at rest, no solver iterations: the positions stay put and the velocity change is the pass alone.
    Attraction for h/2 < r <= h; repulsion where the cohesion spline is negative (r below ~0.27 h)."""
    p = zero_g(pkg, 0)
    for r, attract in [(0.02, False), (0.06, True), (0.075, True), (0.09, True)]:
        sc = block(2, 1, 1, spacing=r * 500.0, fp64=fp64)
        off, on = solver(pkg, sc, fp64), solver(pkg, sc, fp64).set_surface_tension(GAMMA)
        off.step(p)
        on.step(p)
        a, b = off.download(), on.download()
        ps = on.pstar()[:, :3].astype(np.float64)
        d = ps[1] - ps[0]
        rr = float(np.sqrt(d @ d))
        u = d / rr                                            # particle 0 -> particle 1
        dv0 = b["vel"][0].astype(np.float64) - a["vel"][0].astype(np.float64)
        dv1 = b["vel"][1].astype(np.float64) - a["vel"][1].astype(np.float64)
        want = ST.two_particle_dv(rr, H, 1.0, float(p.dt), GAMMA)
        assert (dv0 @ u > 0) == attract and (dv1 @ -u > 0) == attract, (r, dv0, dv1)
        rt = 1e-12 if fp64 else 2e-5
        assert abs(dv0 @ u - want) <= rt * abs(want) and abs(dv1 @ -u - want) <= rt * abs(want), (r, dv0 @ u, want)
        assert np.abs(dv0 - (dv0 @ u) * u).max() <= rt * abs(want)


@pytest.mark.parametrize("fp64", [True, False])
def test_momentum_and_adhesion(pkg, fp64):
    p = zero_g(pkg, 2)
    # a fluid-only blob of equal masses: every pair term is antisymmetric
    sc = block(8, 8, 8, spacing=24.0, fp64=fp64)
    off, on = solver(pkg, sc, fp64), solver(pkg, sc, fp64).set_surface_tension(GAMMA)
    off.step(p)
    on.step(p)
    a, b = off.download(), on.download()
    assert np.array_equal(a["pos"], b["pos"])
    m = b["mass"].astype(np.float64)[:, None]
    mdv = m * (b["vel"].astype(np.float64) - a["vel"].astype(np.float64))
    assert np.abs(mdv).max() > 0
    assert np.abs(mdv.sum(0)).max() <= (1e-12 if fp64 else 1e-6) * np.abs(mdv).sum()
    # adhesion only (gamma = 0): a fluid block beside a wall of obstacle particles at lower x
    wall = block(1, 10, 10, spacing=27.0, centre=(400.0, 500.0, 500.0), fp64=fp64, type_=1)
    fl = block(4, 6, 6, spacing=27.0, centre=(400.0 + 35.0 + 1.5 * 27.0, 500.0, 500.0), fp64=fp64)
    sc = concat(wall, fl)
    off, on = solver(pkg, sc, fp64), solver(pkg, sc, fp64).set_surface_tension(0.0, BETA)
    off.step(p)
    on.step(p)
    a, b = off.download(), on.download()
    assert np.array_equal(a["id"], b["id"]) and np.array_equal(a["pos"], b["pos"])
    obst = b["type"] == 1
    assert np.array_equal(a["vel"][obst], b["vel"][obst])      # obstacles: copied through bit for bit
    ps = on.pstar()[:, :3].astype(np.float64)
    r = np.sqrt(((ps[~obst][:, None, :] - ps[obst][None, :, :]) ** 2).sum(-1))
    pulled = ((r > H / 2) & (r < H)).any(1)
    dvx = (b["vel"][~obst, 0].astype(np.float64) - a["vel"][~obst, 0].astype(np.float64))
    assert pulled.sum() >= 36
    assert (dvx[pulled] < 0).all()                               # towards the wall
    assert (dvx[~(r <= H).any(1)] == 0).all()                    # no obstacle within h: nothing


def principal_ratio(pos):
    x = pos.astype(np.float64)
    ev = np.linalg.eigvalsh(np.cov((x - x.mean(0)).T))
    return float(np.sqrt(ev.max() / ev.min()))


@pytest.mark.parametrize("fp64", [True, False])
def test_cohesion_rounds_an_elongated_block(pkg, fp64):
    """Zero gravity, far from the walls: after STEPS steps the block's largest / smallest principal radius of gyration
    must be clearly smaller with cohesion than without (both start at ~4), and everything stays finite."""
    # measured on the MI355X (40 steps, ratio from ~4.05): gamma 0 -> 3.88, 0.05 -> 3.83, 0.2 -> 2.2-2.4, 0.5 -> 1.05-1.12,
    # 1.0 -> ~1.03 and still finite.  0.2 sits in the middle of the response: a clear margin, no saturation
    STEPS, G = 40, 0.2
    p = zero_g(pkg, 2)
    sc = block(24, 6, 6, fp64=fp64)
    base = principal_ratio(sc["pos"])
    off, on = solver(pkg, sc, fp64), solver(pkg, sc, fp64).set_surface_tension(G)
    off.steps(p, STEPS)
    on.steps(p, STEPS)
    a, b = off.download(), on.download()
    assert np.isfinite(b["pos"]).all() and np.isfinite(b["vel"]).all()
    ra, rb = principal_ratio(a["pos"]), principal_ratio(b["pos"])
    print(f"principal-radius ratio: start {base:.3f}, gamma 0 {ra:.3f}, gamma {G} {rb:.3f}")
    assert rb <= ra - 0.1 * (base - 1.0), (base, ra, rb)


@pytest.mark.parametrize("fp64", [True, False])
def test_graph_replay_with_toggled_coefficients(pkg, fp64):
    sc = scene("cubes1024")
    p = pkg.default_params(2, 1000.0)
    settings = [(GAMMA, 0.0), (0.0, 0.0), (GAMMA, 0.0), (0.0, 0.0), (2 * GAMMA, 0.0), (0.0, 0.0)] * 2
    eager, graphed, still = solver(pkg, sc, fp64), solver(pkg, sc, fp64), solver(pkg, sc, fp64)
    graphed.set_option("graph", 1)
    still.set_option("graph", 1)
    for g, bt in settings:
        eager.set_surface_tension(g, bt).steps(p, 4)
        graphed.set_surface_tension(g, bt).steps(p, 4)
        still.steps(p, 4)
    assert same_bits(eager.download(), graphed.download())
    captured, replays, enabled = graphed.graph_stats()
    base_captured = still.graph_stats()[0]
    assert enabled and replays > 0 and captured > base_captured, (captured, replays, base_captured)


def test_surface_state_is_refused_after_a_new_upload(pkg):
    """The record of the last surface-tension pass describes the particle set it ran on: after an upload reading it is
    PBF_ERR_STATE (-4) until a step has run the pass again."""
    sc = scene("cubes1024")
    p = pkg.default_params(2, 1000.0)
    s = solver(pkg, sc, False).set_surface_tension(GAMMA, BETA).step(p)
    assert s.surface_state().shape == (len(sc["id"]), 4)
    s.upload(**sc)
    with pytest.raises(pkg.PbfError, match=r"\(-4\)"):
        s.surface_state()
    assert np.isfinite(s.step(p).surface_state()).all()


@pytest.mark.parametrize("fp64", [True, False])
def test_deterministic(pkg, fp64):
    sc = scene("obstacles")
    p = pkg.default_params(2, 1000.0)
    runs = []
    for _ in range(2):
        s = solver(pkg, sc, fp64).set_surface_tension(GAMMA, BETA)
        s.steps(p, 20)
        runs.append((s.download(), s.surface_state()))
    assert same_bits(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert np.isfinite(runs[0][0]["vel"]).all()


def test_cli_flag(pkg, tmp_path):
    common = ["--scene", "cubes", "--particles", "8000", "-n", "5", "-w", "0", "--resident", "--no-surface"]
    clouds = []
    for extra, d in [([], "off"), ([f"--surface-tension={GAMMA},{BETA}"], "on")]:
        r = subprocess.run([BIN, *common, *extra, "-o", str(tmp_path / d)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        clouds.append(read_ply(os.path.join(str(tmp_path), d, "cloud.ply")))
    assert clouds[0].shape == clouds[1].shape and np.isfinite(clouds[1]).all()
    assert not np.array_equal(clouds[0], clouds[1])
    r = subprocess.run([BIN, *common, f"--surface-tension={GAMMA}", "--slabs", "2", "-o", str(tmp_path / "slab")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "single-device" in r.stderr


def test_aos_upload_with_surface_tension(pkg):
    """pbf_upload_aos (the C++ advance() path) treats the feature like pbf_upload: the fields grow with the particle
    capacity at the upload, the last record is dropped (it described other particles), and the steps that follow equal
    those after a SoA upload."""
    import ctypes as C
    from pbf_sph_amd import capi

    dt = np.dtype([("id", "<u8"), ("type", "u1"), ("_pad", "u1", 3), ("mass", "<f4"), ("pos", "<f4", 3),
                   ("vel", "<f4", 3), ("colour", "<f4", 4)])
    lay = capi.AosLayout(56, 0, 8, 12, 16, 28, 40)

    def aos(sc):
        a = np.zeros(len(sc["id"]), dt)
        for k in ("id", "type", "mass", "pos", "vel", "colour"):
            a[k] = sc[k]
        return a

    p = pkg.default_params(2, 1000.0)
    small, big = block(4, 4, 4, fp64=False), scene("obstacles")
    big = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in big.items()}
    s = pkg.Solver(h=H).set_surface_tension(GAMMA, BETA)
    a = aos(small)
    assert s.L.pbf_upload_aos(s.ctx, len(a), a.ctypes.data_as(C.c_void_p), C.byref(lay)) == 0
    s.steps(p, 4)
    assert s.surface_state().shape == (len(a), 4)
    b = aos(big)                                                 # more particles than the fields were sized for
    assert s.L.pbf_upload_aos(s.ctx, len(b), b.ctypes.data_as(C.c_void_p), C.byref(lay)) == 0
    with pytest.raises(pkg.PbfError):
        s.surface_state()                                        # the last record described other particles
    s.steps(p, 6)
    ref = solver(pkg, big, False).set_surface_tension(GAMMA, BETA)
    ref.steps(p, 6)
    assert same_bits(s.download(), ref.download())
    assert np.array_equal(s.surface_state(), ref.surface_state())
