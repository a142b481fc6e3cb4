"""pbf_whitewater_* on a GPU: the potentials against the float64 all-pairs restatement (tests/whitewater_ref.py, which
derives the bars), the child counts and their slots recomputed from the device's own n_d and the hash, the emission geometry,
the advection bit for bit against numpy in N on pbf_sample_points' answers, the capacity, determinism across contexts and
gather kernels, that a fluid step never notices, and the refusals.

Scenes: cubes2048 after 5 steps (K = 4), dam8192 after 30 steps (K = 2), and cubes2048 with every fifth particle an obstacle
and unequal masses after 3 steps (K = 2).  The tau ranges of a run are the 10 % and 90 % quantiles of the scene's own
potentials, read back from a first whitewater step with rates 0 — how tools and users are meant to pick them.

The one PBF_FLAG_FAST_MATH case of the potentials test adds 3e-5 of the column maximum to the bars.  That figure is NOT
derived for these potentials (v_rsq and fma have no rounding count, and I_ta divides by |v_ij| r): it is inherited from the
bar tests/test_sample_gpu.py and tests/test_diagnostics_gpu.py give the density sums under that flag."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import whitewater_ref as WR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H = 0.1
ERR_INVALID, ERR_STATE = -1, -4
VARIANTS = [(True, False), (False, False)]
IDS = ["fp64", "fp32"]
SCENES = {"cubes2048": (4, 5, 1000.0), "dam8192": (2, 30, 1100.0), "obstacles2048": (2, 3, 1000.0)}
AMBIGUOUS_CAP = 0.02


def make_scene(pkg, name, fp64):
    if name == "dam8192":
        return pkg.scene_dambreak(8192, fp64)[0]
    sc = {k: v.copy() for k, v in pkg.scene_cubes(2048, fp64).items()}
    if name == "obstacles2048":
        sc["type"][::5] = 1
        sc["mass"] = (0.5 + np.random.default_rng(17).random(len(sc["id"]))).astype(sc["mass"].dtype)
    return sc


def stepped(pkg, name, fp64, fast=False, **options):
    K, steps, side = SCENES[name]
    s = pkg.Solver(h=H, fp64=fp64, flags=pkg.FLAG_FAST_MATH if fast else 0)
    for k, v in options.items():
        s.set_option(k, v)
    p = pkg.default_params(K, side)
    s.upload(**make_scene(pkg, name, fp64)).steps(p, steps)
    return s, p


def quantile_taus(pot):
    """tau ranges from the potentials of a first step: the 10 % and 90 % quantiles of the positive values"""
    out = []
    for col in range(3):
        v = pot[:, col].astype(np.float64)
        v = v[v > 0]
        lo, hi = (np.quantile(v, 0.1), np.quantile(v, 0.9)) if len(v) else (0.0, 1.0)
        out.append((float(lo), float(hi) if hi > lo else float(lo) + 1.0))
    return dict(tau_ta=out[0], tau_wc=out[1], tau_k=out[2])


def configured(s, p, capacity, k_ta, k_wc, seed=11, **more):
    """probe the potentials with rates 0, then configure with the scene's quantile ranges -> cfg dict"""
    s.whitewater_configure(capacity=max(capacity, 1), tau_ta=(0, 1), tau_wc=(0, 1), tau_k=(0, 1))
    s.whitewater_step(p)
    cfg = dict(capacity=capacity, k_ta=k_ta, k_wc=k_wc, seed=seed, lifetime=(2.0, 5.0), k_b=2.0, k_d=0.8, spray_below=6,
               bubble_from=20, **quantile_taus(s.whitewater_potentials()))
    cfg.update(more)
    s.whitewater_configure(**cfg)
    return cfg


def read_state(s):
    return dict(down=s.download(), pstar=s.pstar(), keys=s.keys(), table_size=len(s.table()))


def pool_bytes(s):
    d = s.whitewater_download()
    return b"".join(np.ascontiguousarray(d[k]).tobytes() for k in ("pos", "vel", "life", "kind", "parent_id"))


# ---- 1. potentials ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,fp64,fast", [(n, f, False) for n in SCENES for f, _ in VARIANTS] + [("cubes2048", False, True)],
                         ids=[f"{n}-{i}" for n in SCENES for i in IDS] + ["cubes2048-fp32-fast"])
def test_potentials_against_the_all_pairs_reference(pkg, name, fp64, fast):
    s, p = stepped(pkg, name, fp64, fast)
    dt = np.float64 if fp64 else np.float32
    cfg = configured(s, p, 4096, k_ta=40.0, k_wc=40.0)
    s.whitewater_step(p)
    pot = s.whitewater_potentials().astype(np.float64)
    st = read_state(s)
    ref = WR.potentials(st["down"], st["pstar"], st["keys"], st["table_size"], float(dt(H)), cfg, p.dt, 0, dt)
    fluid = st["down"]["type"] == 0
    assert not pot[~fluid].any()
    share = ref["ambiguous"].sum() / fluid.sum()
    print(name, "ambiguous particles left out:", int(ref["ambiguous"].sum()), "of", int(fluid.sum()), f"= {share:.4%}")
    ok = fluid & ~ref["ambiguous"]
    worst = {}
    for col, key in enumerate(("I_ta", "I_wc", "E_k", "n_d")):
        err = np.abs(pot[:, col] - ref[key])
        bar = ref["bar_" + key].copy()
        top = np.abs(ref[key]).max()
        if fast:   # inherited, not derived (module docstring)
            bar = np.maximum(bar, 3e-5 * top)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0))[ok]
        print(name, key, "max error", err[ok].max(), "largest bar", bar[ok].max(), "column maximum", top, "worst error / bar",
              ratio.max(), "positive values", int((ref[key] > 0).sum()))
        worst[key] = (err[ok] <= bar[ok]).all()
    assert share <= AMBIGUOUS_CAP
    assert all(worst.values()), worst
    assert (ref["I_ta"] > 0).sum() > 100 and (ref["E_k"] > 0).sum() > 100


# ---- 2, 3. counts, slots, geometry ------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp64", [True, False], ids=IDS)
@pytest.mark.parametrize("name,k_ta", [("cubes2048", 40.0), ("dam8192", 2000.0), ("obstacles2048", 400.0)])
def test_children_counts_slots_and_cylinders(pkg, name, k_ta, fp64):
    s, p = stepped(pkg, name, fp64)
    dt = np.float64 if fp64 else np.float32
    N, eps = dt, float(np.finfo(dt).eps)
    cfg = configured(s, p, 1 << 18, k_ta=k_ta, k_wc=k_ta, seed=5)
    stats = s.whitewater_step(p)
    pot, down, pool = s.whitewater_potentials(), s.download(), s.whitewater_download()
    want = WR.counts(pot[:, 3], cfg["seed"], down["id"], 0, dt)
    want[down["type"] != 0] = 0
    print(name, "children", int(want.sum()), "largest count", int(want.max()), stats)
    assert stats["emitted"] + stats["dropped"] == want.sum() and stats["dropped"] == 0 and stats["alive"] == want.sum()
    assert want.sum() > 50
    if k_ta >= 400.0:
        assert want.max() >= 2
    parent = np.repeat(np.arange(len(want)), want)
    assert np.array_equal(pool["parent_id"], down["id"][parent])       # slot order = device order of the parents, then k
    x, v = down["pos"][parent].astype(np.float64), down["vel"][parent].astype(np.float64)
    assert (np.abs(down["vel"][want > 0]).sum(1) > 0).all()            # a particle at rest emits nothing
    rad, ax, along, vl = WR.cylinder(pool["pos"], pool["vel"], x, v, H, p.scale)
    rV = H * p.scale / 2
    # slack: the ~10 roundings of a coordinate of magnitude |x| + r_V, resp. of a velocity of magnitude |v| + r_V
    slack_x = 16 * eps * (np.abs(x).max(1) + rV + p.dt * vl)
    slack_v = 16 * eps * (np.abs(v).max(1) + rV)
    assert (rad <= rV + slack_x).all() and (ax >= -slack_x).all() and (ax <= p.dt * vl + slack_x).all()
    assert (along <= slack_v).all()
    phik = ((np.minimum(pot[:, 2], N(cfg["tau_k"][1])) - np.minimum(pot[:, 2], N(cfg["tau_k"][0]))).astype(dt) /
            N(N(cfg["tau_k"][1]) - N(cfg["tau_k"][0]))).astype(dt)
    life = (N(cfg["lifetime"][0]) + (phik * N(N(cfg["lifetime"][1]) - N(cfg["lifetime"][0]))).astype(dt)).astype(dt)
    assert np.array_equal(pool["life"], life[parent])
    assert np.array_equal(stats["kind"], [int((pool["kind"] == k).sum()) for k in range(3)])


@pytest.mark.parametrize("fp64", [True, False], ids=IDS)
def test_a_particle_at_rest_emits_nothing(pkg, fp64):
    """fluid particles with v == 0 among fast neighbours: one step with K = 0 and no force leaves a velocity of 0
    exactly 0 (finalise: ((pStar - x / scale) / dt + v) * 0.49 with pStar = x / scale), the neighbours keep 0.98 v.  tau_k
    starts below 0, so Phi_k > 0 at E_k = 0 and only the v == 0 select keeps such a particle from emitting."""
    dt = np.float64 if fp64 else np.float32
    rng = np.random.default_rng(3)
    n = 1500
    sc = dict(id=np.arange(n, dtype=np.uint64) + 100, type=np.zeros(n, np.uint8), mass=np.ones(n, dt),
              pos=(rng.random((n, 3)) * 250 + 300).astype(dt), vel=((rng.random((n, 3)) - 0.5) * 2).astype(dt),
              colour=rng.random((n, 4)).astype(dt))
    rest = np.arange(0, n, 10)
    sc["vel"][rest] = 0
    p = pkg.default_params(0, 1000.0)
    p.constant_force[:] = [0.0, 0.0, 0.0]
    s = pkg.Solver(h=H, fp64=fp64).upload(**sc).step(p)
    cfg = dict(capacity=1 << 16, k_ta=3000.0, k_wc=0.0, tau_ta=(0.0, 0.5), tau_wc=(0.0, 1.0), tau_k=(-1.0, 1.0), seed=2)
    s.whitewater_configure(**cfg)
    stats = s.whitewater_step(p)
    down, pot, pool = s.download(), s.whitewater_potentials(), s.whitewater_download()
    still = ~down["vel"].any(1)
    assert np.array_equal(np.sort(down["id"][still]), sc["id"][rest])
    assert (pot[still, 0] > 0).sum() > 100 and not pot[still, 2].any() and not pot[still, 3].any()
    assert stats["emitted"] > 1000 and stats["dropped"] == 0
    assert not np.isin(pool["parent_id"], down["id"][still]).any()
    assert np.isfinite(pool["pos"]).all() and np.isfinite(pool["vel"]).all()
    want = WR.counts(pot[:, 3], cfg["seed"], down["id"], 0, dt)
    assert np.array_equal(pool["parent_id"], down["id"][np.repeat(np.arange(n), want)])


# ---- 4. advection, bit for bit ----------------------------------------------------------------------------------------

def advect_pool(s, p, n, dtype):
    rng = np.random.default_rng(23)
    down = s.download()
    fl = down["pos"][down["type"] == 0].astype(np.float64)
    lo, hi = fl.min(0), fl.max(0)
    cell = H * p.scale
    pos = np.empty((n, 3))
    pos[:100] = fl[rng.integers(0, len(fl), 100)] + (rng.random((100, 3)) - 0.5) * cell          # in the fluid
    order = np.argsort(fl[:, 1])                 # (gravity points along +y: the free surface is at the low end)
    rim = np.concatenate([fl[order[:30]], fl[order[-30:]]])
    out = np.concatenate([-np.ones(30), np.ones(30)])[:, None] * np.array([0.0, 1.0, 0.0])
    pos[100:160] = rim + out * (0.6 * cell) * rng.random((60, 1))                              # at the surface
    pos[160:200] = rim[10:50] + out[10:50] * (3.0 * cell) + (rng.random((40, 3)) - 0.5) * cell  # beyond it
    pos[200:220] = np.array([p.max_bound[0] + 5000.0, 500.0, 500.0]) + rng.random((20, 3))     # outside the grid
    pos[220:240] = lo + rng.random((20, 3)) * (hi - lo)
    pos[220:240, 1] = p.min_bound[1]                                                           # on a bound
    pos[240:] = fl[rng.integers(0, len(fl), n - 240)]
    vel = (rng.random((n, 3)) - 0.5) * 0.4
    life = np.full(n, 3.0)
    life[240:250] = p.dt * 0.5                                                                 # life < dt
    pos, vel, life = pos.astype(dtype), vel.astype(dtype), life.astype(dtype)
    pos[250, 1] = np.nan
    vel[251, 2] = np.nan
    return dict(pos=pos, vel=vel, life=life)


@pytest.mark.parametrize("fp64", [True, False], ids=IDS)
@pytest.mark.parametrize("name", ["dam8192", "obstacles2048"])
def test_advection_bit_for_bit(pkg, name, fp64):
    s, p = stepped(pkg, name, fp64)
    dt = np.float64 if fp64 else np.float32
    cfg = dict(capacity=257, k_ta=0.0, k_wc=0.0, tau_ta=(0, 1), tau_wc=(0, 1), tau_k=(0, 1), k_b=2.0, k_d=0.8, spray_below=6,
               bubble_from=20)
    s.whitewater_configure(**cfg)
    pool = advect_pool(s, p, 257, dt)
    s.whitewater_upload(**pool)
    assert s.whitewater_count == 257
    back = s.whitewater_download()
    assert all(np.array_equal(back[k], pool[k], equal_nan=True) for k in pool)
    pts = np.where(np.isfinite(pool["pos"]), pool["pos"], 1e9).astype(np.float64)   # (a NaN position is outside the grid)
    smp = s.sample(p, pts, velocity=True)
    want = WR.advect(pool, smp, cfg, p, dt)
    stats = s.whitewater_step(p)
    got = s.whitewater_download()
    a = want["alive"]
    print(name, "kinds uploaded", np.bincount(want["kind"], minlength=3), "alive", int(a.sum()), stats)
    assert np.bincount(want["kind"], minlength=3).min() >= 3 and 100 <= a.sum() <= 257 - 22
    assert stats["alive"] == a.sum() == s.whitewater_count and stats["died"] == 257 - a.sum() and stats["emitted"] == 0
    for k in ("pos", "vel", "life", "kind"):
        assert got[k].tobytes() == np.ascontiguousarray(want[k][a]).tobytes(), k
    assert np.array_equal(stats["kind"], np.bincount(want["kind"][a], minlength=3))
    assert (got["parent_id"] == np.uint64(2 ** 64 - 1)).all()


# ---- 5. capacity ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("capacity", [1, 65, 257])
def test_capacity_keeps_the_first_children(pkg, capacity):
    s, p = stepped(pkg, "cubes2048", False)
    cfg = configured(s, p, 1 << 16, k_ta=400.0, k_wc=400.0, seed=3)
    full = s.whitewater_step(p)
    everything = s.whitewater_download()
    assert full["alive"] > 257 and full["dropped"] == 0
    cfg["capacity"] = capacity
    s.whitewater_configure(**cfg)                  # (another capacity: a new, empty pool; frame 0 again)
    st = s.whitewater_step(p)
    kept = s.whitewater_download()
    assert st["alive"] == capacity == s.whitewater_count and st["dropped"] == full["alive"] - capacity and st["emitted"] == capacity
    assert all(np.array_equal(kept[k], everything[k][:capacity]) for k in kept)
    st2 = s.whitewater_step(p)                     # a full pool: survivors first, children only into what the dead left
    assert st2["alive"] <= capacity and st2["alive"] == st2["emitted"] + capacity - st2["died"]


# ---- 6. determinism ---------------------------------------------------------------------------------------------------

def run_sequence(pkg, options, seed=7, capacity=4096, fp64=False):
    s, p = stepped(pkg, "cubes2048", fp64, **options)
    cfg = configured(s, p, capacity, k_ta=200.0, k_wc=200.0, seed=seed)
    out = []
    for _ in range(5):
        s.step(p)
        s.whitewater_step(p)
        out.append(pool_bytes(s))
    return out, s.whitewater_potentials().tobytes(), cfg


def test_same_sequence_same_bytes_on_every_gather_kernel(pkg):
    base, pot, cfg = run_sequence(pkg, {})
    assert len(base[-1]) > 1000 * 37
    again, pot2, _ = run_sequence(pkg, {})
    assert again == base and pot2 == pot
    for options in ({"gather": 0}, {"gather": 3}, {"row_major": 0}, {"gather": 0, "row_major": 0}):   # (every one of these steps bit-identically)
        other, pot3, cfg3 = run_sequence(pkg, options)
        assert cfg3 == cfg and pot3 == pot and other == base, options
    # "coop" shares a particle's list among lanes in lambda / delta-p with rounding-level differences: the FLUID differs, so
    # the invariance is stated on the same resident state — the whitewater step itself must not depend on the option
    s, p = stepped(pkg, "cubes2048", False)
    cfg1 = configured(s, p, 4096, k_ta=200.0, k_wc=200.0, seed=7)
    s.whitewater_step(p)
    one, pot_one = pool_bytes(s), s.whitewater_potentials().tobytes()
    s.set_option("coop", 4)
    s.whitewater_configure(**{**cfg1, "capacity": 4097})    # (another capacity: an empty pool, frame 0 again)
    s.whitewater_step(p)
    assert pool_bytes(s) == one and s.whitewater_potentials().tobytes() == pot_one and len(one) > 100 * 37
    seeded, pot4, _ = run_sequence(pkg, {}, seed=8)
    assert pot4 == pot and seeded[0] != base[0]


@pytest.mark.parametrize("capacity", [0, 1, 65, 257, 4096])
def test_pool_sizes_cross_a_wave_and_a_block(pkg, capacity):
    """the same five frames at every pool size: what fits is the prefix of what a large pool holds after the first frame,
    and every frame's record adds up"""
    s, p = stepped(pkg, "cubes2048", False)
    if capacity == 0:
        s.whitewater_configure(capacity=0, tau_ta=(0, 1), tau_wc=(0, 1), tau_k=(0, 1))
        assert s.whitewater_count == 0
        assert s.L.pbf_whitewater_step(s.ctx, C.byref(p), None) == ERR_STATE
        return
    configured(s, p, capacity, k_ta=200.0, k_wc=200.0, seed=7)
    before = 0
    for _ in range(5):
        s.step(p)
        st = s.whitewater_step(p)
        assert st["alive"] == before - st["died"] + st["emitted"] <= capacity and sum(st["kind"]) == st["alive"]
        assert s.whitewater_count == st["alive"]
        before = st["alive"]
    assert before > 0


# ---- 7. non-interference ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [0, 1])
def test_a_fluid_step_never_notices(pkg, graph):
    def run(with_ww):
        K, _, side = SCENES["dam8192"]
        s = pkg.Solver(h=H, flags=0)
        s.set_option("graph", graph)
        p = pkg.default_params(K, side)
        s.upload(**make_scene(pkg, "dam8192", False))
        if with_ww:
            s.whitewater_configure(capacity=4096, k_ta=50.0, k_wc=50.0, tau_ta=(0.0, 0.5), tau_wc=(0.0, 0.5), tau_k=(0.0, 0.01))
        for _ in range(10):
            s.steps(p, 1)
            if with_ww:
                s.whitewater_step(p)
        return s.download(), s.graph_stats()
    (a, ga), (b, gb) = run(True), run(False)
    assert all(np.array_equal(a[k], b[k]) for k in a) and ga == gb
    if graph:
        assert ga[1] > 0


def test_stage_calls_surface_record_and_diagnostics_are_untouched(pkg):
    K, _, side = SCENES["cubes2048"]
    p = pkg.default_params(K, side)

    def run(with_ww):
        s = pkg.Solver(h=H, flags=pkg.FLAG_STAGE_TIMING)
        s.upload(**make_scene(pkg, "cubes2048", False))
        s.set_surface_tension(0.05, 0.0)
        if with_ww:
            s.whitewater_configure(capacity=4096, k_ta=50.0, k_wc=50.0, tau_ta=(0.0, 0.5), tau_wc=(0.0, 0.5), tau_k=(0.0, 0.01))
        for _ in range(4):
            s.step(p)
            if with_ww:
                s.whitewater_step(p)
        return s

    a, b = run(True), run(False)
    assert {k: v[1] for k, v in a.stage_times().items()} == {k: v[1] for k, v in b.stage_times().items()}
    assert np.array_equal(a.surface_state(), b.surface_state())
    before = bytes(a.diagnostics(p, density=True, raw=True))
    surf = a.surface_state().copy()
    a.whitewater_step(p)
    assert bytes(a.diagnostics(p, density=True, raw=True)) == before and np.array_equal(a.surface_state(), surf)
    assert bytes(b.diagnostics(p, density=True, raw=True)) == before


# ---- 8. errors --------------------------------------------------------------------------------------------------------

def test_refusals(pkg):
    p = pkg.default_params(4, 1000.0)
    sc = make_scene(pkg, "cubes2048", False)
    s = pkg.Solver(h=H).upload(**sc)
    L = s.L
    good = dict(capacity=65, k_ta=1.0, k_wc=1.0, tau_ta=(0, 1), tau_wc=(0, 1), tau_k=(0, 1))
    step = lambda q=p: L.pbf_whitewater_step(s.ctx, C.byref(q), None)
    assert step() == ERR_STATE                                   # unconfigured
    s.whitewater_configure(**good)
    assert step() == ERR_STATE                                   # before any fluid step
    s.step(p)
    assert step() == 0
    pts = np.random.default_rng(1).random((40, 3)) * 300 + 100
    s.whitewater_upload(pts)
    kept = pool_bytes(s)
    foreign = pkg.default_params(4, 1000.0)
    foreign.max_bound[0] = 700.0
    assert step(foreign) == ERR_STATE and L.pbf_whitewater_step(s.ctx, None, None) == ERR_INVALID
    for field in ("dt", "scale"):
        for value in (0.0, -1.0):
            q = pkg.default_params(4, 1000.0)
            setattr(q, field, value)
            assert step(q) == ERR_INVALID and pool_bytes(s) == kept
    bad = [dict(k_ta=-1.0), dict(k_wc=float("nan")), dict(k_ta=float("inf")), dict(tau_ta=(1.0, 1.0)), dict(tau_wc=(2.0, 1.0)),
           dict(tau_k=(0.0, float("nan"))), dict(lifetime=(3.0, 2.0)), dict(k_d=1.5), dict(k_d=-0.1), dict(k_b=float("inf")),
           dict(k_b=float("nan")),
           dict(spray_below=21, bubble_from=20), dict(capacity=2 ** 31)]
    for change in bad:
        w = pkg.whitewater_config(**{**good, **change})
        assert L.pbf_whitewater_configure(s.ctx, C.byref(w)) == ERR_INVALID, change
        assert pool_bytes(s) == kept and s.whitewater_count == 40
    assert L.pbf_whitewater_configure(s.ctx, None) == ERR_INVALID
    big = np.zeros((66, 3), np.float32)
    assert L.pbf_whitewater_upload(s.ctx, 66, big.ctypes.data_as(C.c_void_p), None, None) == ERR_INVALID
    assert L.pbf_whitewater_upload(s.ctx, 3, None, None, None) == ERR_INVALID
    assert pool_bytes(s) == kept
    pot = np.empty((s.n, 4), np.float32)
    read = lambda: L.pbf_read_buffer(s.ctx, pkg.BUF_WHITEWATER, pot.ctypes.data_as(C.c_void_p), pot.nbytes)
    assert step() == 0 and read() == 0
    s.step(p)
    assert read() == ERR_STATE                                   # the arrays have changed since
    s.upload(**sc)
    assert step() == ERR_STATE and read() == ERR_STATE           # after pbf_upload: no table
    s.whitewater_configure(**{**good, "capacity": 0})
    assert s.whitewater_count == 0 and step() == ERR_STATE
    # a slab-configured context
    t = pkg.Solver(h=H).upload(**sc)
    t.whitewater_configure(**good)
    t.step(p)
    cut = pkg.SlabCut(0, 12, 0, 0)
    assert L.pbf_slab_configure(t.ctx, C.byref(cut), 0, 0) == 0
    assert L.pbf_whitewater_step(t.ctx, C.byref(p), None) == ERR_STATE


# ---- 9. shim and CLI --------------------------------------------------------------------------------------------------

def test_shim(pkg):
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_whitewater_shim")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr


def test_benchmark_whitewater_flag(pkg, tmp_path):
    BIN = os.path.join(ROOT, "pbf-sph_amd", "benchmark")
    out = tmp_path / "out"
    common = ["--resident", "--scene", "dam-break", "--particles", "8192", "--solver-iter", "2", "--no-surface", "-n", "12", "-w", "4",
              "-o", str(out)]
    r = subprocess.run([BIN, *common, "--whitewater=300,300,20000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    alive = int(re.search(r"Whitewater\s+: (\d+) alive", r.stdout).group(1))
    ply = (out / "whitewater.ply").read_text().split("\n")
    assert int(next(l for l in ply if l.startswith("element vertex")).split()[-1]) == alive > 0
    body = [l for l in ply[ply.index("end_header") + 1:] if l]
    assert len(body) == alive and {l.split()[3] for l in body} <= {"0", "1", "2"} and (out / "cloud.ply").exists()
    # without the flag: no file, no line; its refusals
    plain = tmp_path / "plain"
    r = subprocess.run([BIN, *common[:-1], str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Whitewater" not in r.stdout and not (plain / "whitewater.ply").exists()
    r = subprocess.run([BIN, *common, "--slabs", "2", "--whitewater=1,1"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--whitewater is a single-device feature" in r.stderr
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert "--whitewater=" in r.stdout
