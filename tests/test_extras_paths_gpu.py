"""The six opt-in velocity ops (VorticityOp, VorticityForceOp, XsphOp; SurfaceDensityOp, SurfaceNormalOp, SurfaceTensionOp)
on every kernel launch_gather(..., GATHER_PLAIN) can send them to, with obstacles that carry a velocity.

  1. the default path (k_gather_lists<N, Op, 16>) against the independent float64 all-pairs evaluation, particle by particle,
     under tests/extras_ref.py's derived bars (validated on the CPU by tests/test_extras_ref_cpu.py);
  2. device == oracle bit for bit on a scene whose obstacles move;
  3. every other launchable path — k_gather_global (gather = 0, pad_lds, PBF_FLAG_NO_LDS), k_gather_lists<.., 12 / 24 / 32>
     (list_max), gather = 3, row_major = 0 — gives the default path's BYTES, with all three passes on;
  4. a captured graph replays the same bytes;
  5. n = 1, 65, 257.

Each pass is measured alone by the twin-solver scheme of tests/test_surface_tension_gpu.py: one run with the pass off, one with
it on (identical ids and positions), the increment is the difference of the two velocities; the predict-time cells come
from a third run stopped after its sort.  The scenes are tests/test_nversion_cpu.py's, their step counts extras_ref.SCENES'.
"""
import numpy as np
import pytest

import extras_ref as ER
from sample_ref import key_cells
from test_hip_parity import assert_state_equal, by_id, params_pair
from test_nversion_cpu import scene

pytestmark = pytest.mark.gpu

H = 0.1
VARIANTS = [(True, False), (False, False), (False, True)]   # (fp64, PBF_FLAG_FAST_MATH)
IDS = ["fp64", "fp32", "fp32-fast"]
# what launch_gather branches on (coop is left out: it does not reach these ops, kTileable = false)
PATHS = [dict(gather=0), dict(gather=0, pad_lds=16384), dict(flags="NO_LDS"), dict(gather=3), dict(row_major=0),
         dict(list_max=12), dict(list_max=24), dict(list_max=32), dict(list_max=12, row_major=0)]
ALL = ("vorticity", "xsph", "surface")


def params(pkg, name, passes=(), iteration=None):
    """iteration: a solver iteration count other than the scene's own"""
    own, _, force = ER.SCENES[name]
    iteration = own if iteration is None else iteration
    p = pkg.default_params(iteration, 1000.0)
    for c in range(3):
        p.constant_force[c] = force[c]
    p.vorticity, p.xsph = int("vorticity" in passes), int("xsph" in passes)
    return p


def run(pkg, name, fp64, fast, passes=(), path=None, stop_after_sort=False, solids=None, iteration=None):
    """-> the solver after the scene's warm steps (passes off) and ONE step with `passes` on; solids(s, name, fp64), when given,
    installs what the ctx carries beside the particles, right after the upload; iteration: params()'s"""
    path = dict(path or {})
    flags = (pkg.FLAG_FAST_MATH if fast else 0) | (pkg.FLAG_NO_LDS if path.pop("flags", None) else 0)
    s = pkg.Solver(h=H, fp64=fp64, flags=flags)
    for k, v in path.items():
        s.set_option(k, v)
    s.upload(**scene(name))
    if solids:
        solids(s, name, fp64)
    p0 = params(pkg, name, iteration=iteration)
    warm = ER.SCENES[name][1]
    if warm:
        s.steps(p0, warm)
    if stop_after_sort:
        return s.stage("predict", p0).stage("sort", p0)
    if "surface" in passes:
        s.set_surface_tension(ER.GAMMA, ER.BETA)
    return s.step(params(pkg, name, passes, iteration))


def state_bytes(s, passes, more=None):
    """more(s) -> further named bytes of the ctx (the records of its solids)"""
    out = {k: v.tobytes() for k, v in s.download().items()}
    if more:
        out.update(more(s))
    if "vorticity" in passes:
        out["omega"] = s.omega().tobytes()
    if "surface" in passes:
        out["surface_state"] = s.surface_state().tobytes()
    return out


def check_against_reference(pkg, name, fp64, fast, solids=None, also=None, iteration=None):
    """test 1 for one scene and variant -> {record: (worst error / bar, ambiguous share)}; solids: run()'s; also(on, off, passes),
    when given, holds whatever else a pass must leave alone; iteration: params()'s"""
    dtype = np.float64 if fp64 else np.float32
    p = params(pkg, name, iteration=iteration)
    off = run(pkg, name, fp64, fast, solids=solids, iteration=iteration)
    a = off.download()
    cut = run(pkg, name, fp64, fast, stop_after_sort=True, solids=solids, iteration=iteration)
    assert np.array_equal(cut.download()["id"], a["id"])
    cells = key_cells(cut.keys())
    ps = off.pstar()[:, :3].astype(np.float64)
    vel, mass = a["vel"].astype(np.float64), a["mass"].astype(np.float64)
    obstacle = a["type"] == 1
    fluid = ~obstacle
    h, dt, gamma, beta = ER.kernel_inputs(dtype, H, p.dt, ER.GAMMA, ER.BETA)
    P = ER.Pairs(ps, h, dtype, cells)
    seen, failed = {}, []

    def hold(record, got, value, bar, amb):
        extra = ER.fast_allowance(value) if fast else 0.0
        ratio, err = ER.worst(got, value, bar, fluid & ~amb, extra)
        share = amb.sum() / max(int(fluid.sum()), 1)
        print(f"{name} {IDS[VARIANTS.index((fp64, fast))]} {record}: worst error / bar {ratio:.3f}, largest error {err:.3e}, "
              f"ambiguous {100 * share:.2f} %")
        if fast:                                                 # what the inherited allowance could be tightened to
            print(f"    without the fast-math allowance: worst error / derived bar {ER.worst(got, value, bar, fluid & ~amb)[0]:.3f}; "
                  f"allowance {np.max(extra):.3e}")
        seen[record] = (ratio, share)
        if not ratio <= 1.0 or share > ER.AMBIGUOUS_CAP:
            failed.append(record)
        assert not np.asarray(got)[obstacle].any(), (record, "an obstacle's record must be zero")

    def twin(passes):
        on = run(pkg, name, fp64, fast, passes, solids=solids, iteration=iteration)
        b = on.download()
        assert np.array_equal(a["id"], b["id"]) and np.array_equal(a["pos"], b["pos"])   # the pass runs after the solve
        assert np.array_equal(on.pstar()[:, :3], off.pstar()[:, :3])
        assert np.array_equal(a["vel"][obstacle], b["vel"][obstacle])                    # bit for bit
        if also:
            also(on, off, passes)
        return on, b["vel"].astype(np.float64) - vel

    on, dv = twin(("vorticity",))
    w = on.omega().astype(np.float64)
    hold("omega", w, *ER.vorticity(P, vel, obstacle))
    hold("confinement", dv, *ER.confinement(P, vel, w, dt, obstacle))
    on, dv = twin(("xsph",))
    hold("xsph", dv, *ER.xsph(P, vel, obstacle))
    on, dv = twin(("surface",))
    ref, amb = ER.surface(P, vel, mass, dt, gamma, beta, obstacle)
    st = on.surface_state().astype(np.float64)
    hold("rho", st[:, 3], *ref["rho"], amb)
    hold("normal", st[:, :3], *ref["n"], amb)
    hold("tension", dv, *ref["dv"], amb)
    assert not failed, (failed, seen)
    return seen


def check_paths(pkg, name, fp64, fast, paths, solids=None, more=None, iteration=None):
    """test 3 for one scene and variant: every path's bytes equal the default path's, passes on and off; solids: run()'s,
    more: state_bytes()'s, iteration: params()'s"""
    want_on = state_bytes(run(pkg, name, fp64, fast, ALL, solids=solids, iteration=iteration), ALL, more)
    want_off = state_bytes(run(pkg, name, fp64, fast, solids=solids, iteration=iteration), (), more)
    assert want_on["vel"] != want_off["vel"]
    for path in paths:
        got_off = state_bytes(run(pkg, name, fp64, fast, (), path, solids=solids, iteration=iteration), (), more)
        solve = [k for k in want_off if got_off[k] != want_off[k]]
        assert not solve, (path, "the SOLVE differs from the default path's (passes off)", solve)
        got_on = state_bytes(run(pkg, name, fp64, fast, ALL, path, solids=solids, iteration=iteration), ALL, more)
        passes = [k for k in want_on if got_on[k] != want_on[k]]
        assert not passes, (path, "the opt-in PASSES differ from the default path's (the solve does not)", passes)


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", ["obstacles_moving", "cloud", "pile"])
def test_default_path_within_the_derived_bars_per_particle(pkg, name, fp64, fast):
    seen = check_against_reference(pkg, name, fp64, fast)
    assert set(seen) == {"omega", "confinement", "xsph", "rho", "normal", "tension"}


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_device_equals_oracle_with_moving_obstacles(pkg, oracle, fp64):
    sc = scene("obstacles_moving")
    s = pkg.Solver(h=H, fp64=fp64).upload(**sc)
    o = oracle.Oracle(fp64, device_pow=True)
    o.set_particles(**sc)
    p, q = params_pair(pkg, oracle, iteration=2)
    p.xsph = p.vorticity = q.xsph = q.vorticity = 1
    for frame in range(4):
        s.step(p)
        o.step(q)
        assert_state_equal(s.download(), o.get_particles(), f"frame {frame}")
    g, orig = by_id(s.download()), by_id(sc)
    obstacle = orig["type"] == 1
    assert np.abs(orig["vel"][obstacle]).max() > 0.5                       # they do carry a velocity, and keep it
    assert np.array_equal(g["vel"][obstacle], orig["vel"][obstacle].astype(g["vel"].dtype))


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", ["obstacles_moving", "pile"])
def test_every_path_gives_the_default_paths_bytes(pkg, name, fp64, fast):
    check_paths(pkg, name, fp64, fast, PATHS)


def test_graph_replay_gives_the_eager_bytes(pkg):
    name = "obstacles_moving"
    p = params(pkg, name, ("vorticity", "xsph"))
    out = []
    for graph in (0, 1):
        s = pkg.Solver(h=H).set_option("graph", graph).upload(**scene(name))
        s.steps(p, 4)
        out.append((state_bytes(s, ("vorticity",)), s.graph_stats()))
    assert out[0][0] == out[1][0]
    assert out[1][1][1] > 0 and out[0][1][1] == 0, (out[0][1], out[1][1])


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_a_single_particle(pkg, fp64, fast):
    on, off = run(pkg, "edges1", fp64, fast, ALL), run(pkg, "edges1", fp64, fast)
    assert not on.omega().any()
    assert state_bytes(on, ()) == state_bytes(off, ())
    st = on.surface_state().astype(np.float64)
    assert not st[:, :3].any() and st[0, 3] > 0                  # its own poly6(0), no normal


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name", ["edges65", "edges257"])
def test_block_edges(pkg, name, fp64, fast):
    """65 and 257 particles: one past a wave and one past a block — the reference and the paths in one pass"""
    check_against_reference(pkg, name, fp64, fast)
    check_paths(pkg, name, fp64, fast, [dict(gather=0), dict(list_max=12), dict(list_max=32)])
