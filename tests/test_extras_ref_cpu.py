"""The bars of tests/extras_ref.py, validated before a device sees them, and the obstacle rule of the three Macklin ops.

  * The fp32 and the fp64 ORACLE against extras_ref on every scene of tests/test_extras_paths_gpu.py: the device is bit-equal
    to this oracle (tests/test_hip_parity.py and test_extras_paths_gpu.py), so a bar that holds here cannot fail on the
    device for a reason of its own.  The oracle has no surface tension: the three Akinci records are held against
    extras_ref.emulate_surface, the three passes restated in N operation by operation.  A worst error / bar above 1 means a
    count in extras_ref's docstring is wrong.
  * Galilean properties no restatement shares a misreading with: a constant velocity added to EVERY particle, obstacles
    included, changes no omega and no XSPH increment; added to the obstacles only it changes both at exactly the fluid
    particles that have an obstacle within h.
"""
import numpy as np
import pytest

import extras_ref as ER
import nversion as NV
import oracle_lib as O
from sample_ref import key_cells
from test_nversion_cpu import scene


def solved_state(name, fp64):
    """the oracle after the warm steps and one step's predict ... finalise: what the opt-in passes read"""
    iteration, warm, force = ER.SCENES[name]
    q = O.make_params(iteration=iteration, force=force)
    o = O.Oracle(fp64)
    o.set_particles(**scene(name))
    for _ in range(warm):
        o.step(q)
    o.predict(q).sort(q).grid_table(q)
    cells = key_cells(o.keys())                                  # the neighbour set is fixed at predict time
    for _ in range(iteration):
        o.lambda_(q).delta(q)
    o.finalise(q)
    return o, q, cells


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", list(ER.SCENES))
def test_oracle_and_emulation_stay_inside_the_derived_bars(name, fp64):
    o, q, cells = solved_state(name, fp64)
    dtype = o.dtype
    st = o.get_particles()
    obstacle = st["type"] == 1
    fluid = ~obstacle
    ps, mass = o.pstar().astype(np.float64), st["mass"].astype(np.float64)
    vel = o.get_vec(0).astype(np.float64)
    h, dt, gamma, beta = ER.kernel_inputs(dtype, q.h, q.dt, ER.GAMMA, ER.BETA)
    P = ER.Pairs(ps, h, dtype, cells)
    ratios, shares = {}, {}

    def hold(record, got, value, bar, amb):
        keep = fluid & ~amb
        ratios[record], err = ER.worst(got, value, bar, keep)
        shares[record] = amb.sum() / max(int(fluid.sum()), 1)
        print(f"{name} {dtype.__name__} {record}: worst error / bar {ratios[record]:.3f}, largest error {err:.3e}, "
              f"ambiguous {100 * shares[record]:.2f} %")
        assert np.array_equal(np.asarray(got)[obstacle], np.zeros_like(np.asarray(got)[obstacle])), record

    o.vorticity(q)
    w = o.get_vec(1).astype(np.float64)
    hold("omega", w, *ER.vorticity(P, vel, obstacle))
    o.vorticity_force(q)
    vel1 = o.get_vec(0).astype(np.float64)
    hold("confinement", vel1 - vel, *ER.confinement(P, vel, w, dt, obstacle))
    o.xsph(q)
    hold("xsph", o.get_vec(0).astype(np.float64) - vel1, *ER.xsph(P, vel1, obstacle))
    rho, nrm, dv = ER.emulate_surface(ps, vel, mass, obstacle, q.h, q.dt, ER.GAMMA, ER.BETA, cells, dtype)
    ref, amb = ER.surface(P, vel, mass, dt, gamma, beta, obstacle)
    hold("rho", rho, *ref["rho"], amb)
    hold("normal", nrm, *ref["n"], amb)
    hold("tension", dv, *ref["dv"], amb)
    assert all(s <= ER.AMBIGUOUS_CAP for s in shares.values()), shares
    assert all(r <= 1.0 for r in ratios.values()), ratios
    if len(ps) > 1:                                              # the bars bound something: every record is non-trivial
        assert np.abs(w).max() > 0 and np.abs(dv).max() > 0 and np.abs(nrm).max() > 0


def test_worst_counts_a_result_that_is_not_finite_as_outside_every_bar():
    keep = np.array([True, True, True])
    for bad in (np.nan, np.inf):
        assert not ER.worst([bad, 1.0, 2.0], [0.0, 1.0, 2.0], [1e-6] * 3, keep)[0] <= 1.0      # the result
        assert not ER.worst([0.0, 1.0, 2.0], [bad, 1.0, 2.0], [1e-6] * 3, keep)[0] <= 1.0      # the reference's value
        assert not ER.worst([0.0, 1.0, 2.0], [0.0, 1.0, 2.0], [bad, 1e-6, 1e-6], keep)[0] <= 1.0   # its bar
    assert ER.worst([np.nan, 1.0, 2.0], [0.0, 1.0, 2.0], [1e-6] * 3, np.array([False, True, True])) == (0.0, 0.0)
    assert ER.worst([0.0, 1.0], [0.0, 1.0 + 1e-7], [0.0, 1e-6], np.array([True, True]))[0] == pytest.approx(0.1, rel=1e-6)
    assert ER.worst([1e-9, 1.0], [0.0, 1.0], [0.0, 1e-6], np.array([True, True]))[0] == np.inf   # a zero bar: zero error only


def test_the_bars_notice_a_wrong_term():
    """the reference's own check: an obstacle neighbour read as at rest, and ONE neighbour dropped from a particle's sum,
    are both outside the bar by orders of magnitude (measured: 2e5 bars and more; asserted: 100)"""
    o, q, cells = solved_state("obstacles_moving", False)
    st = o.get_particles()
    obstacle = st["type"] == 1
    fluid = ~obstacle
    ps, vel = o.pstar().astype(np.float64), o.get_vec(0).astype(np.float64)
    h, dt, _, _ = ER.kernel_inputs(np.float32, q.h, q.dt)
    P = ER.Pairs(ps, h, np.float32, cells)
    still = np.where(obstacle[:, None], 0.0, vel)
    # the nearest neighbour of every particle, and its term of eq. 15 and of eq. 17
    r, grad = NV.pair_tables(ps, h, cells)
    rr = np.where((r >= NV.EPSILON) & (r <= 0.8 * h), r, np.inf)
    j = rr.argmin(1)
    rows = np.arange(len(ps))
    has = fluid & np.isfinite(rr[rows, j])
    assert has.sum() > 500
    vij = vel[j] - vel
    term = {"omega": np.cross(vij, -grad[rows, j]), "xsph": NV.C_XSPH * vij * NV.poly6(r[rows, j], h)[:, None]}
    for record, fn in (("omega", ER.vorticity), ("xsph", ER.xsph)):
        value, bar, amb = fn(P, vel, obstacle)
        wrong, _, _ = fn(P, still, obstacle)
        touched = fluid & (P.inH & obstacle[None, :]).any(1)
        ratio, _ = ER.worst(wrong, value, bar, touched & ~amb)
        print(record, "obstacle neighbours at rest: error / bar", ratio)
        assert ratio > 100.0
        dropped = value - term[record]
        each = np.array([ER.worst(dropped[i:i + 1], value[i:i + 1], bar[i:i + 1], np.array([True]))[0] for i in rows[has & ~amb]])
        print(record, "nearest neighbour dropped: error / bar, smallest over the particles", each.min(), "median", np.median(each))
        assert each.min() > 100.0


def test_galilean_properties_with_obstacles():
    o, q, cells = solved_state("obstacles_moving", True)
    st = o.get_particles()
    obstacle = st["type"] == 1
    fluid = ~obstacle
    ps, vel = o.pstar().astype(np.float64), o.get_vec(0).astype(np.float64)
    d = ps[:, None, :] - ps[None, :, :]
    r = np.sqrt((d * d).sum(-1))
    r = np.where((np.abs(cells[:, None, :] - cells[None, :, :]) <= 1).all(-1), r, np.inf)
    touched = fluid & ((r <= q.h * (1 - 1e-6)) & obstacle[None, :]).any(1)
    untouched = fluid & ~((r <= q.h) & obstacle[None, :]).any(1)
    assert touched.sum() > 100 and untouched.sum() > 10

    def records(v):
        o.set_vec(0, v)
        o.vorticity(q)
        w = o.get_vec(1).copy()
        o.xsph(q)
        out = o.get_vec(0).copy()
        assert np.array_equal(out[obstacle], v[obstacle])        # an obstacle keeps its velocity bit for bit
        assert not w[obstacle].any()
        return w, out - v

    shift = np.array([0.7, -1.3, 0.4])
    w0, x0 = records(vel)
    w1, x1 = records(vel + shift)                                # everyone: only differences of velocities enter
    assert np.abs(w1 - w0).max() <= 1e-12 * np.abs(w0).max()
    assert np.abs(x1 - x0)[fluid].max() <= 1e-12 * np.abs(x0).max() + 4e-16   # (+ the add into a velocity of order 1)
    w2, x2 = records(vel + np.where(obstacle[:, None], shift, 0.0))           # the obstacles alone
    assert (w2[touched] != w0[touched]).any(1).all() and (x2[touched] != x0[touched]).any(1).all()
    assert np.array_equal(w2[untouched], w0[untouched]) and np.array_equal(x2[untouched], x0[untouched])
