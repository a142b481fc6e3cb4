"""N-version check of the parity-unpinned floating-point stages (VERDICT r02 #1c): the oracle's lambda / delta-p /
finalise (and the opt-in vorticity / XSPH) against tests/nversion.py — a grid-free, sort-free, all-pairs float64
evaluation written from the reference's text (ompsph.hpp:215-264) alone.  Two independent restatements of the
same lines agreeing to 1e-12 is not the reference binary agreeing (parity stays "unpinned": the reference's
OpenMP backend needs glm, which this image lacks), but it removes the failure mode "oracle and kernel share one
misreading" for everything the two restatements do not share: the grid walk, the sort, the candidate order, the
constants' promotion, the kernels' branches.
"""
import numpy as np
import pytest

import nversion as NV
import oracle_lib as O

REL = 1e-12


def rel_err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def scene(name):
    rng = np.random.default_rng(17)
    if name == "cubes1024":
        sc = O.scene_cubes(1024, True)
    elif name == "cloud":      # ~rest density, irregular, some particles ON the box walls (clamp), coincident pairs
        n = 1800
        pos = rng.random((n, 3)) * np.array([330.0, 330.0, 330.0]) + np.array([0.0, 670.0, 0.0])
        pos[:40, 0] = 0.0
        pos[40:80, 1] = 1000.0
        pos[80:90] = pos[90:100]           # r = 0 between different particles
        sc = dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n), pos=pos,
                  vel=(rng.random((n, 3)) - 0.5) * 2.0, colour=rng.random((n, 4)))
    elif name == "obstacles":  # + obstacle particles (lambda = 0, fixed, still neighbours) and unequal masses
        sc = O.scene_cubes(1024, True)
        sc["type"][::5] = 1
        sc["mass"] = 0.5 + rng.random(len(sc["id"]))
    elif name == "obstacles_moving":   # the obstacles CARRY a velocity (predict and finalise never touch it): what the
        sc = scene("obstacles")        # opt-in velocity passes read from an obstacle neighbour is then not 0
        obstacle = sc["type"] == 1
        sc["vel"] = sc["vel"].copy()
        sc["vel"][obstacle] = (rng.random((int(obstacle.sum()), 3)) - 0.5) * 2.0
    elif name == "pile":       # 300 fluid + 20 obstacles inside 0.045 solver units, across a cell corner: every particle
        n = 320                # is within h of nearly every other.  r = 0 with DIFFERENT velocities: five fluid particles
        pos = rng.random((n, 3)) * 22.5 + 489.0        # at rest lie on five obstacles that carry a velocity (a fluid
        vel = (rng.random((n, 3)) - 0.5) * 2.0         # particle at rest stays put with no force and no iterations, a
        type_ = np.zeros(n, np.uint8)                  # moving one would leave), and two fluid pairs at rest coincide
        type_[300:] = 1
        pos[10:15], vel[10:15] = pos[300:305], 0.0
        pos[20:22], vel[20:24] = pos[22:24], 0.0
        sc = dict(id=np.arange(n, dtype=np.uint64), type=type_, mass=0.5 + rng.random(n), pos=pos, vel=vel,
                  colour=rng.random((n, 4)))
    elif name.startswith("edges"):   # edges1 / edges65 / edges257: a line-by-line filled block at rest spacing, moving
        n = int(name[5:])
        k = int(np.ceil(n ** (1.0 / 3.0)))
        g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
        sc = dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n),
                  pos=g * 27.0 + 437.0, vel=(rng.random((n, 3)) - 0.5) * 2.0, colour=rng.random((n, 4)))
    else:
        raise KeyError(name)
    return sc


@pytest.mark.parametrize("name", ["cubes1024", "cloud", "obstacles"])
def test_oracle_lambda_delta_finalise_equal_all_pairs_evaluation(name):
    sc = scene(name)
    q = O.make_params(iteration=1, mode=O.JACOBI, sort=O.SORT_STABLE)
    o = O.Oracle(True, device_pow=False)       # std::pow exactly as ompsph.hpp:240
    o.set_particles(**sc)
    if name == "cubes1024":
        for _ in range(3):                     # leave the lattice: an irregular, partly wall-clamped state
            o.step(q)
    o.predict(q).sort(q).grid_table(q)
    st = o.get_particles()                     # sorted order; vel = predicted velocity
    ps = o.pstar().astype(np.float64)
    obstacle = st["type"] == 1
    h, scale, dt = q.h, q.scale, q.dt
    assert o.keys().max() < len(o.table()), "every particle must lie inside the grid for the all-pairs equivalence"
    cells = NV.predict_cells(ps, h, scale, list(q.min_bound))   # fixed at predict time (ompsph.hpp:152)
    for it in range(2):
        o.lambda_(q)
        # first iteration: plain all pairs (a pair within h is always inside the 27 cells); later ones: pStar has
        # moved away from the cells it was binned into, the walk only sees the predict-time neighbourhood
        cm = None if it == 0 else cells
        lam, rho = NV.lambdas(ps, st["mass"].astype(np.float64), h, obstacle, cm)
        assert rel_err(o.lambdas(), lam) <= REL, (name, it, "lambda")
        o.delta(q)
        ps_new, dp = NV.delta(ps, lam, h, scale, list(q.min_bound), list(q.max_bound), obstacle, cm)
        # pStar is O(1), deltaP O(1e-3): compare the MOVE so that the bar bites on the computed part
        move_o, move_n = o.pstar() - ps, ps_new - ps
        assert np.abs(move_o - move_n).max() <= REL * max(np.abs(move_n).max(), 1e-30) + 4e-16, (name, it, "delta-p")
        ps = o.pstar().astype(np.float64)      # continue from the oracle's state (errors do not compound)
    pos_before, vel_before = st["pos"].astype(np.float64), st["vel"].astype(np.float64)
    o.finalise(q)
    pos, vel = NV.finalise(ps, pos_before, vel_before, dt, scale)
    g = o.get_particles()
    keep = ~obstacle
    assert rel_err(g["pos"][keep], pos[keep]) <= REL and rel_err(g["vel"][keep], vel[keep]) <= 1e-11
    assert np.array_equal(g["pos"][obstacle], pos_before[obstacle])


def test_oracle_predict_equals_formula():
    sc = scene("cloud")
    q = O.make_params(iteration=0)
    o = O.Oracle(True)
    o.set_particles(**sc)
    o.predict(q)
    v, ps = NV.predict(sc["pos"], sc["vel"], sc["mass"], q.dt, q.scale, list(q.constant_force))
    assert rel_err(o.pstar(), ps) <= REL and rel_err(o.get_particles()["vel"], v) <= REL


@pytest.mark.parametrize("name", ["cubes1024", "cloud", "obstacles_moving"])
def test_oracle_extras_equal_all_pairs_evaluation(name):
    """The opt-in extras (absent from the reference; Macklin & Mueller 2013 eq. 15-17) against the same equations
    evaluated over all pairs — including the SIGN of the vorticity (eq. 15 differentiates with respect to the
    neighbour's position) and, on obstacles_moving, the obstacle rule: no vorticity and no velocity change of its own, a
    full neighbour with the velocity it carries."""
    sc = scene(name)
    q = O.make_params(iteration=2)
    o = O.Oracle(True)
    o.set_particles(**sc)
    for _ in range(2):
        o.step(q)
    q0 = O.make_params(iteration=2)
    o.predict(q0).sort(q0).grid_table(q0)
    cells = NV.predict_cells(o.pstar().astype(np.float64), q0.h, q0.scale, list(q0.min_bound))
    for _ in range(2):
        o.lambda_(q0).delta(q0)
    o.finalise(q0)                             # extras run on the post-solve state, in the predict-time cells
    ps = o.pstar().astype(np.float64)
    vel = o.get_vec(0).astype(np.float64)
    obstacle = o.get_particles()["type"] == 1      # (all False but on obstacles_moving)
    assert obstacle.any() == (name == "obstacles_moving")
    o.vorticity(q0)
    w = NV.vorticity(ps, vel, q0.h, cells, obstacle=obstacle)
    assert rel_err(o.get_vec(1), w) <= 1e-11
    o.vorticity_force(q0)
    dv = NV.vorticity_force_dv(ps, w, q0.h, q0.dt, cells, obstacle=obstacle)
    assert np.abs((o.get_vec(0) - vel) - dv).max() <= 1e-9 * np.abs(dv).max()
    vel2 = o.get_vec(0).astype(np.float64)
    o.xsph(q0)
    dx = NV.xsph(ps, vel2, q0.h, cells, obstacle=obstacle) - vel2
    assert np.abs((o.get_vec(0) - vel2) - dx).max() <= 1e-9 * np.abs(dx).max()
    assert np.array_equal(o.get_vec(0)[obstacle], vel[obstacle])


def rotating_blob(n_side=14, spacing=27.0, omega_z=3.0, centre=(500.0, 500.0, 500.0), fp64=True):
    """A block of fluid at rest spacing (6378^(-1/3) solver units = 27 world units) in rigid rotation about +z
    through its centre: v = Omega z_hat x r, curl v = 2 Omega z_hat."""
    dt = np.float64 if fp64 else np.float32
    ax = (np.arange(n_side) - (n_side - 1) / 2.0) * spacing
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    vel = np.stack([-omega_z * g[:, 1], omega_z * g[:, 0], np.zeros(len(g))], -1) / 500.0   # solver units = world / scale
    n = len(g)
    return dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n, dt),
                pos=(g + np.asarray(centre)).astype(dt), vel=vel.astype(dt), colour=np.full((n, 4), 0.5, dt)), g


def angular_momentum_z(pos, vel, centre):
    r = pos.astype(np.float64) - np.asarray(centre)
    return float((r[:, 0] * vel[:, 1].astype(np.float64) - r[:, 1] * vel[:, 0].astype(np.float64)).sum())


def test_oracle_rigid_rotation_vorticity_points_along_the_rotation_axis():
    """with (v_b - v_a) x grad_{p_a} W a rigid +z rotation gave omega = (0, 0, -|w|) and the
    confinement force DECELERATED vortices.  Physical property, independent of any restatement: omega must be parallel
    to +z (curl v = 2 Omega) and the confinement force must not remove angular momentum about that axis."""
    sc, rel = rotating_blob()
    centre = (500.0, 500.0, 500.0)
    q = O.make_params(iteration=0, force=(0.0, 0.0, 0.0), vorticity=0, xsph=0)
    o = O.Oracle(True)
    o.set_particles(**sc)
    o.step(q)                                  # K = 0, no gravity: advect by v dt, v <- 0.98 v, state sorted
    st = o.get_particles()
    r = np.linalg.norm(st["pos"] - np.asarray(centre), axis=1)
    inner = r < 100.0                          # full kernel support
    o.vorticity(q)
    w = o.get_vec(1)
    assert np.all(w[inner, 2] > 0), "omega must point along +z for a +z rotation"
    assert np.abs(w[inner, :2]).max() < 1e-6 * np.abs(w[inner, 2]).min()
    l0 = angular_momentum_z(st["pos"], o.get_vec(0), centre)
    o.vorticity_force(q)
    l1 = angular_momentum_z(st["pos"], o.get_vec(0), centre)
    assert l0 > 0 and l1 > l0, ("vorticity confinement must add angular momentum to a vortex, not remove it", l0, l1)


def test_oracle_xsph_conserves_momentum_and_smooths():
    sc = scene("cloud")
    q = O.make_params(iteration=2)
    o = O.Oracle(True)
    o.set_particles(**sc)
    o.step(q)
    v0 = o.get_vec(0).astype(np.float64)
    o.xsph(q)
    v1 = o.get_vec(0).astype(np.float64)
    assert np.abs(v1.sum(0) - v0.sum(0)).max() <= 1e-12 * np.abs(v0).sum()   # equal masses: sum m v unchanged
    assert v1.var(0).sum() < v0.var(0).sum()                                   # a smoothing filter
