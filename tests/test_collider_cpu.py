"""The static SDF collider on the CPU: tests/collider_ref.py — the NumPy restatement the device is held to bit for bit
(tests/test_collider_gpu.py) — against float64 closed forms, the edge cases of its index arithmetic, the sdf_* helpers, and
the preconditions of the GPU physics scene on a float64 all-pairs step (tests/nversion.py)."""
import numpy as np
import pytest

import collider_ref as CR
import nversion as NV

DTYPES = [np.float32, np.float64]
IDS = ["fp32", "fp64"]


# ---- (a) the tilted plane ---------------------------------------------------------------------------------------------
def plane_errors(dtype, seed, n=200_000):
    """-> (|n.w' - d - margin| of the hit particles that end on no box face, in units of eps_N * PLANE_UNIT; hit share;
    share of the hits that end on a face)"""
    lat, fr = CR.plane_case(dtype)
    rng = np.random.default_rng(seed)
    q = (rng.random((n, 3)) * 1000.0).astype(dtype) / fr[0]
    phi, moved, hit = CR.project(lat, fr, q)
    face = CR.on_face(fr, moved)
    free = hit & ~face
    w = moved[free].astype(np.float64) * CR.SCALE
    err = np.abs(CR.plane_phi(CR.PLANE_N, CR.PLANE_D, w) - CR.MARGIN)
    assert np.array_equal(moved[~hit], q[~hit])                       # a select: bit for bit
    return err / (np.finfo(dtype).eps * CR.PLANE_UNIT), hit.mean(), (hit & face).sum() / max(hit.sum(), 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_plane_projection_is_rounding_only(dtype):
    """Trilinear interpolation reproduces a plane, so a projected particle lands on phi = margin up to rounding.  The bar is
    8 x the worst measured with this restatement on seed 1 (collider_ref.PLANE_WORST); other seeds must stay below it."""
    worst = {}
    for seed in (1, 2, 3):
        units, share, on_face = plane_errors(dtype, seed)
        worst[seed] = units.max()
        print(f"{np.dtype(dtype).name} seed {seed}: worst {units.max():.3f} eps * {CR.PLANE_UNIT:.0f}, hit {100 * share:.1f} %, "
              f"of those on a face {100 * on_face:.2f} %")
        assert 0.03 < share < 0.3 and len(units) > 1000
        assert units.max() <= CR.plane_bar_units(dtype)
    assert abs(worst[1] - CR.PLANE_WORST[np.dtype(dtype).name]) <= 0.01 * CR.PLANE_WORST[np.dtype(dtype).name], worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_plane_phi_and_hit_follow_the_closed_form(dtype):
    lat, fr = CR.plane_case(dtype)
    rng = np.random.default_rng(5)
    q = (rng.random((50_000, 3)) * 1000.0).astype(dtype) / fr[0]
    phi, moved, hit = CR.project(lat, fr, q)
    w = q.astype(np.float64) * CR.SCALE
    inside = np.isfinite(phi)
    true = CR.plane_phi(CR.PLANE_N, CR.PLANE_D, w)
    tol = 64 * np.finfo(dtype).eps * CR.PLANE_UNIT
    assert np.abs(phi[inside] - true[inside]).max() <= tol
    clear = np.abs(true - CR.MARGIN) > tol                            # away from the threshold the decision is the closed form's
    assert np.array_equal(hit[inside & clear], (true < CR.MARGIN)[inside & clear])
    assert not hit[~inside].any()
    # the lattice does not cover the whole box (y ends at 838): some points are outside
    assert 0.05 < (~inside).mean() < 0.5


# ---- (b) the sphere ----------------------------------------------------------------------------------------------------
def test_sphere_interpolation_error_bound():
    """|phi_interp - phi_true| <= 3 spacing^2 / (8 r_min): the trilinear error is at most spacing^2 / 8 times the sum of the
    three pure second derivatives over the cell, which for a distance function is 2 / r, and every visited cell stays
    beyond 2/3 r_min of the centre (asserted)."""
    spacing, centre, r = 25.0, np.array([500.0, 480.0, 510.0]), 300.0
    dims = (41, 41, 41)
    origin = (0.0, -20.0, 10.0)
    lat = CR.Lattice(CR.lattice_of(lambda x: CR.sphere_phi(centre, r, x), origin, spacing, dims), origin, spacing, 0.0, np.float64)
    fr = CR.frame(CR.SCALE, (0, 0, 0), (1000, 1000, 1000), np.float64)
    rng = np.random.default_rng(3)
    d = rng.normal(size=(40_000, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    w = centre + d * rng.uniform(200.0, 450.0, size=(len(d), 1))
    phi, _, _ = CR.sample(lat, fr, w)
    inside = np.isfinite(phi)
    assert inside.mean() > 0.9
    dist = np.linalg.norm(w[inside] - centre, axis=1)
    r_min = dist.min()
    assert r_min - np.sqrt(3.0) * spacing >= 2.0 / 3.0 * r_min
    err = np.abs(phi[inside] - CR.sphere_phi(centre, r, w[inside]))
    print(f"sphere: worst interpolation error {err.max():.4f}, bound {3 * spacing ** 2 / (8 * r_min):.4f}")
    assert err.max() <= 3.0 * spacing ** 2 / (8.0 * r_min)
    assert err.max() > 1e-3                                            # (it IS an interpolation error, not rounding)


# ---- (c) the index arithmetic -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dims", [(2, 2, 2), (3, 5, 4), (23, 19, 27)])
def test_edge_points(dtype, dims):
    lat, fr, pts, names = CR.edge_case(dims, dtype)
    phi, moved, hit = CR.sample(lat, fr, pts)
    q = (pts.astype(dtype) / fr[0])
    by = dict(zip(names, range(len(names))))
    true = CR.plane_phi(CR.EDGE_N, CR.EDGE_D, pts)
    tol = 64 * np.finfo(dtype).eps * 1000.0
    for a in range(3):
        k = by[f"last{a}"]                                             # ON the last node of axis a: inside, i = dims - 2, f = 1
        assert np.isfinite(phi[k]) and abs(phi[k] - true[k]) <= tol, (a, phi[k], true[k])
        k = by[f"beyond{a}"]                                           # one ulp beyond it: outside
        assert phi[k] == np.inf and not hit[k] and np.array_equal(moved[k], q[k])
        k = by[f"first{a}"]
        assert np.isfinite(phi[k]) and abs(phi[k] - true[k]) <= tol
        k = by[f"before{a}"]
        assert phi[k] == np.inf and not hit[k]
    for name in ("nan", "+inf", "-inf", "mixed"):
        k = by[name]
        assert phi[k] == np.inf and not hit[k]
        assert np.array_equal(moved[k], q[k], equal_nan=True)
    k = by["corner"]                                                   # the far corner node itself
    assert abs(phi[k] - true[k]) <= tol
    assert hit.any() and (~hit).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_constant_lattice_below_the_margin_never_hits(dtype):
    """len == 0: there is no direction to leave by"""
    lat = CR.Lattice(np.full((4, 3, 5), -7.0), (0, 0, 0), 300.0, 13.5, dtype)
    fr = CR.frame(CR.SCALE, (0, 0, 0), (1000, 1000, 1000), dtype)
    pts = np.random.default_rng(0).random((500, 3)) * 590.0
    phi, moved, hit = CR.sample(lat, fr, pts)
    assert np.all(phi == dtype(-7.0)) and not hit.any()
    assert np.array_equal(moved, pts.astype(dtype) / fr[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_box_wins_over_the_collider(dtype):
    """a plane that pushes out of the box: the second clamp puts the particle on the image of the face"""
    origin, spacing, dims = (-50.0, -50.0, -50.0), 100.0, (12, 12, 12)
    phi = CR.lattice_of(lambda x: 950.0 - x[..., 0], origin, spacing, dims)      # solid: x > 950, pushes towards -x ... margin 1000
    lat = CR.Lattice(phi, origin, spacing, 1000.0, dtype)
    fr = CR.frame(CR.SCALE, (0, 0, 0), (1000, 1000, 1000), dtype)
    _, moved, hit = CR.sample(lat, fr, np.array([[500.0, 500.0, 500.0]]))
    assert hit[0] and moved[0, 0] == fr[1][0] / fr[0] and CR.on_face(fr, moved)[0]


# ---- (d) the helpers ----------------------------------------------------------------------------------------------------
def test_sdf_helpers_hand_values(pkg):
    s = pkg.sdf_sphere((1.0, 2.0, 3.0), 2.0)
    assert s(np.array([1.0, 2.0, 3.0])) == -2.0 and s(np.array([4.0, 2.0, 3.0])) == 1.0 and s(np.array([1.0, 0.0, 3.0])) == 0.0
    b = pkg.sdf_box((0.0, 0.0, 0.0), (2.0, 4.0, 6.0))
    assert b(np.array([1.0, 2.0, 3.0])) == -1.0                        # the centre: the nearest faces are x = 0 and x = 2
    assert b(np.array([1.0, 3.5, 3.0])) == -0.5
    assert b(np.array([5.0, 2.0, 3.0])) == 3.0                         # beyond a face
    assert b(np.array([5.0, 8.0, 3.0])) == 5.0                         # beyond an edge: (3, 4, 0)
    assert b(np.array([2.0, 4.0, 6.0])) == 0.0
    p = pkg.sdf_plane((0.0, -2.0, 0.0), -5.0)                          # solid: y > 5
    assert p(np.array([0.0, 5.0, 0.0])) == 0.0 and p(np.array([9.0, 7.0, 1.0])) == -2.0 and p(np.array([0.0, 0.0, 0.0])) == 5.0
    lat = pkg.sdf_lattice(p, (1.0, 2.0, 3.0), 0.5, (2, 3, 4))
    assert lat.shape == (2, 3, 4) and lat.dtype == np.float64 and lat.flags["C_CONTIGUOUS"]
    assert lat[1, 2, 3] == 5.0 - 3.0 and lat[0, 0, 0] == 3.0
    # the index order is pbf_sample_lattice's: node (i, j, k) at (i * dims[1] + j) * dims[2] + k
    x = pkg.sdf_lattice(lambda v: v[..., 0] * 100 + v[..., 1] * 10 + v[..., 2], (0, 0, 0), 1.0, (2, 3, 4))
    assert x.reshape(-1)[(1 * 3 + 2) * 4 + 3] == 123.0
    # union and complement
    bowl = pkg.sdf_lattice(lambda v: np.minimum(-s(v), p(v)), (0, 0, 0), 1.0, (3, 3, 3))
    assert bowl[1, 2, 2] == min(-s(np.array([1.0, 2.0, 2.0])), p(np.array([1.0, 2.0, 2.0])))
    assert np.array_equal(CR.lattice_of(p, (1.0, 2.0, 3.0), 0.5, (2, 3, 4)), lat)   # the test-side twin of sdf_lattice


# ---- the GPU physics scenes' preconditions, on a float64 all-pairs step ----------------------------------------------------
def all_pairs_run(steps, lat, iteration=4):
    """the block scene under tests/nversion.py's stages (float64, all pairs, cells fixed at predict time), the collider applied
    after delta-p's clamp as DeltaOp::end does -> list of pStar (solver frame) after every step"""
    sc = CR.block_scene()
    pos, vel, mass = sc["pos"].astype(np.float64), sc["vel"].astype(np.float64), sc["mass"].astype(np.float64)
    fr = CR.frame(CR.SCALE, (0, 0, 0), (1000, 1000, 1000), np.float64)
    h, dt, lo, hi = 0.1, 0.0083 * np.float32(1.5), [0.0] * 3, [1000.0] * 3
    out = []
    for _ in range(steps):
        vel, ps = NV.predict(pos, vel, mass, dt, CR.SCALE, (0.0, 9.8, 0.0))
        cells = NV.predict_cells(ps, h, CR.SCALE, lo)
        for _ in range(iteration):
            lam, _ = NV.lambdas(ps, mass, h, None, cells)
            ps, _ = NV.delta(ps, lam, h, CR.SCALE, lo, hi, None, cells)
            if lat is not None:
                _, ps, _ = CR.project(lat, fr, ps)
        pos, vel = NV.finalise(ps, pos, vel, dt, CR.SCALE)
        out.append(ps)
    return out, fr


def test_block_on_plane_scene_meets_its_preconditions():
    """the scene of test_collider_gpu's physics test: with the collider no particle is on a box face and every one stays on the
    fluid side of the plane within (a)'s bar; without it the block falls below the plane by more than a cell"""
    lat, _ = CR.plane_case(np.float64, CR.BLOCK_PLANE_D, **CR.BLOCK_LATTICE)
    bar = CR.plane_bar_world(np.float64)
    with_, fr = all_pairs_run(CR.BLOCK_STEPS, lat)
    touched = False
    for ps in with_:
        assert not CR.on_face(fr, ps).any()
        phi = CR.plane_phi(CR.PLANE_N, CR.BLOCK_PLANE_D, ps * CR.SCALE)
        assert phi.min() >= CR.MARGIN - bar, phi.min()
        touched |= bool((phi < CR.MARGIN + 1.0).any())
    assert touched                                                     # the block does reach the plane within the run
    without, _ = all_pairs_run(CR.BLOCK_STEPS, None)
    phi = CR.plane_phi(CR.PLANE_N, CR.BLOCK_PLANE_D, without[-1] * CR.SCALE)
    print(f"without the collider the lowest particle ends at phi = {phi.min():.1f} world units (a cell is {0.1 * CR.SCALE:.0f})")
    assert phi.min() < -0.1 * CR.SCALE
