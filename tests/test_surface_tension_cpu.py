"""CPU checks of the surface-tension restatement (tests/surface_tension_ref.py) and of the new C-ABI entry: the kernels'
shapes, a two-particle closed form, momentum conservation, and that pbf_set_surface_tension is exported and bound."""
import numpy as np
import pytest

import nversion as NV
import surface_tension_ref as ST

H = 0.1


def test_cohesion_kernel_shape():
    assert ST.cohesion_kernel(H, H) == 0.0                       # C(h) = 0
    assert ST.cohesion_kernel(1.0001 * H, H) == 0.0
    eps = 1e-9
    lo, hi = float(ST.cohesion_kernel(H / 2 - eps, H)), float(ST.cohesion_kernel(H / 2 + eps, H))
    peak = float(ST.cohesion_kernel(H / 2, H))
    assert abs(lo - hi) <= 1e-6 * peak                           # continuous at h/2
    assert ST.cohesion_kernel(0.01 * H, H) < 0.0                 # repulsive near 0
    assert ST.cohesion_kernel(0.2 * H, H) < 0.0
    assert ST.cohesion_kernel(0.4 * H, H) > 0.0                  # (the sign changes at r ~ 0.27 h, not at h/2)
    r = np.linspace(0.51 * H, H, 200)
    assert (ST.cohesion_kernel(r, H) >= 0.0).all()


def test_adhesion_kernel_shape():
    r = np.linspace(0.0, 1.2 * H, 12001)
    a = ST.adhesion_kernel(r, H)
    assert (a[(r <= H / 2) | (r > H)] == 0.0).all()              # zero outside (h/2, h]
    inside = (r > H / 2) & (r <= H)
    assert (a[inside & (r < H)] > 0.0).all()
    assert abs(r[np.argmax(a)] - 0.75 * H) <= 1e-4 * H             # maximum at 3h/4
    # closed form of the peak: (-4 (3h/4)^2 / h + 6 (3h/4) - 2h)^(1/4) = (h/4)^(1/4)
    assert np.isclose(float(ST.adhesion_kernel(0.75 * H, H)), 0.007 / H ** 3.25 * (H / 4) ** 0.25, rtol=1e-14)


@pytest.mark.parametrize("r", [0.02, 0.054, 0.07, 0.09])
def test_two_particles_match_the_closed_form(r):
    ps = np.array([[0.5, 0.5, 0.5], [0.5 + r, 0.5, 0.5]])
    mass = np.array([1.3, 1.3])
    dt, gamma = 0.01, 0.7
    dv, rho, nrm = ST.delta_v(ps, mass, H, dt, gamma, 0.0)
    w = ST.two_particle_dv(r, H, 1.3, dt, gamma)
    towards = np.array([1.0, 0.0, 0.0])                          # particle 0 -> particle 1
    assert np.allclose(dv[0], w * towards, rtol=1e-12, atol=0) and np.allclose(dv[1], -w * towards, rtol=1e-12, atol=0)
    assert np.allclose(rho, 1.3 * (NV.poly6(np.array(0.0), H) + NV.poly6(np.array(r), H)), rtol=1e-14)
    assert np.allclose(nrm[0], -nrm[1], rtol=1e-14)
    assert nrm[0, 0] > 0.0                                       # the normal of particle 0 points at particle 1
    # attraction beyond the zero of C (plus the always-repulsive curvature term of a pair), repulsion close in
    assert (w > 0.0) == (r > 0.05)


def test_fluid_cloud_conserves_momentum():
    """With equal masses every pair term is antisymmetric (K_ij = K_ji, C x_ij / r and n_i - n_j flip sign)."""
    rng = np.random.default_rng(5)
    ps = rng.random((300, 3)) * 0.35
    mass = np.full(300, 0.8)
    dv, _, _ = ST.delta_v(ps, mass, H, 0.0125, 0.3, 0.0)
    mom = (mass[:, None] * dv).sum(0)
    assert np.abs(dv).max() > 0.0
    assert np.abs(mom).max() <= 1e-12 * np.abs(mass[:, None] * dv).sum()


def test_adhesion_pulls_fluid_towards_an_obstacle():
    ps = np.array([[0.5, 0.5, 0.5], [0.5 + 0.07, 0.5, 0.5]])
    dv, rho, nrm = ST.delta_v(ps, np.array([1.0, 2.0]), H, 0.01, 0.0, 0.5, obstacle=np.array([False, True]))
    assert dv[0, 0] > 0.0 and dv[0, 1] == 0.0 and dv[0, 2] == 0.0
    assert (dv[1] == 0.0).all() and rho[1] == 0.0 and (nrm[1] == 0.0).all()
    assert np.isclose(dv[0, 0], 0.01 * 0.5 * 2.0 * float(ST.adhesion_kernel(0.07, H)), rtol=1e-12)


def test_set_surface_tension_is_exported_and_bound():
    from conftest import load_package

    pkg = load_package()
    from pbf_sph_amd import capi

    assert "pbf_set_surface_tension" in capi.exported_symbols()
    assert hasattr(capi.Solver, "set_surface_tension") and hasattr(capi.Solver, "surface_state")
    assert hasattr(pkg.Solver, "set_surface_tension")
