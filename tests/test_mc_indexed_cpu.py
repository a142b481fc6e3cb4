"""The indexed marching-cubes mesh, without a GPU: the checker (tests/mc_indexed_ref.py) against the oracle's triangle
soup, closed forms that share no reading with the checker, and the library's new entry points.

The bound on negative-oriented cube edges (2, 3, 6, 7), derived from rounding counts
-----------------------------------------------------------------------------------
A lattice edge with end values a (lower node) and b (+axis node) and field values v_a, v_b.  The indexed mesh computes
    w  = fl((iso - v_a) / (v_b - v_a)),   r  = fl(fl(a * fl(1 - w))  + fl(b * w)),
the soup, on a cube edge that runs against the axis, starts from the other end:
    w' = fl((iso - v_b) / (v_a - v_b)),   r' = fl(fl(b * fl(1 - w')) + fl(a * w')).
u is the unit roundoff (2^-24, 2^-53), M(x) = a (1 - x) + b x the exact mix.

 1. r against M(w): four roundings, fl(1 - w), the two products and the sum; the a term carries three of them, the b term
    two.  |r - M(w)| <= 3u |a| |1 - w| + 2u |b| |w| <= 3u max(|a|, |b|) (|1 - w| + |w|), and |1 - w| + |w| = 1 for w in
    [0, 1].  Likewise |r' - M(1 - w')| <= 3u max(|a|, |b|), because b (1 - w') + a w' = M(1 - w').
 2. The weights: W = (iso - v_a) / (v_b - v_a) and W' = 1 - W exactly, both in [0, 1] on a crossed edge.  w and w' carry
    three roundings each (numerator, denominator, quotient): w = W (1 + t), w' = W' (1 + t'), |t|, |t'| <= 3u.  So
    w - (1 - w') = W t + W' t', at most 3u (W + W') = 3u in magnitude, and |M(w) - M(1 - w')| = |b - a| |w - (1 - w')|
    <= 3u |b - a|.
 3. Together: |r - r'| <= 6u max(|a|, |b|) + 3u |b - a|.
 4. Second order: (1 + u)^3 - 1 <= 3u (1 + 2u) in steps 1 and 2, and w may exceed 1 by 3u (1 + 2u), so that
    |1 - w| + |w| <= 1 + 6u (1 + 2u): a factor (1 + 10u) covers all of it.
 5. Underflow: sums and differences are exact when they underflow; a quotient or a product that does is off by at most
    half the smallest subnormal eta.  w's or w''s enters times |b - a|, the products' directly:
    + eta (|b - a| + 2).

    bound = (6u max(|a|, |b|) + 3u |b - a|) (1 + 10u) + eta (|b - a| + 2)

Nothing in it is fitted.  Largest observed |r - r'| / bound on the oracle's lattices (this file, printed per case):
0.56 in fp32 (faces, resolution 3) and 0.62 in fp64 (faces resolution 3, cloud resolution 2) over the 46 cases below;
the test asserts <= 1.

A field value that is not finite (a particle exactly on a node: size / 0) voids step 2; the three such vertices of the
on_node scene are held bit for bit instead (mc_indexed_ref.compare_with_soup).
"""
import ctypes
import os

import numpy as np
import pytest

import mc_closed_forms as CF
import mc_indexed_ref as R
import mc_scenes as M
import oracle_lib as O
from test_mc_nversion_cpu import oracle_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STOCK = dict(h=0.1, scale=500.0, min_bound=(0.0,) * 3)


def run_checker(m, s, mc, fp64):
    """The checker on the lattice of an oracle / device surface dict `m` -> (indexed dict, consts)."""
    dtype = np.float64 if fp64 else np.float32
    consts = R.grid_constants(s["h"], s["scale"], s["min_bound"], mc[0], dtype)
    assert m["pn"].dtype == dtype
    return R.extract(m["sample"], m["pn"], m["c"], *consts, mc[1]), consts


def straddling_edges(sample, v, iso):
    """Lattice edges whose end values straddle the isolevel, counted directly from the field values."""
    f = (v < v.dtype.type(iso)).reshape([int(x) for x in sample])
    return int((f[1:] != f[:-1]).sum() + (f[:, 1:] != f[:, :-1]).sum() + (f[:, :, 1:] != f[:, :, :-1]).sum())


def check_against_soup(m, s, mc, fp64, label):
    ix, consts = run_checker(m, s, mc, fp64)
    rep = R.compare_with_soup(ix, m, (m["sample"], m["pn"], m["c"]), consts, mc[1])
    print(f"{label}: V={len(ix['vs'])} T={len(ix['tris'])} vertices on +edges {rep['n_pos']}, on -edges {rep['n_neg']} "
          f"(+ {rep['n_inf']} at an infinite field value, held bit for bit), largest error / bound {rep['worst']:.3f}")
    assert rep["n_pos"] + rep["n_neg"] + rep["n_inf"] == len(m["vs"]) > 0        # no vertex left out
    assert rep["n_neg"] > 0 and rep["n_pos"] > 0
    # closed forms that do not read the checker's edge set
    assert len(ix["vs"]) == straddling_edges(m["sample"], m["pn"][:, 0], mc[1])
    assert np.unique(ix["tris"]).size == len(ix["vs"])            # no orphan vertices
    return ix, rep


@pytest.mark.parametrize("fp64", [False, True])
def test_checker_vs_oracle_soup_cubes(oracle, fp64):
    sc = oracle.scene_cubes(2048, fp64)
    o = oracle.Oracle(fp64)
    o.set_particles(**sc)
    p = oracle.make_params(threads=4)
    for _ in range(3):
        o.step(p)
    mc = (2.0, 100.0, 25.0, 0.5)
    m = o.surface(p, oracle.OracleMc(*mc))
    assert np.isfinite(m["vs"]).all() and np.isfinite(m["ns"]).all() and np.isfinite(m["cs"]).all()
    ix, rep = check_against_soup(m, STOCK, mc, fp64, f"cubes {'f64' if fp64 else 'f32'}")
    assert len(ix["tris"]) > 2000


CASES = [(n, mc, fp64) for n in M.NAMES for mc in M.PARAMS[n] for fp64 in (False, True)]


@pytest.mark.parametrize("name,mc,fp64", CASES, ids=[f"{n}-{mc[0]}-{mc[3]}-{'f64' if d else 'f32'}" for n, mc, d in CASES])
def test_checker_vs_oracle_soup_scenes(name, mc, fp64):
    s, o, q, st, cells = oracle_state(name, fp64)
    m = o.surface(q, O.OracleMc(*mc))
    check_against_soup(m, s, mc, fp64, f"{name} {mc} {'f64' if fp64 else 'f32'}")


def one_particle(fp64):
    dtype = np.float64 if fp64 else np.float32
    s = dict(CF.ONE, sc=CF._particle(CF.ONE_POS))
    o = O.Oracle(fp64, device_pow=True)
    o.set_particles(**M.cast(s["sc"], dtype))
    q = M.oracle_params(s, threads=2)
    o.step(q)
    return s, o.surface(q, O.OracleMc(*CF.ONE_MC))


def assert_closed_manifold(tris, nv):
    """Every undirected edge in exactly two triangles, once per direction, by index; -> Euler characteristic."""
    bad, edges = R.directed_edge_defects(tris)
    assert bad == 0 and edges > 0, (bad, edges)
    assert 2 * edges == 3 * len(tris)
    return nv - edges + len(tris)


@pytest.mark.parametrize("fp64", [False, True])
def test_one_particle_sphere_is_a_sphere_by_index(oracle, fp64):
    s, m = one_particle(fp64)
    ix, rep = check_against_soup(m, s, CF.ONE_MC, fp64, f"one particle {'f64' if fp64 else 'f32'}")
    chi = assert_closed_manifold(ix["tris"], len(ix["vs"]))
    assert chi == 2, chi                                          # V - E + F = 2


@pytest.mark.parametrize("fp64", [False, True])
def test_blob_inside_the_lattice_is_closed_by_index(fp64):
    mc = M.PARAMS["blob"][0]
    s, o, q, st, cells = oracle_state("blob", fp64)
    m = o.surface(q, O.OracleMc(*mc))
    # well inside: no crossed edge touches the lattice's boundary planes
    ix, _ = run_checker(m, s, mc, fp64)
    smp = np.array([int(v) for v in m["sample"]])
    xyz = np.stack([ix["owner"] // (smp[1] * smp[2]), (ix["owner"] // smp[2]) % smp[1], ix["owner"] % smp[2]], 1)
    assert (xyz >= 1).all() and (xyz + 1 < smp - 1).all()
    v, t = len(ix["vs"]), len(ix["tris"])
    chi = assert_closed_manifold(ix["tris"], v)
    assert t % 2 == 0 and v == t // 2 + chi                       # V = T / 2 + chi, chi an integer
    print(f"blob {'f64' if fp64 else 'f32'}: V={v} T={t} chi={chi}; bytes 40V+12T={40 * v + 12 * t} vs 120T={120 * t} (fp32 sizes)")


def test_library_exports_indexed_entry_points(pkg):
    names = ("pbf_surface_indexed", "pbf_download_mesh_indexed", "pbf_map_mesh_indexed")
    from pbf_sph_amd import capi
    L = ctypes.CDLL(pkg.LIB_PATH)
    for n in names:
        assert hasattr(L, n), n
        assert n in capi.exported_symbols(), n
    header = open(os.path.join(ROOT, "include", "pbf_hip.h")).read()
    for n in names:
        assert f"int {n}(" in header
