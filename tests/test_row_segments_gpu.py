"""The list of non-empty x-segments k_diffuse_rows works from is written by the row table's k_scan_apply (a segment is
1 << segShift <= 64 aligned cells of one row; non-empty = its populations do not sum to zero).  A segment left out loses
its particles' diffusion, one listed twice or wrongly diffuses twice or faults — either shows in the colours: compared bit for
bit after two steps, option row_diffuse 1 against 0 (k_diffuse_bricks, no segments) and both against the oracle.

  * a grid of 5 x 5 x 5 cells: the row cube has P = 8, a segment is a whole row (segShift = pshift = 3);
  * a grid of 2 x 2 x 2 cells (P = 4, segShift = 2): a lane of the apply pass holds more than one segment;
  * a grid of 100 x 4 x 4 cells: P = 128, two segments of 64 cells per row.  (The grid carries two cells of padding on
    either side of the box, so no axis has fewer than 4 cells: 100 x 4 x 4 is the narrowest grid with 100 cells along x.)
    The four rows of z = 0 hold particles in their second segment only; row (1, 1) holds cells 63 and 64 and nothing else — its first
    segment is occupied only in its last cell, its second only in its first; the other rows are filled at random;
  * the second scene again with obstacles in it: the typed path.

K = 0 solver iterations and no gravity: the occupancy is the test's, in both steps (delta-p would clamp the particles
into the box proper, one cell across); the random rows drift along x."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CELL = 50.0  # world units per cell: h * scale


def at_cells(cells, rng):
    """one particle somewhere inside each of the given cells (x, y, z)"""
    c = np.asarray(cells, np.float64)
    return (c - 2.0) * CELL + rng.uniform(5.0, 45.0, c.shape)


def make(pos, vel, rng, obstacles=False):
    n = len(pos)
    ty = np.zeros(n, np.uint8)
    if obstacles:
        ty[::7] = 1
    return dict(id=np.arange(n, dtype=np.uint64), type=ty, mass=np.ones(n, np.float32), pos=pos.astype(np.float32),
                vel=vel.astype(np.float32), colour=rng.uniform(0.0, 1.0, (n, 4)).astype(np.float32))


def small_cube():
    rng = np.random.default_rng(3)
    cells = rng.integers(0, 5, (400, 3))
    pos = at_cells(cells, rng)
    vel = rng.uniform(-2.0, 2.0, (400, 3))
    return make(pos, vel, rng), (60.0, 60.0, 60.0), (5, 5, 5)


def tiny_cube():
    """max_bound below min_bound by two cells: what is left of the grid is its padding, 2 x 2 x 2 cells"""
    rng = np.random.default_rng(9)
    cells = rng.integers(0, 2, (40, 3))
    return make(at_cells(cells, rng), rng.uniform(-1.0, 1.0, (40, 3)), rng), (-100.0, -100.0, -100.0), (2, 2, 2)


def long_rows(obstacles):
    rng = np.random.default_rng(5)
    cells, drift = [], []
    for z in range(4):
        for y in range(4):
            if z == 0:  # rows with an empty first segment
                xs = rng.integers(64, 100, 30)
            elif (y, z) == (1, 1):  # last cell of the first segment, first cell of the second, nothing else
                xs = np.array([63] * 3 + [64] * 4)
            else:
                xs = rng.integers(0, 100, 60)
            cells += [(x, y, z) for x in xs]
            drift += [0.0 if z == 0 or (y, z) == (1, 1) else 1.0] * len(xs)
    cells = np.array(cells)
    pos = at_cells(cells, rng)
    vel = np.zeros((len(cells), 3))
    vel[:, 0] = rng.uniform(-2.0, 2.0, len(cells)) * np.array(drift)  # along the row only; 0 where the pattern must hold
    order = rng.permutation(len(cells))
    return make(pos[order], vel[order], rng, obstacles), (4810.0, 10.0, 10.0), (100, 4, 4)


SCENES = {"cube2": tiny_cube, "cube5": small_cube, "rows100": lambda: long_rows(False), "rows100_typed": lambda: long_rows(True)}


@pytest.mark.parametrize("name", list(SCENES))
def test_row_segments_colours(pkg, oracle, name):
    sc, max_bound, extent = SCENES[name]()
    p = pkg.default_params(0, 1000.0)
    p.max_bound[:] = max_bound
    p.constant_force[:] = (0.0, 0.0, 0.0)
    q = oracle.make_params(iteration=0, max_bound=max_bound, force=(0.0, 0.0, 0.0), mode=oracle.JACOBI,
                           sort=oracle.SORT_STABLE)
    o = oracle.Oracle(False, device_pow=True)
    o.set_particles(**sc)
    got = {}
    for row_diffuse in (1, 0):
        s = pkg.Solver(h=0.1)
        s.set_option("row_diffuse", row_diffuse)
        s.upload(**sc)
        s.step(p)
        if row_diffuse:
            e, _ = s.extent()
            assert tuple(int(v) for v in e) == extent, e
        s.step(p)
        got[row_diffuse] = s.download()
    for _ in range(2):
        o.step(q)
    w = o.get_particles()
    assert not np.array_equal(np.sort(w["colour"], axis=0), np.sort(sc["colour"], axis=0))  # something diffused
    for k in ("id", "type", "colour", "pos", "vel"):
        assert np.array_equal(got[1][k], got[0][k]), (name, "row_diffuse 1 against 0", k)
        assert np.array_equal(got[1][k], w[k]), (name, "row_diffuse 1 against the oracle", k)
        assert np.array_equal(got[0][k], w[k]), (name, "row_diffuse 0 against the oracle", k)
    if name.startswith("rows100"):  # the pattern held in both steps (the second step's sort saw it too)
        cx, cy, cz = (np.floor(w["pos"].astype(np.float64) / CELL + 2.0).astype(np.int64)).T
        assert cx[cz == 0].min() >= 64
        assert sorted(set(cx[(cy == 1) & (cz == 1)])) == [63, 64]
