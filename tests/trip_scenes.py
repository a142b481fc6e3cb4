"""Scenes that take the loops of the single-workgroup scans and selects beyond their first trip, shared by the CPU file
that checks the scenes (tests/test_scan_trips_cpu.py) and the GPU files that use them, with the checks themselves:

  k_slab_scan            64 tiles a trip    pbf_slab_step on a rank of more than 64 x 1024 array slots     box102400, 3 ranks
  k_slab_arrival_ghosts  256 arrivals       more than 256 arrivals, a boundary-column one behind the 256th  (the same run)
  k_sel_scan             256 tiles a trip   pbf_slab_migrate / pbf_slab_ghosts on more than 262 144 slots   box286720, 2 ranks
  k_drain_scan           256 tiles a trip   pbf_set_drains on 263 245 particles                             drain_scene
  k_sort_big_cells       64 workgroups      66 (67) cells of more than 2 048 members                        piles_scene

Everything is built from fixed seeds in float64 and cast: the same particles on every rank and engine."""
import numpy as np

CELL = 50.0                      # world units per cell: h * scale
SEL_TILE = DRAIN_TILE = 1024     # csrc/pbf_slab.hpp, csrc/pbf_kernels.hpp
BIG_CELL = 2048                  # csrc/pbf_kernels.hpp
SORT_GROUPS = 64                 # workgroups of k_sort_big_cells (csrc/pbf_hip.hip stage_sort)

# ---- boxN: the slab worker's moving scene -------------------------------------------------------------------------------
PER_CELL, BOX_NY, BOX_NZ = 20, 16, 16


def box_shape(n):
    """(cells along x, box side): a box of nx x 16 x 16 cells holds n particles at about 20 per cell; the bounds are the cube
    of the box's length"""
    nx = -(-int(n) // (PER_CELL * BOX_NY * BOX_NZ))
    assert BOX_NY <= nx <= 1000, n
    return nx, nx * CELL


def box_scene(n, fp64=False, seed=20):
    """n particles uniform at random in [0, nx] x [0, 16] x [0, 16] cells; velocities as random_box of
    tests/test_sort_slots_gpu.py has them (a step moves a particle by 6.2 v world units, v uniform in +-2: about a third
    change cell per step); random colours; ids are the source indices.  Returns (particles, box side)."""
    nx, side = box_shape(n)
    rng = np.random.default_rng(seed)
    dt = np.float64 if fp64 else np.float32
    pos = rng.uniform(0.0, 1.0, (n, 3)) * (nx * CELL, BOX_NY * CELL, BOX_NZ * CELL)
    vel = rng.uniform(-2.0, 2.0, (n, 3))
    colour = rng.uniform(0.0, 1.0, (n, 4))
    return dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n, dt), pos=pos.astype(dt),
                vel=vel.astype(dt), colour=colour.astype(dt)), side


# pbf_slab_step, three ranks: the box's 20 columns are the grid's 2 .. 21; the middle rank owns 14 of them (71 680 particles
# = 70 tiles), the outer ranks three each
STEP_SCENE, STEP_CUTS, STEP_WORLD = "box102400", "c:5,19", 3
STEP_SLOTS = 66 * SEL_TILE       # the middle rank holds at least that many array slots when a step begins
STEP_EDGE = 64 * SEL_TILE        # first array index of k_slab_scan's second trip
ARRIVAL_TRIP = 256               # arrivals per trip of k_slab_arrival_ghosts
# the staged API, two ranks: 56 columns (2 .. 57), rank 0 owns 53 of them (271 360 particles = 265 tiles)
STAGED_SCENE, STAGED_CUTS, STAGED_WORLD = "box286720", "c:55", 2
STAGED_SLOTS = 258 * SEL_TILE
STAGED_EDGE = 256 * SEL_TILE     # first array index of k_sel_scan's second trip

TRACE_KEYS = ("slots", "n_migrate", "top_left", "top_right", "top_keep", "slot_left", "slot_right", "n_ghosts",
              "top_copy_left", "top_copy_right", "slot_copy_left", "slot_copy_right", "arrivals", "top_arrival_copy")


def check_step_trips(ranks, steps):
    """the CPU twin's counters (slab_worker --trace, tests/slab_engines.py) of the three-rank run: in every step the middle
    rank's k_slab_scan runs a second trip in which all four classes have something to place; in at least one step
    k_slab_arrival_ghosts runs a second trip with a copy to write"""
    mid = ranks[1]
    assert all(len(mid["trace_" + k]) == steps for k in TRACE_KEYS)
    for s in range(steps):
        assert int(mid["trace_slots"][s]) >= STEP_SLOTS, (s, int(mid["trace_slots"][s]))
        for k in ("slot_left", "slot_right", "slot_copy_left", "slot_copy_right"):
            assert int(mid["trace_" + k][s]) >= STEP_EDGE, (s, k, int(mid["trace_" + k][s]))
    late = [s for s in range(steps) if int(mid["trace_arrivals"][s]) > ARRIVAL_TRIP and
            int(mid["trace_top_arrival_copy"][s]) >= ARRIVAL_TRIP]
    assert late, (mid["trace_arrivals"], mid["trace_top_arrival_copy"])
    for r in (0, 2):  # the outer ranks stay small: one trip
        assert int(ranks[r]["trace_slots"].max()) < STEP_EDGE


def check_staged_trips(ranks, steps):
    """the same for the staged API's two selects on rank 0: migrants to the neighbour, stayers and boundary-column copies at
    array indices of k_sel_scan's second trip"""
    big = ranks[0]
    for s in range(steps):
        assert int(big["trace_n_migrate"][s]) >= STAGED_SLOTS and int(big["trace_n_ghosts"][s]) >= STAGED_SLOTS, s
        for k in ("top_right", "top_keep", "top_copy_right"):
            assert int(big["trace_" + k][s]) >= STAGED_EDGE, (s, k, int(big["trace_" + k][s]))
    assert int(ranks[1]["trace_n_migrate"].max()) < STAGED_EDGE


# ---- drains on 256 + 1 + a partial tile ---------------------------------------------------------------------------------
DRAIN_N = 256 * DRAIN_TILE + DRAIN_TILE + 77
DRAIN_EDGE = 256 * DRAIN_TILE    # first source index of k_drain_scan's second trip
DRAIN_LAST = 257 * DRAIN_TILE    # first source index of the last, partial tile
DRAIN_SIDE = 1500.0
DRAINS_MIXED = [((400.0, 500.0, 600.0), 420.0), ((1000.0, 900.0, 800.0), 380.0)]
DRAINS_SECOND = [((750.0, 750.0, 750.0), 520.0)]       # for the Z-sorted set behind a step
DRAINS_NOWHERE = [((-5000.0, -5000.0, -5000.0), 10.0)]
DRAINS_ALL = [((750.0, 750.0, 750.0), 1.0e5)]
# a sheet of 20 x 20 particles, 25 apart, around (750, 200, 750); the first drain takes the corner at (500, 200, 500)
SHEET_SOURCES = [(900001, (750.0, 200.0, 750.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0, 1.0), 400.0)]
SHEET_DRAINS = [((500.0, 200.0, 500.0), 150.0), DRAINS_MIXED[0]]
SHEET_COUNT = 400


def drain_scene(fp64=False, seed=31):
    """263 245 particles uniform at random in the bounds, in that (upload) order; every 50th is an obstacle, so every tile
    holds both kinds"""
    n = DRAIN_N
    rng = np.random.default_rng(seed)
    dt = np.float64 if fp64 else np.float32
    pos = rng.uniform(0.0, DRAIN_SIDE, (n, 3))
    vel = rng.uniform(-2.0, 2.0, (n, 3))
    colour = rng.uniform(0.0, 1.0, (n, 4))
    kind = (np.arange(n) % 50 == 17).astype(np.uint8)
    return dict(id=np.arange(n, dtype=np.uint64), type=kind, mass=np.ones(n, dt), pos=pos.astype(dt), vel=vel.astype(dt),
                colour=colour.astype(dt))


def check_drain_trips(sc, want):
    """`want` = the reference's survivors of the upload-order scene `sc` (ids are the source indices): between 5 % and 50 %
    of the fluid left; drained particles and survivors both beyond the first trip's tiles and both in the last tile"""
    fluid = sc["type"] == 0
    kept = np.zeros(len(sc["id"]), bool)
    kept[want["id"].astype(np.int64)] = True
    assert kept[~fluid].all()
    gone = fluid & ~kept
    assert 0.05 < gone.sum() / fluid.sum() < 0.5, gone.sum() / fluid.sum()
    for lo in (DRAIN_EDGE, DRAIN_LAST):
        assert gone[lo:].any() and (kept & fluid)[lo:].any(), lo


# ---- more pile-ups than sorting workgroups ------------------------------------------------------------------------------
PILES, PILE_SIDE = SORT_GROUPS + 2, 500.0     # bounds of 10 cells + 2 cells of padding on either side: 14 cells per axis
PILE_TABLE_N = 4088                           # morton(14, 14, 14)


def pile_cell_of(pos):
    return np.floor(np.asarray(pos, np.float64) / CELL + 2.0).astype(np.int64)


def piles_scene(overflow=False, seed=66):
    """66 cells of BIG_CELL + 1 members each — no two of them neighbours (every second cell of the bounds' 10^3), so that a
    whole step stays cheap on the CPU — plus 500 particles elsewhere in the bounds, plus (overflow) BIG_CELL + 52 particles
    outside the table, along x, with many keys; in a random upload order, at rest"""
    rng = np.random.default_rng(seed)
    lattice = np.stack(np.meshgrid(*[np.arange(2, 12, 2)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)   # 125 cells
    cells = lattice[rng.permutation(len(lattice))[:PILES]]
    piles = ((cells[:, None, :] - 2) * CELL + rng.uniform(5.0, 45.0, (PILES, BIG_CELL + 1, 3))).reshape(-1, 3)
    rest = rng.uniform(0.0, PILE_SIDE, (1200, 3))
    taken = {tuple(c) for c in cells}
    rest = rest[[tuple(c) not in taken for c in pile_cell_of(rest)]][:500]
    assert len(rest) == 500
    parts = [piles, rest]
    if overflow:  # cells 16 .. 23 along x: a key above PILE_TABLE_N whatever y and z are
        m = BIG_CELL + 52
        parts.append(np.stack([rng.uniform(14 * CELL, 22 * CELL, m), rng.uniform(0.0, PILE_SIDE, m),
                               rng.uniform(0.0, PILE_SIDE, m)], axis=1))
    pos = np.concatenate(parts)
    pos = pos[rng.permutation(len(pos))]
    n = len(pos)
    return dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n, np.float32),
                pos=pos.astype(np.float32), vel=np.zeros((n, 3), np.float32),
                colour=rng.uniform(0.0, 1.0, (n, 4)).astype(np.float32))


def check_pile_trips(keys, overflow):
    """`keys` = the oracle's keys of the scene: more listed cells than k_sort_big_cells has workgroups"""
    keys = np.asarray(keys).astype(np.int64)
    _, members = np.unique(keys[keys < PILE_TABLE_N], return_counts=True)
    assert int((members > BIG_CELL).sum()) == PILES > SORT_GROUPS
    outside = keys[keys >= PILE_TABLE_N]
    if overflow:
        assert len(outside) > BIG_CELL and len(np.unique(outside)) >= 5
    else:
        assert len(outside) == 0
