"""Scenes of the composed-solids tests (tests/test_solids_scene_gpu.py, tests/test_solids_extras_gpu.py), shared with their
CPU companion tests/test_solids_composed_cpu.py: scene_cases.main_scene with one inlet born inside the collider's margin shell
and one drain over the surface the collider projects the fluid onto, the collider's plane, the scenery's wall, and the host
arithmetic of the counts.  Everything here is geometry in float64 and numpy; nothing needs a device."""
import numpy as np

import collider_pose_ref as PR
import collider_ref as CR
import scene_cases as S

SHARE = 0.3                                  # of the fluid starts below the collider's plane (phi < margin)
WALL_N, WALL_SHARE = (-0.9, 0.1, 0.3), 0.1   # the scenery: a wall across the collider's plane that a tenth of the fluid starts behind
FRAMES, RESERVE = 6, 4096
SHEET_PHI = 1.5                              # the moved inlet's sheet: its middle this far outside the solid, inside the shell
INLET_XZ, OUTLET_XZ, OUTLET_WIDTH = (300.0, 300.0), (200.0, 200.0), 25.0
TILE = 1024                                  # particles per partial record of k_wrench_partial / k_collider_friction (DIAG_TILE)


def unit(n):
    n = np.asarray(n, np.float64)
    return n / np.sqrt((n * n).sum())


def fluid_positions(sc):
    return sc["pos"][sc["type"] == 0].astype(np.float64)


def plane_d(sc, share=SHARE, normal=CR.PLANE_N):
    """the d of test_collider_pose_gpu.body_lattice_through's world plane: `share` of the fluid starts with phi < margin"""
    return float(np.quantile(CR.plane_phi(normal, 0.0, fluid_positions(sc)), share)) - CR.MARGIN


def on_plane(sc, xz, phi):
    """the world point over (x, z) at the signed distance phi from the collider's plane"""
    n, d = unit(CR.PLANE_N), plane_d(sc)
    return (float(xz[0]), float((d + phi - n[0] * xz[0] - n[2] * xz[1]) / n[1]), float(xz[1]))


def sheet(source, h=S.H, scale=S.SCALE):
    """float64 world positions of one source's sheet (scene_cases.np_emit's, ompsph.hpp:93-105)"""
    _, centre, _, _, rate = source
    empty = {k: np.zeros((0,) + s, t) for k, s, t in (("id", (), np.uint64), ("type", (), np.uint8), ("mass", (), np.float64),
                                                      ("pos", (3,), np.float64), ("vel", (3,), np.float64), ("colour", (4,), np.float64))}
    return S.np_emit(empty, [source], np.float64, h, scale)["pos"]


def composed_scene(sc):
    """main_scene with two changes: the first inlet stands where its 4 x 4 sheet is born inside the collider's margin shell
    (the sheet is 75 wide and the plane tilted, so its middle is placed SHEET_PHI outside the solid), and the wide drain
    becomes a smaller one centred on the surface phi = margin, where the first projection leaves what it pushed"""
    sources, drains = S.main_scene(sc)
    tag, _, velocity, colour, rate = sources[0]
    half = 0.25 * S.H * S.SCALE                                # the sheet's middle lies half a spacing before its centre
    y = on_plane(sc, (INLET_XZ[0] - half, INLET_XZ[1] - half), SHEET_PHI)[1]
    sources = [(tag, (INLET_XZ[0], y, INLET_XZ[1]), velocity, colour, rate), sources[1]]
    drains = [(on_plane(sc, OUTLET_XZ, CR.MARGIN + 10.0), OUTLET_WIDTH), drains[1]]
    return sources, drains


def emitted_per_frame(sources):
    """host arithmetic (pbf_set_sources): floor(sqrt(rate)) x ceil(sqrt(rate)) per source"""
    return sum(int(np.floor(np.sqrt(r))) * int(np.ceil(np.sqrt(r))) for *_, r in sources)


def records(n):
    """partial records a pass over n particles writes: (n + 1023) / 1024"""
    return (int(n) + TILE - 1) // TILE


def depletion_scene(dtype):
    """no obstacle particle: a 9 x 9 x 9 block at rest spacing that the collider's plane passes through"""
    k = 9
    g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3)
    n = len(g)
    return dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n, dtype), pos=(g * 27.0 + 392.0).astype(dtype),
                vel=np.zeros((n, 3), dtype), colour=np.full((n, 4), 0.5, dtype))


def shrinking_scene(sc, dtype):
    """the drains-only sub-case: the scene's particles and 60 more fluid particles in a corner that neither solid reaches
    (low x: outside the wall; low y: above the collider's plane), so that the count starts above 2 x 1024 — 2 060 — and a drain
    around them carries it below -> (the particles, the drains: the corner's and the outlet)"""
    g = np.stack(np.meshgrid(np.arange(5), np.arange(3), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    n = len(g)
    extra = dict(id=np.arange(n, dtype=np.uint64) + 500000, type=np.zeros(n, np.uint8), mass=np.ones(n, dtype),
                 pos=(g * 27.0 + np.array([120.0, 20.0, 850.0])).astype(dtype), vel=np.zeros((n, 3), dtype), colour=np.full((n, 4), 0.25, dtype))
    out = {k: np.concatenate([np.asarray(v).astype(extra[k].dtype), extra[k]]) for k, v in sc.items()}
    corner = ((174.0, 47.0, 890.5), 120.0)
    return out, [corner, composed_scene(sc)[1][0]]


# ---- the velocity passes with the solids on (tests/test_solids_extras_gpu.py) ---------------------------------------------------
# test_nversion_cpu.scene(name) -> the share of its fluid that starts below the collider's plane, as the friction tests choose it
EXTRAS_SHARE = {"cloud": 0.5, "obstacles_moving": 0.5, "edges65": 0.15}
# the solids act inside delta-p, so every scene runs two iterations here: edges65 too, whose own count in extras_ref.SCENES is none
EXTRAS_ITERATION = 2
