"""Scenes of the resident sources / drains / queries tests, shared by the CPU and the GPU file, and a numpy restatement
of emit and drain written from the reference's lines alone (src/omp/ompsph.hpp:93-118)."""
import numpy as np

RED, GREEN = (1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 1.0)
H, SCALE = 0.1, 500.0
GROWTH_FRAMES = 3   # sources only: 2000 + 3 x 28 crosses 2048 = 8 x 256 upwards


def cubes_with_obstacle(pkg, fp64=False):
    sc = {k: v.copy() for k, v in pkg.scene_cubes(2048, fp64).items()}
    sc["type"][7] = 1
    return sc


def shim_scene(sc):
    """sources, drain and query points of tests/test_cli_gpu.py::test_shim_scene_dynamics_vs_oracle"""
    sources = [(100777, (500, 300, 500), (0, 1, 0), RED, 16.0), (100888, (200, 700, 800), (3, 0, -2), GREEN, 10.0)]
    drains = [(tuple(float(v) for v in sc["pos"][7]), 60.0)]
    points = [tuple(float(v) for v in sc["pos"][100]), (990.0, 990.0, 990.0), (510.0, 310.0, 510.0)]
    return sources, drains, points


def main_scene(sc):
    """the issue's main scene: an inlet away from the fluid, one at its centre inside a small drain, a wide drain"""
    c = tuple(float(v) for v in sc["pos"].astype(np.float64).mean(axis=0))
    sources = [(100777, (500, 300, 500), (0, 1, 0), RED, 16.0), (100888, c, (3, 0, -2), GREEN, 10.0)]
    drains = [(tuple(float(v) for v in sc["pos"][100]), 170.0), (c, 40.0)]
    return sources, drains


def np_emit(sc, sources, dtype, h=H, scale=SCALE):
    """ompsph.hpp:93-105 in `dtype`: appended behind the particles present"""
    N = dtype
    spacing = N(N(h) * N(scale)) / N(2)
    out = {k: [v] for k, v in sc.items()}
    for tag, centre, velocity, colour, rate in sources:
        size = np.sqrt(N(rate))
        width, depth = int(np.floor(size)), int(np.ceil(size))
        half = np.array([N(width), N(0), N(depth)], N) * N(0.5) * spacing
        offset = np.array(centre, N) - half
        for x in range(width):
            for z in range(depth):
                pos = offset + np.array([N(x), N(0), N(z)], N) * spacing
                out["id"].append(np.array([tag], np.uint64)), out["type"].append(np.zeros(1, np.uint8))
                out["mass"].append(np.ones(1, N)), out["pos"].append(pos.astype(N)[None])
                out["vel"].append(np.array(velocity, N)[None]), out["colour"].append(np.array(colour, N)[None])
    return {k: np.concatenate(v) for k, v in out.items()}


def np_drain(sc, drains, dtype):
    """ompsph.hpp:107-118 in `dtype`: stable erase of the fluid particles with distance(centre, position) < width"""
    N = dtype
    gone = np.zeros(len(sc["id"]), bool)
    for centre, width in drains:
        d = sc["pos"].astype(N) - np.array(centre, N)
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(N) + d[:, 2] * d[:, 2]
        gone |= np.sqrt(s.astype(N)) < N(width)
    gone &= sc["type"] != 1
    return {k: v[~gone] for k, v in sc.items()}


def same(a, b, keys=("id", "type", "mass", "pos", "vel", "colour")):
    """every field, every bit (byte comparison: -0.0 differs from 0.0)"""
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return False
    return True


def oracle_frame(O, o, q, sources, drains, points=()):
    """one advance() of the oracle: emit -> drain -> predict -> sort -> grid_table [-> queries] -> diffuse -> K x
    (lambda, delta) -> finalise; returns (counts before / after emit / after drain, query answers)"""
    n0 = o.n
    if sources:
        o.emit(sources)
    n1 = o.n
    if drains:
        o.drain(drains)
    n2 = o.n
    answers = []
    if n2:
        o.predict(q).sort(q).grid_table(q)
        answers = [o.query(q, pt) for pt in points]
        o.diffuse(q)
        for _ in range(int(q.iteration)):
            o.lambda_(q).delta(q)
        o.finalise(q)
    return (n0, n1, n2), answers
