"""The scenes of the anisotropy tests — TEST INFRASTRUCTURE.

`cubes1024`, `cloud` and `obstacles` are those of tests/test_nversion_cpu.py, `strays` that of tests/test_sample_cpu.py.  They
are at or above rest density: nearly every fluid particle has more than 8 neighbours, so with min_neighbours = 8 the isotropic
branch holds under 3 % of the fluid in each of them.  `sparse` is added for that branch: 900 particles drawn uniformly in a
330^3 world-unit box clear of the walls, a third of `cloud`'s density — about 11.5 neighbours within h on average, so with
min_neighbours = 8 a quarter of the fluid has too few neighbours and three quarters have enough (with 25 none has).
"""
import numpy as np

import oracle_lib as O
from test_nversion_cpu import scene as _nversion_scene
from test_sample_cpu import oracle_state as _sample_state

SCENES = ["cubes1024", "cloud", "obstacles", "sparse"]

_STATES = {}


def scene(name):
    if name != "sparse":
        return _nversion_scene(name)
    rng = np.random.default_rng(23)
    n = 900
    pos = rng.random((n, 3)) * 330.0 + np.array([100.0, 500.0, 100.0])
    return dict(id=np.arange(n, dtype=np.uint64), type=np.zeros(n, np.uint8), mass=np.ones(n), pos=pos,
                vel=(rng.random((n, 3)) - 0.5) * 2.0, colour=rng.random((n, 4)))


def oracle_state(name):
    """the oracle's state after the 3 steps (K = 2) the GPU test takes, in float64 (`strays`: see tests/test_sample_cpu.py)"""
    if name != "sparse":
        return _sample_state(name)
    if name not in _STATES:
        q = O.make_params(iteration=2, mode=O.JACOBI, sort=O.SORT_STABLE)
        o = O.Oracle(True)
        o.set_particles(**scene(name))
        for _ in range(3):
            o.step(q)
        _STATES[name] = dict(down=o.get_particles(), pstar=o.pstar().astype(np.float64), keys=o.keys().astype(np.uint32),
                             scale=q.scale)
    return _STATES[name]
