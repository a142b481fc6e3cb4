"""The reference-side values test_oracle_vs_ref.py checks the oracle against.

Computed live from oracle/_ref/libref_grid.so (the reference's own glm-free headers, built only where the reference
is present), or read from golden/ref_live.npz, which golden/make_golden.py writes from these same functions.  Every
input is seeded or derived from the oracle, so both sources hold the same values.  The fixture keeps numbers and
SHA-256 digests only.
"""
import ctypes as C
import hashlib
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_live.npz")
SCENE_COUNTS = (1024, 8192, 9000)
SCENE_FIELDS = ("id", "pos", "colour", "mass", "vel")
GIA_STRIDE = 37


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def digest(*arrays):
    """SHA-256 over dtype, shape and bytes of each array, as 32 uint8."""
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def morton_inputs():
    rng = np.random.default_rng(1)
    return rng.integers(0, 2048, size=(4000, 3)), rng.integers(0, 2 ** 31, size=4000)


def morton(R):
    xyz, codes = morton_inputs()
    return {"morton_enc": np.array([R.ref_morton_encode(int(x), int(y), int(z)) for x, y, z in xyz], np.uint64),
            "morton_dec": np.array([[R.ref_morton_decode(int(c), a) for a in range(3)] for c in codes], np.uint64)}


def foreach_homes(tn):
    rng = np.random.default_rng(2)
    return np.concatenate([np.array([0, 1, 2, 3, tn - 1, tn - 2, tn, tn + 9], np.uint64),
                           rng.integers(0, tn + 100, 300, dtype=np.uint64)])


def foreach_grid(R):
    """sph::foreach_grid's visits from every home cell on an identity table of extent 24^3 (table[c] = c: every
    cell holds exactly one "particle" whose index is the cell code)."""
    tn = R.ref_morton_encode(24, 24, 24)
    table = np.arange(tn, dtype=np.uint64)
    buf = np.empty(64, np.uint64)
    counts, visits = [], []
    for h in foreach_homes(tn):
        k = R.ref_foreach_grid(int(h), vp(table), tn, vp(buf), 64)
        counts.append(k)
        visits.append(buf[:k].copy())
    return {"fg_tn": np.array([tn], np.uint64), "fg_counts": np.array(counts, np.uint64),
            "fg_visits": np.concatenate(visits)}


def real_frame(O, fp64):
    """The oracle after three steps of the 8192-particle two-cube scene, then predict + sort + grid table."""
    s = O.scene_cubes(8192, fp64)
    o = O.Oracle(fp64)
    o.set_particles(**s)
    p = O.make_params()
    for _ in range(3):
        o.step(p)
    o.predict(p).sort(p).grid_table(p)
    return o


def grid_index_inputs(o, fp64):
    """(pStar - minExtent) of every GIA_STRIDE-th sorted particle, in the run's precision."""
    dt = np.float64 if fp64 else np.float32
    _, m = o.extent()
    return (o.pstar()[::GIA_STRIDE] - m).astype(dt)


def grid_table(R, o, fp64):
    """makeGridTable over the oracle's sorted keys, and zCurveGridIndexAtCoordAt of grid_index_inputs."""
    nm = "f64" if fp64 else "f32"
    keys = o.keys()
    e, _ = o.extent()
    tn = R.ref_make_grid_table(int(e[0]), int(e[1]), int(e[2]), 0, None, None)
    t = np.empty(tn, np.uint64)
    R.ref_make_grid_table(int(e[0]), int(e[1]), int(e[2]), len(keys), vp(keys), vp(t))
    f = R.ref_grid_index_at_f64 if fp64 else R.ref_grid_index_at_f32
    h = float((np.float64 if fp64 else np.float32)(0.1))
    d = grid_index_inputs(o, fp64)
    return {f"gt_{nm}_keys": keys, f"gt_{nm}_table": t, f"gt_{nm}_d": d,
            f"gt_{nm}_gia": np.array([f(float(x), float(y), float(z), h) for x, y, z in d], np.uint64)}


def scene(R, count, fp64):
    """simpleConfigWith2Cubes(count, 4, 500) from the reference's factory: {field: array}."""
    nm, dt = ("f64", np.float64) if fp64 else ("f32", np.float32)
    fn = getattr(R, "ref_scene_cubes_" + nm)
    n = fn(count, 4, 500.0, None, None, None, None, None, None, None)
    a = dict(id=np.empty(n, np.uint64), type=np.empty(n, np.uint8), mass=np.empty(n, dt), pos=np.empty((n, 3), dt),
             vel=np.empty((n, 3), dt), colour=np.empty((n, 4), dt))
    fn(count, 4, 500.0, vp(a["id"]), vp(a["type"]), vp(a["mass"]), vp(a["pos"]), vp(a["vel"]), vp(a["colour"]), None)
    return a


def scene_digest(a):
    return digest(*(a[k] for k in SCENE_FIELDS))


def all_values(O, R):
    """Everything ref_live.npz holds, computed live."""
    out = {**morton(R), **foreach_grid(R)}
    for fp64 in (False, True):
        nm = "f64" if fp64 else "f32"
        out.update(grid_table(R, real_frame(O, fp64), fp64))
        for count in SCENE_COUNTS:
            out[f"scene_{count}_{nm}"] = scene_digest(scene(R, count, fp64))
    return out
