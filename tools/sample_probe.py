#!/usr/bin/env python3
"""Time pbf_sample_lattice on the settled dam-break, with one PBF_DIAG_DENSITY pass on the same state for scale.

    python tools/sample_probe.py [--particles 1048576] [--dims 128] [--settle 400] [--reps 5] [--fp64]

The solver runs on a torch stream; each figure is the time between two events recorded on that stream around ONE call,
after a warm-up call of the same kind (which also makes the allocations), the median of `reps` such calls.  The calls
synchronise, so the interval holds the launch, the kernel, the copies of the outputs that were asked for and the stream
sync: the "*_kernel" entries hand over the 1-byte-per-point `outside` array only (every other output NULL: as close to
the kernel as a call gets, not a kernel-trace figure), the "*_call" entries all outputs the flags allow.
Prints one JSON line."""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_package():
    pkg_dir = os.path.join(ROOT, "pbf-sph_amd")
    spec = importlib.util.spec_from_file_location("pbf_sph_amd", os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["pbf_sph_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--dims", type=int, default=128)
    ap.add_argument("--settle", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fp64", action="store_true")
    a = ap.parse_args()
    import ctypes as C
    pkg = load_package()
    from pbf_sph_amd import capi
    stream = torch.cuda.Stream()
    sc, side = pkg.scene_dambreak(a.particles, a.fp64)
    s = pkg.Solver(h=0.1, fp64=a.fp64, stream=stream.cuda_stream).upload(**sc)
    p = pkg.default_params(4, side)
    s.steps(p, a.settle).sync()
    n = a.dims ** 3
    dt = np.float64 if a.fp64 else np.float32
    arrays = dict(rho=np.zeros(n, dt), weight=np.zeros(n, dt), mv=np.zeros(3 * n, dt), mc=np.zeros(4 * n, dt),
                  count=np.zeros(2 * n, np.uint32), outside=np.zeros(n, np.uint8))
    origin, spacing = np.zeros(3), np.full(3, side / (a.dims - 1))
    dims = np.full(3, a.dims, np.uint64)

    def lattice(what, names):
        out = capi.SampleOut(*[arrays[k].ctypes.data if k in names else None for k in ("rho", "weight", "mv", "mc", "count", "outside")])
        rc = s.L.pbf_sample_lattice(s.ctx, C.byref(p), origin.ctypes.data, spacing.ctypes.data, dims.ctypes.data, what, C.byref(out))
        assert rc == 0, s.L.pbf_last_error(s.ctx)

    def timed(fn):
        fn()                                    # warm-up: allocations, code load
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))

    both = pkg.SAMPLE_VELOCITY | pkg.SAMPLE_COLOUR
    res = dict(particles=len(sc["id"]), box_side=side, settle_steps=a.settle, dims=[a.dims] * 3, fp64=a.fp64, reps=a.reps,
               lattice_both_kernel=timed(lambda: lattice(both, ["outside"])),
               lattice_none_kernel=timed(lambda: lattice(0, ["outside"])),
               lattice_both_call=timed(lambda: lattice(both, list(arrays))),
               lattice_none_call=timed(lambda: lattice(0, ["rho", "weight", "count", "outside"])),
               diag_density=timed(lambda: s.diagnostics(p, density=True)))
    res["in_fluid_points"] = int((arrays["weight"] > 0).sum())
    res["outside_points"] = int(arrays["outside"].sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
