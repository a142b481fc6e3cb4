#!/usr/bin/env python3
"""Time pbf_anisotropy_compute on the settled dam-break, with one PBF_DIAG_DENSITY pass on the same state for scale.

    python tools/anisotropy_probe.py [--particles 1048576] [--settle 400] [--reps 5] [--fp64]

The method of tools/sample_probe.py: the solver runs on a torch stream; each figure is the time between two events recorded
on that stream around ONE call, after a warm-up call of the same kind (which also makes the allocations), the median of
`reps` such calls.  The calls synchronise, so the interval holds the launch, the kernel, the copies of the outputs that were
asked for and the stream sync: "kernel" hands over the 4-byte-per-particle neighbour counts only (as close to the kernel
as a call gets, not a kernel-trace figure), "call" all five arrays.  Prints one JSON line."""
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
    ap.add_argument("--settle", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fp64", action="store_true")
    a = ap.parse_args()
    pkg = load_package()
    stream = torch.cuda.Stream()
    sc, side = pkg.scene_dambreak(a.particles, a.fp64)
    s = pkg.Solver(h=0.1, fp64=a.fp64, stream=stream.cuda_stream).upload(**sc)
    p = pkg.default_params(4, side)
    s.steps(p, a.settle).sync()
    last = {}

    def timed(fn):
        fn()                                    # warm-up: allocations, code load
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            last["out"] = fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))

    res = dict(particles=len(sc["id"]), box_side=side, settle_steps=a.settle, fp64=a.fp64, reps=a.reps,
               anisotropy_kernel=timed(lambda: s.anisotropy(p, only=["neighbours"])),
               anisotropy_call=timed(lambda: s.anisotropy(p)),
               diag_density=timed(lambda: s.diagnostics(p, density=True)))
    res["nbr_mean_diag"] = last["out"]["nbr_mean"]       # (obstacles count as neighbours there, not here)
    got = s.anisotropy(p)
    res["neighbours_mean"] = float(got["neighbours"].mean())
    res["anisotropic_share"] = float((got["neighbours"] > 25).mean())
    res["radii_median"] = [float(x) for x in np.median(got["radii"], 0)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
