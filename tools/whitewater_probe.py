#!/usr/bin/env python3
"""Percentiles of the whitewater potentials on a scene — how the tau ranges of pbf_whitewater are picked — and the time of
one whitewater step on it.

    python tools/whitewater_probe.py [--scene dam-break|cubes] [--particles 1048576] [--iteration 4] [--settle 200]
                                     [--pool 0] [--reps 5] [--fp64]

Steps the scene `settle` times, runs one whitewater step with rates 0 (the potentials do not depend on the tau ranges or
the rates) and prints, for I_ta, I_wc and E_k over the fluid particles, the share of positive values and their 1 / 5 / 10 /
25 / 50 / 75 / 90 / 95 / 99 % quantiles.  A tau range of (10 %, 90 %) of the positive values is a reasonable start.
Then `reps` whitewater steps with rates 1 on that range and a pool of `pool` uploaded foam particles (0: an empty pool),
each between two events on the solver's stream, after one warm-up step: the interval around a host-blocking call,
polled read-back included — a figure for orientation, not a kernel time (profiles/whitewater_cost.md has the trace).
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
QUANTILES = (0.01, 0.05, 0.10, 0.25, 0.50, 0.75, 0.90, 0.95, 0.99)


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
    ap.add_argument("--scene", default="dam-break", choices=["dam-break", "cubes"])
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--iteration", type=int, default=4)
    ap.add_argument("--settle", type=int, default=200)
    ap.add_argument("--pool", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fp64", action="store_true")
    a = ap.parse_args()
    pkg = load_package()
    stream = torch.cuda.Stream()
    if a.scene == "dam-break":
        sc, side = pkg.scene_dambreak(a.particles, a.fp64)
    else:
        sc, side = pkg.scene_cubes(a.particles, a.fp64), 1000.0
    s = pkg.Solver(h=0.1, fp64=a.fp64, stream=stream.cuda_stream).upload(**sc)
    p = pkg.default_params(a.iteration, side)
    s.steps(p, a.settle).sync()
    capacity = max(4 * a.pool, 1 << 16)
    s.whitewater_configure(capacity=capacity, tau_ta=(0, 1), tau_wc=(0, 1), tau_k=(0, 1))
    s.whitewater_step(p)
    pot = s.whitewater_potentials().astype(np.float64)
    down = s.download()
    fluid = down["type"] == 0
    res = dict(scene=a.scene, particles=len(sc["id"]), box_side=side, settle_steps=a.settle, fp64=a.fp64)
    taus = {}
    for col, name in enumerate(("I_ta", "I_wc", "E_k")):
        v = pot[fluid, col]
        pos = v[v > 0]
        q = [float(x) for x in np.quantile(pos, QUANTILES)] if len(pos) else []
        res[name] = dict(positive_share=float(len(pos) / max(len(v), 1)), max=float(v.max()) if len(v) else 0.0,
                         quantiles_of_positive={f"{int(k * 100)}%": x for k, x in zip(QUANTILES, q)})
        taus[name] = (q[2], q[6]) if len(pos) and q[6] > q[2] else (0.0, 1.0)
    s.whitewater_configure(capacity=capacity, k_ta=1.0, k_wc=1.0, tau_ta=taus["I_ta"], tau_wc=taus["I_wc"], tau_k=taus["E_k"])
    if a.pool:
        pick = np.random.default_rng(1).integers(0, int(fluid.sum()), a.pool)
        s.whitewater_upload(down["pos"][fluid][pick], down["vel"][fluid][pick])
    stats = s.whitewater_step(p)                  # warm-up: allocations, code load
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        stats = s.whitewater_step(p)
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    res["step"] = dict(pool_uploaded=a.pool, reps=a.reps, median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms),
                       last_stats=stats)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
