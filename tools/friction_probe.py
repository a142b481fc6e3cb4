#!/usr/bin/env python3
"""What the collider friction pass costs per step, and what one pbf_collider_friction_reaction call costs.

    python tools/friction_probe.py step [--particles 1048576] [--iteration 4] [--settle 80] [--steps 200] [--reps 3]
    python tools/friction_probe.py observer [--particles 1048576] [--iteration 4] [--settle 80] [--calls 200]

Both run the dam-break with a ball of radius 500 in the path of the column (profiles/collider_body_1m.md's: a 25^3 lattice
of spacing 50 in the ball's own frame, posed at (2600, 4300, 1000), turning about y at 1 rad per time).

step      `reps` times, alternated from one common settled state: the wall time of pbf_steps(p, steps) from the call to the
          end of pbf_sync with the reaction alone, and with friction on (mu 0.5, the spin as the contact velocity).  Two
          solvers of one process, each warmed with `steps` steps first.  Prints the times and the difference per step.
observer  `calls` calls of pbf_collider_friction_reaction after one step: the mean host time of a call (one single-workgroup
          launch and the polled read-back), and beside it the same figure for pbf_collider_reaction (two launches).

Each prints one JSON line.  A host clock around work that ends in a device synchronise; no trace, no counters.  Run each
sub-command as a process of its own under a time limit, chained with `&&`:

    timeout -k 10 300 python tools/friction_probe.py step && timeout -k 10 300 python tools/friction_probe.py observer
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTRE, RADIUS, SPIN = (2600.0, 4300.0, 1000.0), 500.0, (0.0, 1.0, 0.0)
LATTICE = dict(origin=(-600.0,) * 3, spacing=50.0, dims=(25, 25, 25))
MARGIN, MU = 13.5, 0.5


def load_package():
    pkg_dir = os.path.join(ROOT, "pbf-sph_amd")
    spec = importlib.util.spec_from_file_location("pbf_sph_amd", os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["pbf_sph_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def with_ball(pkg, state, friction):
    s = pkg.Solver(h=0.1).upload(**state)
    phi = pkg.sdf_lattice(pkg.sdf_sphere((0.0, 0.0, 0.0), RADIUS), LATTICE["origin"], LATTICE["spacing"], LATTICE["dims"])
    s.set_collider(phi, LATTICE["origin"], LATTICE["spacing"], MARGIN).set_collider_pose(np.eye(3), CENTRE).set_collider_reaction(True)
    return s.set_collider_friction(MU, (0.0, 0.0, 0.0), SPIN) if friction else s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["step", "observer"])
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--iteration", type=int, default=4)
    ap.add_argument("--settle", type=int, default=80)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    pkg = load_package()
    sc, side = pkg.scene_dambreak(a.particles, False)
    p = pkg.default_params(a.iteration, side)
    state = pkg.Solver(h=0.1).upload(**sc).steps(p, a.settle).download()
    n = len(state["id"])
    if a.what == "step":
        runs = {False: with_ball(pkg, state, False), True: with_ball(pkg, state, True)}
        for s in runs.values():
            s.steps(p, a.steps).sync()
        ms = {False: [], True: []}
        for _ in range(a.reps):
            for on in (False, True):
                s = runs[on].upload(**state)
                s.steps(p, 5).sync()                           # (the first steps after an upload allocate nothing new, but sort an unsorted state)
                t0 = time.perf_counter()
                s.steps(p, a.steps).sync()
                ms[on].append(1e3 * (time.perf_counter() - t0))
        fr = runs[True].collider_friction_reaction()
        wr = runs[True].collider_reaction()
        print(json.dumps({"what": "step", "particles": n, "steps": a.steps, "reaction_alone_ms": ms[False], "friction_ms": ms[True],
                          "per_step_ms": (statistics.median(ms[True]) - statistics.median(ms[False])) / a.steps,
                          "last_pass": {"in_contact": fr["particles"], "slid": fr["hits"], "passes": fr["step"]},
                          "last_step_hits": wr["hits"]}))
    else:
        s = with_ball(pkg, state, True).steps(p, 5).sync()
        out = {}
        for name, call in (("friction_reaction", s.collider_friction_reaction), ("reaction", s.collider_reaction)):
            call()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call(raw=True)
            out[name + "_ms_per_call"] = 1e3 * (time.perf_counter() - t0) / a.calls
        print(json.dumps({"what": "observer", "particles": n, "calls": a.calls, **out}))


if __name__ == "__main__":
    main()
