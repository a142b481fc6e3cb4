"""Worker of the slab tests: one rank of an N-rank run of pbf-sph_amd/slab.py.

  engine "oracle": CPU engine (tests/slab_engines.py), gloo, CPU tensors        — runs anywhere
  engine "hip"   : the product kernels on cuda:0 driven by slab.py's Python protocol, gloo with host-staged buffers
  engine "hipc"  : the product path: pbf_slab_step inside libpbf_hip.so (C ABI) with the host-callback transport
                   over gloo                                                      — several ranks share ONE GPU
Writes the rank's final owned particles to <out>/rank<r>.npz.

  --scene mc:<name>   a scene of tests/mc_scenes.py with its own params (mc_scenes.device_params)
  --cuts c:3,7        explicit cell columns of the interior cuts
  --surface "<res,iso,size,infl>;..."   (hipc) after the steps, pbf_surface once per set on every rank — it is collective,
                      and repeatable while the copies are pending — stored as surf<i>_{sample,pn,c,vs,ns,cs,rounds}
                      (rounds = what the call added to pbf_comm_rounds); a set marked "!" is expected to be refused:
                      surf<i>_{rc,rounds}.  After the final download both surface calls once more: after_rc = their codes.
  --peek-at S         download the owned particles after step S (peek_*), then go on stepping
  --scene boxN        the moving box of tests/trip_scenes.py
  --trace             (oracle) per step, where in the arrays the selects' classes sit: trace_<counter>[step], the counters of
                      OracleEngine.trace"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from conftest import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", default="oracle")
    ap.add_argument("--scene", default="cubes2048")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--iteration", type=int, default=4)
    ap.add_argument("--cuts", default="even")
    ap.add_argument("--fp64", action="store_true")
    ap.add_argument("--rebalance", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=0, help="records in the first message of an assembly round (hipc)")
    ap.add_argument("--xsph", type=int, default=0)
    ap.add_argument("--vorticity", type=int, default=0)
    ap.add_argument("--surface", default="")
    ap.add_argument("--peek-at", type=int, default=0)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = load_package()
    from pbf_sph_amd import slab

    if a.scene.startswith("mc:"):
        import mc_scenes as M
        ms = M.make(a.scene[3:])
        # the column formula below and slab.column_of assume these
        assert ms["h"] == 0.1 and ms["scale"] == 500.0 and tuple(ms["min_bound"]) == (0.0, 0.0, 0.0), a.scene
        sc, side = M.cast(ms["sc"], np.float64 if a.fp64 else np.float32), 1000.0
        p = M.device_params(pkg, ms)
    else:
        if a.scene.startswith("cubes"):
            sc, side = pkg.scene_cubes(int(a.scene[5:]), a.fp64), 1000.0
        elif a.scene.startswith("box"):
            import trip_scenes
            sc, side = trip_scenes.box_scene(int(a.scene[3:]), a.fp64)
        else:
            sc, side = pkg.scene_dambreak(int(a.scene[3:]), a.fp64)
        p = pkg.default_params(a.iteration, side)
    p.xsph, p.vorticity = a.xsph, a.vorticity
    if a.cuts == "even":
        cuts = slab.even_cuts(world, side)
    elif a.cuts.startswith("x:"):  # explicit world-space cut positions
        cuts = [0] + [slab.column_of(float(v)) for v in a.cuts[2:].split(",")] + [1024]
    elif a.cuts.startswith("c:"):  # explicit cell columns
        cuts = [0] + [int(v) for v in a.cuts[2:].split(",")] + [1024]
    else:
        cuts = slab.balanced_cuts(world, sc["pos"][:, 0], side)
    col = ((sc["pos"][:, 0].astype(np.float64) / 500.0 + 0.2) / 0.1).astype(np.int64)
    mine = (col >= cuts[rank]) & (col < cuts[rank + 1])
    part = {k: v[mine] for k, v in sc.items()}
    cap = len(sc["id"])
    if a.engine == "oracle":
        from slab_engines import OracleEngine
        eng = OracleEngine(a.fp64, device_pow=True)
        eng.upload(**part)
        if a.trace:
            eng.trace = []
        get = eng.download
        stage = False
    else:
        s = pkg.Solver(h=0.1, fp64=a.fp64, device=0)
        s._chk(s.L.pbf_reserve(s.ctx, cap), "pbf_reserve")
        s.upload(**part)
        eng = slab.HipEngine(s, torch, torch.device("cuda", 0))
        get = s.download
        stage = True
    assert len(cuts) == world + 1, (cuts, world)
    extra = {}

    def run(drv):
        if 0 < a.peek_at < a.steps:
            drv.steps(p, a.peek_at)
            extra.update({"peek_" + k: v for k, v in get().items()})
            drv.steps(p, a.steps - a.peek_at)
        else:
            drv.steps(p, a.steps)

    assert not a.surface or a.engine == "hipc", "--surface needs the library's slab step"
    if a.engine == "hipc":
        drv = slab.CSlabSolver(s, dist, torch, rank, world, cuts, a.chunk or cap, a.chunk or cap, transport="gloo-host",
                               rebalance_every=a.rebalance)
        run(drv)
        for i, spec in enumerate(x for x in a.surface.split(";") if x):
            mc = pkg.McParams(*[float(v) for v in spec.lstrip("!").split(",")])
            r0 = drv.rounds
            if spec.startswith("!"):
                nt = C.c_uint64()
                extra[f"surf{i}_rc"] = s.L.pbf_surface(s.ctx, C.byref(p), C.byref(mc), C.byref(nt))
            else:
                for k, v in s.surface(p, mc).items():
                    extra[f"surf{i}_{k}"] = v
            extra[f"surf{i}_rounds"] = drv.rounds - r0
        stats = dict(migrated=-1, ghosts=-1, exchanges=drv.rounds, recuts=drv.stats["recuts"])
        cuts = drv.cuts
    else:
        drv = slab.SlabSolver(eng, dist, rank, world, cuts, cap, stage_via_host=stage, rebalance_every=a.rebalance)
        run(drv)
        stats = dict(migrated=drv.stats["migrated"], ghosts=drv.stats["ghosts"], exchanges=drv.stats["exchanges"],
                     recuts=drv.stats["recuts"])
        cuts = drv.cuts
    out = get()
    if a.trace and a.engine == "oracle":
        extra.update({"trace_" + k: np.array([t[k] for t in eng.trace], np.int64) for k in eng.trace[0]})
    if a.surface:  # the download dropped the copies: both calls are refused, and neither exchanges anything
        mc, nv, nt, r0 = pkg.McParams(), C.c_uint64(), C.c_uint64(), drv.rounds
        extra["after_rc"] = np.array([s.L.pbf_surface(s.ctx, C.byref(p), C.byref(mc), C.byref(nt)),
                                      s.L.pbf_surface_indexed(s.ctx, C.byref(p), C.byref(mc), C.byref(nv), C.byref(nt))])
        extra["after_rounds"] = drv.rounds - r0
    os.makedirs(a.out, exist_ok=True)
    np.savez(os.path.join(a.out, f"rank{rank}.npz"), cuts=np.array(cuts), **stats, **out, **extra)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
