"""Multi-rank slab driver on CPU: world_size 2 and 3 with the "gloo" backend and the oracle engine.
Checks the N>1 host logic (cuts, migration, ghost copies, per-phase refresh, neighbour exchange):
the union of the ranks' particles after S steps equals a single-rank run to summation-order noise,
nothing is lost or duplicated, and particles really crossed the cut."""
import os
import queue
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def launch(world, out, *extra, timeout=600):
    port = 29500 + (os.getpid() % 2000)
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "slab_worker.py"), "--out", out, *extra],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    # One watcher per rank drains its output (a rank must never block on a full pipe) and reports its exit.  The first
    # failure, or the deadline, ends the remaining ranks at once: a rank stuck in an exchange with a vanished peer must
    # not stay behind holding the device.
    outs, ended = [""] * world, queue.Queue()

    def watch(r):
        outs[r] = procs[r].stdout.read()
        ended.put(procs[r].wait())

    watchers = [threading.Thread(target=watch, args=(r,), daemon=True) for r in range(world)]
    for t in watchers:
        t.start()
    deadline = time.monotonic() + timeout
    try:
        for _ in range(world):
            if ended.get(timeout=max(0.0, deadline - time.monotonic())) != 0:
                break
    except queue.Empty:
        pass
    finally:
        late = [r for r, p in enumerate(procs) if p.poll() is None]
        for r in late:
            procs[r].kill()
        for t in watchers:
            t.join()
    # (the rank that fails FIRST holds the cause; the others only see their peer vanish — or were ended here)
    assert not late and all(p.returncode == 0 for p in procs), f"ranks ended by the launcher: {late}\n" + "\n".join(
        f"--- rank {r} (exit {p.returncode}) ---\n" + "\n".join(ln for ln in o.splitlines() if "socket.cpp" not in ln)[-1500:]
        for r, (p, o) in enumerate(zip(procs, outs)))
    return [np.load(os.path.join(out, f"rank{r}.npz")) for r in range(world)]


def merged(parts):
    cat = {k: np.concatenate([p[k] for p in parts]) for k in ("id", "pos", "vel", "colour", "type")}
    o = np.argsort(cat["id"], kind="stable")
    return {k: v[o] for k, v in cat.items()}


@pytest.mark.parametrize("world,steps,cuts", [(2, 6, "x:210"), (3, 4, "x:210,700")])
def test_slabs_match_single_rank_oracle(oracle, pkg, tmp_path, world, steps, cuts):
    # the cuts run THROUGH the two cubes (x in [100, 320] and [600, 820]), so every phase needs its neighbour
    parts = launch(world, str(tmp_path), "--engine", "oracle", "--scene", "cubes2048", "--steps", str(steps),
                   "--cuts", cuts)
    got = merged(parts)
    sc = pkg.scene_cubes(2048)
    assert np.array_equal(got["id"], np.sort(sc["id"]))  # nothing lost, nothing duplicated, no ghost leaked
    o = oracle.Oracle(False, device_pow=True)
    o.set_particles(**sc)
    q = oracle.make_params(mode=oracle.JACOBI, sort=oracle.SORT_STABLE, threads=2)
    for _ in range(steps):
        o.step(q)
    w = o.get_particles()
    wo = np.argsort(w["id"], kind="stable")
    d = np.linalg.norm(got["pos"].astype(np.float64) - w["pos"][wo], axis=1)
    # same arithmetic, only the order inside a cell (hence the fp32 summation order) may differ
    assert d.max() <= 2e-2 and d.mean() <= 1e-4, (d.max(), d.mean())
    assert sum(int(p["ghosts"]) for p in parts) > 0
    assert all(int(p["exchanges"]) >= steps * 8 for p in parts)  # 2K field refreshes per step at least


def test_particles_cross_the_cut(oracle, pkg, tmp_path):
    """A dam-break column next to the cut: after 25 steps fluid has migrated to the other rank."""
    parts = launch(2, str(tmp_path), "--engine", "oracle", "--scene", "dam2048", "--steps", "25", "--iteration", "2",
                   "--cuts", "x:150")
    got = merged(parts)
    sc, side = pkg.scene_dambreak(2048)
    assert np.array_equal(got["id"], np.sort(sc["id"]))
    assert sum(int(p["migrated"]) for p in parts) > 0
    o = oracle.Oracle(False, device_pow=True)
    o.set_particles(**sc)
    q = oracle.make_params(iteration=2, max_bound=(side,) * 3, mode=oracle.JACOBI, sort=oracle.SORT_STABLE, threads=2)
    for _ in range(25):
        o.step(q)
    w = o.get_particles()
    wo = np.argsort(w["id"], kind="stable")
    d = np.linalg.norm(got["pos"].astype(np.float64) - w["pos"][wo], axis=1)
    assert np.percentile(d, 99) <= 0.5 and d.mean() <= 0.05, (d.max(), d.mean())
    assert got["pos"].min() >= 0 and got["pos"].max() <= side


def test_recut_moves_cuts_towards_balance_in_bounded_steps(pkg):
    from pbf_sph_amd import slab
    h = np.zeros(1024, np.int64)
    h[10:70] = 100            # all the fluid in columns 10..69
    cuts = [0, 300, 600, 1024]
    seen = [cuts]
    for _ in range(400):
        new = slab.recut(cuts, h)
        # bounded move, strictly increasing, ends pinned
        assert new[0] == 0 and new[-1] == 1024
        assert all(abs(a - b) <= slab.MAX_CUT_MOVE for a, b in zip(new, cuts))
        assert all(new[g + 1] - new[g] >= 1 for g in range(3))
        if new == cuts:
            break
        cuts = new
        seen.append(cuts)
    loads = [h[cuts[g]:cuts[g + 1]].sum() for g in range(3)]
    assert max(loads) <= 1.1 * sum(loads) / 3, (cuts, loads)   # converged to the quantiles
    assert cuts[2] - cuts[1] >= slab.MIN_SLAB_COLUMNS
    # deterministic: the same inputs give the same cuts (every rank computes them independently)
    assert slab.recut(seen[0], h) == slab.recut(list(seen[0]), h.copy())


@pytest.mark.parametrize("scene,cuts", [("dam2048", "x:400,700"), ("dam8192", "balanced")])
def test_slabs_rebalance_cpu(oracle, pkg, tmp_path, scene, cuts):
    """3 ranks, re-cut every 2 steps: particles of a transferred column migrate through the ordinary migration
    round; the union still equals the single-rank run to summation-order noise.  "x:400,700": cuts placed badly;
    "balanced": particle-count quantiles of the start column = slabs only TWO columns wide, cuts moving through
    the fluid, particles crossing > 1 column per step in the lattice blow-up (this is what bench.py's strong
    scaling does; it needs the local key frame's margin, PBF_SLAB_FRAME_MARGIN)."""
    steps = 12
    parts = launch(3, str(tmp_path), "--engine", "oracle", "--scene", scene, "--steps", str(steps), "--iteration", "2",
                   "--cuts", cuts, "--rebalance", "2")
    assert int(parts[0]["recuts"]) > 0
    assert all(np.array_equal(parts[0]["cuts"], p["cuts"]) for p in parts)       # every rank agrees on the cuts
    assert not np.array_equal(parts[0]["cuts"], [0, 10, 16, 1024])               # and they moved
    got = merged(parts)
    sc, side = pkg.scene_dambreak(int(scene[3:]))
    assert np.array_equal(got["id"], np.sort(sc["id"]))
    o = oracle.Oracle(False, device_pow=True)
    o.set_particles(**sc)
    q = oracle.make_params(iteration=2, max_bound=(side,) * 3, mode=oracle.JACOBI, sort=oracle.SORT_STABLE, threads=2)
    for _ in range(steps):
        o.step(q)
    w = o.get_particles()
    wo = np.argsort(w["id"], kind="stable")
    d = np.linalg.norm(got["pos"].astype(np.float64) - w["pos"][wo], axis=1)
    assert np.percentile(d, 99) <= 0.5 and d.mean() <= 0.05, (d.max(), d.mean())


@pytest.mark.parametrize("xsph,vort", [(1, 1), (1, 0), (0, 1)])
def test_slabs_with_xsph_and_vorticity_cpu(oracle, pkg, tmp_path, xsph, vort):
    """The opt-in extras in slab mode: the owners refresh their copies' velocity / vorticity before each op that reads
    them; the union equals the single-rank oracle (which runs the three ops back to back) to summation-order noise."""
    steps = 4
    parts = launch(2, str(tmp_path), "--engine", "oracle", "--scene", "cubes2048", "--steps", str(steps), "--cuts", "x:210",
                   "--xsph", str(xsph), "--vorticity", str(vort))
    got = merged(parts)
    sc = pkg.scene_cubes(2048)
    assert np.array_equal(got["id"], np.sort(sc["id"]))
    o = oracle.Oracle(False, device_pow=True)
    o.set_particles(**sc)
    q = oracle.make_params(mode=oracle.JACOBI, sort=oracle.SORT_STABLE, threads=2, xsph=xsph, vorticity=vort)
    plain = oracle.Oracle(False, device_pow=True)
    plain.set_particles(**sc)
    q0 = oracle.make_params(mode=oracle.JACOBI, sort=oracle.SORT_STABLE, threads=2)
    for _ in range(steps):
        o.step(q)
        plain.step(q0)
    w = o.get_particles()
    wo = np.argsort(w["id"], kind="stable")
    dv = np.abs(got["vel"].astype(np.float64) - w["vel"][wo]).max()
    d = np.linalg.norm(got["pos"].astype(np.float64) - w["pos"][wo], axis=1)
    assert d.max() <= 2e-2 and d.mean() <= 1e-4 and dv <= 1e-3, (d.max(), d.mean(), dv)
    # ... and the extras really act (the comparison above is not vacuous)
    wp = plain.get_particles()
    assert np.abs(w["vel"][wo] - wp["vel"][np.argsort(wp["id"], kind="stable")]).max() > 1e-6
