"""Floating bodies through the layers above the C ABI (item 9 of tests/test_collider_body_gpu.py's list): the C++ shim
(Solver::setColliderBody / clearColliderBody / colliderBody through advance(), host/test_collider_body_shim.cpp) and
`benchmark --collider-body ... --collider-body-report` give the frames and the body states of the same run over the C ABI,
bit for bit."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import collider_pose_ref as PR
import collider_ref as CR
from test_collider_gpu import solver
from test_collider_pose_gpu import body_lattice_through

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pbf-sph_amd", "benchmark")
# the body of host/test_collider_body_shim.cpp
SHIM_BODY = dict(mass=300.0, inertia=(3e6, 4e6, 5e6), gain=0.49, accel=(0.0, 200.0, 0.0), linear_damping=0.1, angular_damping=0.3,
                 rot=np.eye(3), centre=(500.0, 500.0, 500.0), velocity=(10.0, -20.0, 5.0), angular_velocity=(0.2, 0.1, -0.3))


def test_shim(pkg, tmp_path):
    from pbf_sph_amd import capi
    frames = 4
    sc = pkg.scene_cubes(2048)
    lat, phi64, origin, _ = body_lattice_through(sc, np.float32, (SHIM_BODY["rot"], np.array(SHIM_BODY["centre"])), 0.4)
    with open(tmp_path / "lattice.bin", "wb") as f:
        f.write(np.array(lat.dims, np.uint32).tobytes() + np.array(origin, np.float64).tobytes() +
                np.array([PR.BODY_SPACING, CR.MARGIN], np.float64).tobytes() + lat.phi.tobytes())
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_collider_body_shim"), str(tmp_path / "lattice.bin"),
                        str(tmp_path / "dump.bin"), str(frames)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    raw = open(tmp_path / "dump.bin", "rb").read()
    n = int(np.frombuffer(raw, np.uint64, 1)[0])
    at = 8

    def take(dtype, shape):
        nonlocal at
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at).reshape(shape)
        at += a.nbytes
        return a

    def particles():
        return dict(id=take(np.uint64, (n,)), type=take(np.uint8, (n,)), mass=take(np.float32, (n,)), pos=take(np.float32, (n, 3)),
                    vel=take(np.float32, (n, 3)), colour=take(np.float32, (n, 4)))

    first, last = particles(), particles()
    # the same frames over the C ABI: advance() is upload -> step -> download
    s = solver(pkg, False)
    s.set_collider(phi64, origin, PR.BODY_SPACING, CR.MARGIN).set_collider_body(**SHIM_BODY)
    p = pkg.default_params(4, 1000.0)
    p.dt = float(np.float32(p.dt))                            # the shim's config holds dt in N; the body takes it as a double
    st, size = first, C.sizeof(capi.ColliderBodyState)
    for k in range(frames):
        st = s.upload(**st).step(p).download()
        assert bytes(s.collider_body_state(raw=True)) == raw[at:at + size], k
        at += size
    assert at == len(raw)
    for k in last:
        assert st[k].tobytes() == last[k].tobytes(), k
    assert s.collider_body_state()["steps"] == frames


def test_cli_collider_body_and_report(pkg, tmp_path):
    # the cubes lie in y <= 198 (gravity is +y): the solid y > 150 starts inside them and sinks away under its own weight
    common = ["--scene", "cubes", "--particles", "2048", "--solver-iter", "4", "-n", "5", "-w", "0", "--resident", "--no-surface",
              "--collider=plane:0,-1,0,-150,13.5,50"]
    r = subprocess.run([BIN, *common, "--collider-body=300,3e6,4e6,5e6", "--collider-body-report", "-o", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.split("\n") if l.startswith('{"frame"')]
    assert [l["frame"] for l in lines] == [0, 1, 2, 3, 4] and all("body" in l for l in lines)
    # the same frames from Python: the CLI's lattice is the analytic plane, in double, on the box plus one spacing ABOUT the
    # body's centre (a plane: the box's), rounded to N; the body starts at rest there under constant_force * scale
    ax = (-50.0 - 500.0) + np.arange(23, dtype=np.float64) * 50.0
    w = ax + 500.0
    y = np.broadcast_to(w[None, :, None], (23, 23, 23))
    phi = ((0.0 * w[:, None, None] + -1.0 * y) + 0.0 * w[None, None, :]) / 1.0 - -150.0
    s = solver(pkg, False).upload(**pkg.scene_cubes(2048))
    base = pkg.default_params(4, 1000.0)
    base.dt = float(np.float32(base.dt))                      # the driver's config holds dt in N; the body takes it as a double
    g = float(np.float32(base.constant_force[1])) * float(np.float32(base.scale))
    s.set_collider(phi, (-550.0,) * 3, 50.0, 13.5)
    s.set_collider_body(mass=300.0, inertia=(3e6, 4e6, 5e6), gain=0.49, accel=(0.0, g, 0.0), rot=np.eye(3), centre=(500.0,) * 3,
                        centre_min=(0.0,) * 3, centre_max=(1000.0,) * 3)
    hits = 0
    for frame, l in enumerate(lines):
        st = s.step(pkg.apply_motion(base, frame, False)).collider_body_state()
        got = l["body"]
        for k in ("centre", "quat", "velocity", "angular_velocity", "impulse", "angular"):
            assert list(st[k]) == got[k], (frame, k, st[k], got[k])
        assert list(st["rot"].reshape(9)) == got["rot"], frame
        assert (st["hits"], st["steps"], st["rejected"]) == (got["hits"], got["steps"], got["rejected"]) and st["steps"] == frame + 1
        hits += st["hits"]
    assert hits > 0 and st["centre"][1] > 500.0
    # every second frame; refused with slabs, with --collider-motion and for a plane without moments; ignored without a collider
    r = subprocess.run([BIN, *common, "--collider-body=300,3e6,4e6,5e6", "--collider-body-report=2", "-o", str(tmp_path / "o2")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and [json.loads(l)["frame"] for l in r.stdout.split("\n") if l.startswith('{"frame"')] == [1, 3]
    r = subprocess.run([BIN, *common, "--collider-body=300,3e6,4e6,5e6", "--slabs", "2", "-o", str(tmp_path / "o3")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0 and "single-device" in r.stderr
    r = subprocess.run([BIN, *common, "--collider-body=300,3e6,4e6,5e6", "--collider-motion=1,0,0", "-o", str(tmp_path / "o4")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "both own" in r.stderr
    r = subprocess.run([BIN, *common, "--collider-body=300", "-o", str(tmp_path / "o5")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "moments" in r.stderr
    r = subprocess.run([BIN, *common[:-1], "--collider-body=300", "-o", str(tmp_path / "o6")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ignored" in r.stdout
    r = subprocess.run([BIN, *common, "--collider-body=300,1", "-o", str(tmp_path / "o7")], capture_output=True, text=True, timeout=300)
    # (a parse error prints the reason and the usage and exits 0, as every parse error of the driver: nothing may have run)
    assert "--collider-body: expected mass" in r.stderr and "Benchmark completed" not in r.stdout and '{"frame"' not in r.stdout
    r = subprocess.run([BIN, *common, "--collider-body=0", "-o", str(tmp_path / "o8")], capture_output=True, text=True, timeout=300)
    assert "--collider-body: mass and moments must be > 0" in r.stderr and "Benchmark completed" not in r.stdout
    h = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--collider-body=" in h and "--collider-body-report" in h
    # a sphere gets a solid ball's moments and floats from its own centre
    r = subprocess.run([BIN, *common[:-1], "--collider=sphere:300,250,300,80", "--collider-body=40", "--collider-body-report=5", "-o",
                        str(tmp_path / "o9")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    body = [json.loads(l) for l in r.stdout.split("\n") if l.startswith('{"frame"')][-1]["body"]
    assert body["steps"] == 5 and body["rejected"] == 0 and np.isfinite(body["centre"]).all()
    assert "moments 102400 102400 102400" in r.stdout, r.stdout
