"""Collider friction through the layers above the C ABI (item 7 of tests/test_collider_friction_gpu.py's list): the C++ shim
(Solver::setColliderFriction / clearColliderFriction / colliderFrictionReaction through advance(),
host/test_collider_friction_shim.cpp) and `benchmark --collider-friction=mu ... --collider-friction-report` give the frames and
the sums of the same run over the C ABI, bit for bit."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import collider_pose_ref as PR
import collider_ref as CR
from test_collider_gpu import solver
from test_collider_pose_gpu import body_lattice_through, cli_pose

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pbf-sph_amd", "benchmark")
# the pose and the friction of host/test_collider_friction_shim.cpp
SHIM_POSE = (np.eye(3), np.array([500.0, 500.0, 500.0]))
SHIM_FRICTION = dict(mu=0.5, velocity=(60.0, 0.0, -25.0), angular_velocity=(0.1, -0.2, 0.4))


def test_shim(pkg, tmp_path):
    from pbf_sph_amd import capi
    frames = 4
    sc = pkg.scene_cubes(2048)
    lat, phi64, origin, _ = body_lattice_through(sc, np.float32, SHIM_POSE, 0.4)
    with open(tmp_path / "lattice.bin", "wb") as f:
        f.write(np.array(lat.dims, np.uint32).tobytes() + np.array(origin, np.float64).tobytes() +
                np.array([PR.BODY_SPACING, CR.MARGIN], np.float64).tobytes() + lat.phi.tobytes())
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_collider_friction_shim"), str(tmp_path / "lattice.bin"),
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
    s.set_collider(phi64, origin, PR.BODY_SPACING, CR.MARGIN).set_collider_pose(*SHIM_POSE).set_collider_friction(**SHIM_FRICTION)
    p = pkg.default_params(4, 1000.0)
    p.dt = float(np.float32(p.dt))                            # the shim's config holds dt in N
    st, size, slid = first, C.sizeof(capi.ColliderWrench), 0
    for k in range(frames):
        st = s.upload(**st).step(p).download()
        assert bytes(s.collider_friction_reaction(raw=True)) == raw[at:at + size], k
        slid += s.collider_friction_reaction()["hits"]
        at += size
    assert at == len(raw) and slid > 0
    for k in last:
        assert st[k].tobytes() == last[k].tobytes(), k


def test_cli_collider_friction_and_report(pkg, tmp_path):
    # the cubes lie in y <= 198 (gravity is +y): the plane y = 150 cuts through them; it slides along x and turns about y
    common = ["--scene", "cubes", "--particles", "2048", "--solver-iter", "4", "-n", "5", "-w", "0", "--resident", "--no-surface",
              "--collider=plane:0,-1,0,-150,13.5,50"]
    motion = (40.0, 0.0, -15.0, 0.0, 0.5, 0.0, 500.0, 150.0, 500.0)
    r = subprocess.run([BIN, *common, "--collider-friction=0.5", "--collider-motion=" + ",".join(repr(v) for v in motion),
                        "--collider-friction-report", "-o", str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.split("\n") if l.startswith('{"frame"')]
    assert [l["frame"] for l in lines] == [0, 1, 2, 3, 4] and all("friction" in l for l in lines)
    assert "Collider friction    : mu 0.5" in r.stdout
    # the same frames from Python: the CLI's lattice is the analytic plane, in double, on the box plus one spacing, rounded to N;
    # the pose of frame f is a turn by |w| f dt about the axis through the pivot, then v f dt, and the friction record holds the
    # velocity of the solid's point at the pose's t
    ax = -50.0 + np.arange(23, dtype=np.float64) * 50.0
    y = np.broadcast_to(ax[None, :, None], (23, 23, 23))
    phi = ((0.0 * ax[:, None, None] + -1.0 * y) + 0.0 * ax[None, None, :]) / 1.0 - -150.0
    s = solver(pkg, False).upload(**pkg.scene_cubes(2048))
    base = pkg.default_params(4, 1000.0)
    s.set_collider(phi, (-50.0,) * 3, 50.0, 13.5)
    v, w, pivot = np.array(motion[:3]), np.array(motion[3:6]), np.array(motion[6:])
    dt = float(np.float32(base.dt))                           # the driver's config holds dt in N
    slid = 0
    for frame, l in enumerate(lines):
        tau = frame * dt
        rot, trans = cli_pose(list(motion), frame, dt)
        d = np.array([trans[a] - (pivot[a] + v[a] * tau) for a in range(3)])
        vel = [v[0] + (w[1] * d[2] - w[2] * d[1]), v[1] + (w[2] * d[0] - w[0] * d[2]), v[2] + (w[0] * d[1] - w[1] * d[0])]
        s.set_collider_pose(rot, trans).set_collider_friction(0.5, vel, w)
        fr = s.step(pkg.apply_motion(base, frame, False)).collider_friction_reaction()
        got = l["friction"]
        for key in ("impulse", "angular", "abs_impulse", "abs_angular"):
            assert list(fr[key]) == got[key], (frame, key, fr[key], got[key])
        assert (fr["hits"], fr["particles"], fr["step"]) == (got["hits"], got["particles"], got["step"]) and fr["step"] == frame + 1
        slid += fr["hits"]
    assert slid > 0
    # every second frame; inf is accepted; refused with slabs; ignored without a collider; parse errors
    r = subprocess.run([BIN, *common, "--collider-friction=inf", "--collider-friction-report=2", "-o", str(tmp_path / "o2")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.split("\n") if l.startswith('{"frame"')]
    assert [l["frame"] for l in lines] == [1, 3] and "mu inf" in r.stdout and lines[-1]["friction"]["hits"] > 0
    r = subprocess.run([BIN, *common, "--collider-friction=0.5", "--slabs", "2", "-o", str(tmp_path / "o3")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0 and "single-device" in r.stderr
    r = subprocess.run([BIN, *common[:-1], "--collider-friction=0.5", "-o", str(tmp_path / "o4")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ignored" in r.stdout
    # (a parse error prints the reason and the usage and exits 0, as every parse error of the driver: nothing may have run)
    r = subprocess.run([BIN, *common, "--collider-friction=0.5,1", "-o", str(tmp_path / "o5")], capture_output=True, text=True, timeout=300)
    assert "--collider-friction: expected mu" in r.stderr and "Benchmark completed" not in r.stdout and '{"frame"' not in r.stdout
    for bad in ("0", "-1", "nan"):
        r = subprocess.run([BIN, *common, "--collider-friction=" + bad, "-o", str(tmp_path / "o6")], capture_output=True, text=True, timeout=300)
        assert "--collider-friction: mu must be > 0" in r.stderr and "Benchmark completed" not in r.stdout, bad
    h = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--collider-friction=" in h and "--collider-friction-report" in h
    # with a body: the body supplies the contact velocity and takes the kicks
    r = subprocess.run([BIN, *common[:-1], "--collider=sphere:300,250,300,80", "--collider-body=40", "--collider-friction=0.5",
                        "--collider-body-report=5", "--collider-friction-report=5", "-o", str(tmp_path / "o7")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [json.loads(l) for l in r.stdout.split("\n") if l.startswith('{"frame"')]
    body = [l for l in out if "body" in l][-1]["body"]
    assert body["steps"] == 5 and body["rejected"] == 0 and np.isfinite(body["centre"]).all() and [l for l in out if "friction" in l][-1]["friction"]["step"] == 5
