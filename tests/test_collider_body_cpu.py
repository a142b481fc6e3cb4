"""The collider's rigid body on the CPU (pbf_set_collider_body, csrc/pbf_collider_body.hpp): the float64 restatement
tests/collider_body_ref.py — the reference tests/test_collider_body_gpu.py holds the device to — against closed forms, the
impulse cases, the stand-alone host program of the header (plain and under the sanitizers) bit for bit, and the parameter
check."""
import os
import subprocess

import numpy as np
import pytest

import collider_body_ref as BR
import collider_pose_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)
DT = float(np.float32(0.0083))
K = 40


# ---- 1. closed forms over K advances --------------------------------------------------------------------------------------
def test_free_fall_closed_form():
    """zero sums: v_k = k dt a, x_k = x_0 + dt^2 a k (k + 1) / 2, within 4 k eps max|x| (two roundings per quantity per step,
    doubled)"""
    accel, x0 = np.array([0.0, 9800.0, -310.0]), np.array([420.0, 310.0, 555.0])
    b = BR.Body(3.5, (900.0, 1400.0, 2100.0), PR.GENERIC[0], x0, accel=accel)
    for k in range(1, K + 1):
        b.advance(DT, np.zeros(3), np.zeros(3))
        want = x0 + DT * DT * accel * (k * (k + 1) / 2.0)
        err = np.abs(b.x - want).max()
        assert err <= 4 * k * EPS * np.abs(want).max(), (k, err)
    print(f"free fall after {K} advances: error {err / EPS:.2f} eps, bar {4 * K * np.abs(want).max():.0f} eps")
    assert b.steps == K and b.rejected == 0 and np.array_equal(b.w, np.zeros(3))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_spin_about_a_principal_axis_closed_form(axis):
    """zero sums, w along a body axis of the identity start pose: each advance turns the body by exactly 2 atan(|w| dt / 2)
    (the normalised first-order update is a Cayley step), so k advances turn it by 2 k atan(|w| dt / 2), within 4 k eps rad"""
    w = np.zeros(3)
    w[axis] = 1.7
    b = BR.Body(3.5, (900.0, 1400.0, 2100.0), np.eye(3), (0.0, 0.0, 0.0), angular_velocity=w)
    for k in range(1, K + 1):
        b.advance(DT, np.zeros(3), np.zeros(3))
        angle = 2.0 * np.arctan2(b.q[1 + axis], b.q[0])
        want = 2.0 * k * np.arctan(1.7 * DT / 2.0)
        assert abs(angle - want) <= 4 * k * EPS, (k, angle - want)
        others = [b.q[1 + a] for a in range(3) if a != axis]
        assert others == [0.0, 0.0]
    print(f"spin about axis {axis} after {K} advances: angle error {abs(angle - want) / EPS:.2f} eps")
    assert np.array_equal(b.w, w) and np.array_equal(b.x, np.zeros(3))


def test_rotation_stays_orthonormal():
    """max |R^T R - I| stays below the pose check's 1e-5 after 2000 advances under a generic w, and every pose passes the check"""
    b = BR.Body(3.5, (900.0, 1400.0, 2100.0), PR.GENERIC[0], PR.GENERIC[1], angular_velocity=(2.3, -4.1, 1.2))
    worst = 0.0
    for k in range(2000):
        b.advance(DT, np.zeros(3), np.zeros(3))
        R = b.rot.reshape(3, 3)
        worst = max(worst, np.abs(R.T @ R - np.eye(3)).max())
        if k % 100 == 0:
            assert PR.pose_ok(*b.pose())
    print(f"max |R^T R - I| over 2000 advances: {worst:.3e}")
    assert worst < PR.ORTHO_BOUND and worst < 1e-13 and PR.pose_ok(*b.pose())


# ---- 2. impulse cases -----------------------------------------------------------------------------------------------------
def body(**kw):
    d = dict(mass=3.5, inertia=(900.0, 1400.0, 2100.0), rot=PR.GENERIC[0], centre=(420.0, 310.0, 555.0), velocity=(30.0, 0.0, -12.0),
             angular_velocity=(0.4, -0.9, 0.2), gain=0.49)
    d.update(kw)
    return BR.Body(**d)


def test_a_pure_impulse_changes_v_alone():
    P = np.array([0.012, -0.03, 0.007])
    b = body()
    v0, w0 = b.v.copy(), b.w.copy()
    b.advance(DT, P, np.zeros(3), 5)
    want = v0 - 0.49 * P / (3.5 * DT)
    assert np.abs(b.v - want).max() <= 4 * EPS * np.abs(want).max()
    assert np.array_equal(b.w, w0) and b.hits == 5 and np.array_equal(b.impulse, P)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_pure_angular_impulse_along_a_body_axis(axis):
    """L = l R e_b changes w by -gain l / (I_b dt) about R e_b"""
    R = PR.GENERIC[0]
    inertia = (900.0, 1400.0, 2100.0)
    e = R[:, axis]
    b = body()
    w0, v0 = b.w.copy(), b.v.copy()
    b.advance(DT, np.zeros(3), 2.5 * e)
    want = w0 - 0.49 * 2.5 / (inertia[axis] * DT) * e
    assert np.abs(b.w - want).max() <= 16 * EPS * max(np.abs(want).max(), 0.49 * 2.5 / (inertia[axis] * DT))
    assert np.array_equal(b.v, v0)
    other = body(inertia=tuple(i * (1.0 if a == axis else 7.0) for a, i in enumerate(inertia))).advance(DT, np.zeros(3), 2.5 * e)
    assert np.abs(other.w - want).max() <= 16 * EPS * max(np.abs(want).max(), 1.0)   # (the other moments do not enter)


def test_factors_of_zero_freeze_their_axes():
    P, L = np.array([0.012, -0.03, 0.007]), np.array([1.5, -2.5, 0.5])
    b = body(linear_factor=(0.0, 1.0, 0.0), angular_factor=(1.0, 0.0, 1.0), accel=(50.0, 9800.0, -70.0))
    x0 = b.x.copy()
    for _ in range(12):
        b.advance(DT, P, L)
        assert b.x[0].tobytes() == x0[0].tobytes() and b.x[2].tobytes() == x0[2].tobytes() and b.x[1] != x0[1]
        assert b.v[0] == 0 and b.v[2] == 0 and b.w[1] == 0 and b.w[0] != 0 and b.w[2] != 0
    frozen = body(linear_factor=(0.0,) * 3, angular_factor=(0.0,) * 3, rot=np.eye(3), accel=(50.0, 9800.0, -70.0))
    words = None
    for _ in range(12):
        frozen.advance(DT, P, L)
        pose = frozen.rot.tobytes() + frozen.x.tobytes() + frozen.q.tobytes()
        assert words in (None, pose)
        words = pose
    assert np.array_equal(frozen.rot.reshape(3, 3), np.eye(3)) and np.array_equal(frozen.x, x0)


def test_a_centre_bound_clamps_and_stops():
    b = body(accel=(0.0, 9800.0, 0.0), centre_max=(np.inf, 316.0, np.inf), centre_min=(419.9, -np.inf, -np.inf), velocity=(-30.0, 0.0, -12.0))
    clamped = [False, False]
    for _ in range(40):
        vy = b.v[1]
        b.advance(DT, np.zeros(3), np.zeros(3))
        assert 419.9 <= b.x[0] and b.x[1] <= 316.0
        if b.x[1] == 316.0:
            assert b.v[1] == 0.0
            clamped[1] = True
        if b.x[0] == 419.9:
            assert b.v[0] == 0.0
            clamped[0] = True
    assert clamped == [True, True] and b.v[2] == -12.0


def test_a_nan_sum_is_skipped_and_counted():
    a, b = body(accel=(0.0, 9800.0, 0.0)), body(accel=(0.0, 9800.0, 0.0))
    a.advance(DT, np.zeros(3), np.zeros(3))
    b.advance(DT, np.array([0.01, np.nan, 0.0]), np.array([1.0, 2.0, 3.0]))
    assert b.rejected == 1 and a.rejected == 0 and b.steps == 1
    for k in ("x", "q", "v", "w", "rot"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    b.advance(DT, np.array([1e308, 0.0, 0.0]), np.zeros(3))           # (the impulse overflows)
    b.advance(DT, np.zeros(3), np.array([0.0, 0.0, np.inf]))
    assert b.rejected == 3 and np.isfinite(np.concatenate([b.x, b.q, b.v, b.w])).all()


# ---- 3. the host program against the restatement ----------------------------------------------------------------------------
def run_program(name):
    exe = os.path.join(ROOT, "pbf-sph_amd", name)
    assert os.path.exists(exe), "build() makes it"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, out[-4000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    return r.stdout.split("\n")


def words(tokens):
    return np.array([int(t, 16) for t in tokens], np.uint64)


@pytest.mark.parametrize("name", ["test_collider_body", "test_collider_body_san"])
def test_host_program_equals_the_restatement_bit_for_bit(name):
    """the header's advance() — the text k_body_advance runs — on the sequences the program prints as hex words"""
    lines = run_program(name)
    cases, b, steps = {}, None, 0
    for line in lines:
        t = line.split()
        if not t:
            continue
        if t[0] == "case":
            w = words(t[2:]).view(np.float64)
            dt, p = w[0], w[1:]
            assert len(p) == 40
            b = BR.Body(mass=p[0], inertia=p[1:4], gain=p[4], linear_damping=p[5], angular_damping=p[6], accel=p[7:10],
                        linear_factor=p[10:13], angular_factor=p[13:16], centre_min=p[16:19], centre_max=p[19:22], rot=p[22:31],
                        centre=p[31:34], velocity=p[34:37], angular_velocity=p[37:40])
            cases[t[1]] = 0
            case = t[1]
        elif t[0] == "sums":
            s = words(t[1:7]).view(np.float64)
            b.advance(dt, s[:3], s[3:], int(t[7]))
        elif t[0] == "state":
            got = words(t[1:]).tobytes()
            want = b.state_words()
            assert got == want, (name, case, cases[case], np.frombuffer(got, np.float64)[:28] - np.frombuffer(want, np.float64)[:28])
            cases[case] += 1
            steps += 1
    assert set(cases) == {"free-fall", "spin-z", "tumble", "tumble-branch1", "tumble-branch2", "tumble-branch3", "frozen-axes",
                          "clamped", "rejected-sums"}, cases
    assert cases["free-fall"] == 40 and cases["spin-z"] == 40 and steps == 158
    assert b.rejected == 2                                    # (the last case: a NaN and an overflow)


def test_the_conversion_covers_every_branch():
    """R(q(R)) = R within a few eps where the trace is positive and where each diagonal entry leads"""
    for axis, angle in (((0.3, -0.5, 0.8), 0.7), ((1, 0.1, -0.05), 3.0), ((0.1, 1, 0.07), 3.1), ((-0.06, 0.1, 1), 2.9)):
        R = PR.rotation(axis, angle)
        q = BR.quaternion_of(R)
        assert abs(float(q @ q) - 1.0) <= 4 * EPS
        assert np.abs(BR.rotation_of(q).reshape(3, 3) - R).max() <= 16 * EPS, (axis, angle)


# ---- 4. the parameter check --------------------------------------------------------------------------------------------------
REFUSALS = {
    "non-finite mass": (dict(mass=np.nan), "non-finite parameter"),
    "NaN centre bound": (dict(centre_max=(np.inf, np.inf, np.nan)), "non-finite parameter"),
    "non-finite start velocity": (dict(angular_velocity=(0.0, np.inf, 0.0)), "non-finite start velocity"),
    "zero mass": (dict(mass=0.0), "mass <= 0"),
    "negative mass": (dict(mass=-1.0), "mass <= 0"),
    "zero inertia": (dict(inertia=(900.0, 0.0, 2100.0)), "inertia <= 0"),
    "negative gain": (dict(gain=-0.1), "gain < 0"),
    "negative linear damping": (dict(linear_damping=-1e-9), "damping < 0"),
    "negative angular damping": (dict(angular_damping=-2.0), "damping < 0"),
    "linear factor 0.5": (dict(linear_factor=(1.0, 1.0, 0.5)), "factor other than 0 or 1"),
    "angular factor -1": (dict(angular_factor=(-1.0, 1.0, 1.0)), "factor other than 0 or 1"),
    "centre_min > centre_max": (dict(centre_min=(5.0, -np.inf, -np.inf), centre_max=(4.0, np.inf, np.inf)), "centre_min > centre_max"),
    "reflected start pose": (dict(rot=np.diag([1.0, 1.0, -1.0]) @ PR.GENERIC[0]), "det rot < 0"),
    "sheared start pose": (dict(rot=PR.GENERIC[0] + 1e-4 * np.eye(3)[[1, 0, 2]] * [[1], [0], [0]]), "not a rotation"),
    "non-finite start centre": (dict(centre=(np.inf, 0.0, 0.0)), "non-finite entry in trans"),
}


def test_every_refusal_has_its_reason():
    """the host program's verdicts and reasons, and the restated check's on the same bodies"""
    lines = run_program("test_collider_body")
    seen = {l[len("refuse "):].split(": ")[0]: l.split(": ", 1)[1] for l in lines if l.startswith("refuse ")}
    assert set(seen) == set(REFUSALS), set(seen) ^ set(REFUSALS)
    for name, (kw, reason) in REFUSALS.items():
        assert reason in seen[name], (name, seen[name])
        verdict = BR.params_ok(**kw)
        assert verdict is not None and (verdict in reason or verdict == "pose"), (name, verdict)
    assert BR.params_ok() is None and BR.params_ok(gain=0.0, linear_factor=(0.0,) * 3, centre_min=(1.0,) * 3, centre_max=(1.0,) * 3) is None
    assert "ok refused a non-finite parameter anywhere" in lines and "ok accepted infinite centre bounds" in lines
