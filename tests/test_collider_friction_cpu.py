"""The collider friction on the CPU (pbf_set_collider_friction, csrc/pbf_collider_friction.hpp): the NumPy restatement
tests/collider_friction_ref.py — the reference tests/test_collider_friction_gpu.py holds the device to — against a float64
evaluation of the same formulas, the mutations it must tell apart, kick() against closed forms, the stand-alone host program
(plain and under the sanitizers) bit for bit, and the argument check."""
import os
import subprocess

import numpy as np
import pytest

import collider_body_ref as BR
import collider_friction_ref as FR
import collider_pose_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)
DT = float(np.float32(0.0083))
DTYPES = [np.float32, np.float64]


# ---- 1. the restatement in N against the same formulas in float64 ----------------------------------------------------------
def properties(dtype, seed, mu=1.0, mutation=None):
    """-> the worst of each property over the acting contacts of FR.contacts(seed), in FR.bar units' unit (eps_N * SPEED_UNIT):
    |un' - un|, |s' - max(0, s - mu jn)|, max(0, s' - s); un, s, jn, n and vb from the float64 evaluation of the contract on
    the same N inputs, un' and s' in float64 from the N result"""
    c = FR.contacts(dtype, seed)
    kw = dict(scale=FR.SCALE, dt=FR.DT, mu=mu, V=FR.V, W=FR.W, t=FR.T)
    got = FR.friction(dtype, vel=c["vel"], pos=c["pos"], A=c["A"], mutation=mutation, **kw)
    rounded = lambda x: np.asarray(x, np.float64).astype(dtype).astype(np.float64)       # (the kernel's inputs, exactly)
    kw64 = {k: rounded(v) for k, v in kw.items()}
    to64 = lambda k: float(kw64[k])
    ref = FR.friction(np.float64, vel=c["vel"].astype(np.float64), pos=c["pos"].astype(np.float64), A=c["A"].astype(np.float64), **kw64)
    act = ref["act"]
    assert act.sum() > 0.9 * len(act) and np.array_equal(act, got["act"])
    with np.errstate(all="ignore"):
        u = got["vel"].astype(np.float64) - ref["vb"]
        un = (u * ref["n"]).sum(axis=1)
        ut = u - un[:, None] * ref["n"]
        s = np.sqrt((ut * ut).sum(axis=1))
        want = np.maximum(0.0, ref["s"] - to64("mu") * ref["jn"])
    unit = float(np.finfo(dtype).eps) * FR.SPEED_UNIT
    clamped = (to64("mu") * ref["jn"] >= ref["s"])[act]
    return dict(normal=np.abs(un - ref["un"])[act].max() / unit, tangential=np.abs(s - want)[act].max() / unit,
                growth=np.maximum(0.0, s - ref["s"])[act].max() / unit, clamped=float(clamped.mean()), stuck=s[act][clamped].max() / unit if clamped.any() else 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_properties_against_float64(dtype):
    """On 2e5 random contacts: the pass leaves the normal relative speed alone, leaves the tangential relative speed at
    max(0, s - mu jn), never lets it grow, and with mu = inf leaves none.  The bar is 8 x the worst measured with this
    restatement on seed 1 (collider_friction_ref.FRICTION_WORST); other seeds must stay below it."""
    name = np.dtype(dtype).name
    bar = FR.bar_units(dtype)
    worst = {}
    for seed in (1, 2, 3):
        p = properties(dtype, seed)
        worst[seed] = max(p["normal"], p["tangential"], p["growth"])
        print(f"{name} seed {seed}: normal {p['normal']:.3f} tangential {p['tangential']:.3f} growth {p['growth']:.3f} "
              f"(eps * {FR.SPEED_UNIT:.0f}); stuck share {100 * p['clamped']:.1f} %; bar {bar:.2f}")
        assert 0.1 < p["clamped"] < 0.9                      # (both branches of the min are exercised)
        assert worst[seed] <= bar
    assert abs(worst[1] - FR.FRICTION_WORST[name]) <= 0.01 * FR.FRICTION_WORST[name], worst
    p = properties(dtype, 1, mu=np.inf)
    print(f"{name} mu = inf: normal {p['normal']:.3f} tangential left {p['stuck']:.3f}")
    assert p["clamped"] == 1.0 and p["stuck"] <= bar and p["normal"] <= bar and p["tangential"] <= bar


@pytest.mark.parametrize("mutation", FR.MUTATIONS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_mutations_are_told_apart(dtype, mutation):
    p = properties(dtype, 1, mutation=mutation)
    worst = max(p["normal"], p["tangential"], p["growth"])
    print(f"{np.dtype(dtype).name} {mutation}: worst {worst:.3e} units, bar {FR.bar_units(dtype):.2f}")
    assert worst >= 100.0 * FR.bar_units(dtype)


def test_a_lane_that_does_not_act_keeps_its_bits():
    for dtype in DTYPES:
        c = FR.contacts(dtype, 4)
        A = c["A"].copy()
        A[::3, 3] = 0                                        # never hit
        A[1::3, :3] = 0                                      # hit, but the displacements cancelled: no normal
        r = FR.friction(dtype, FR.SCALE, FR.DT, 0.5, FR.V, FR.W, FR.T, c["vel"], c["pos"], A)
        idle = ~r["act"]
        assert idle[::3].all() and idle[1::3].all() and r["act"][2::3].all()
        assert r["vel"][idle].tobytes() == c["vel"][idle].tobytes() and not r["dv"][idle].any()
        assert r["vel"].dtype == dtype and not FR.terms(np.ones(len(A)), FR.SCALE, r)[idle].any()


# ---- 2. kick() ---------------------------------------------------------------------------------------------------------------
def body(**kw):
    d = dict(mass=3.5, inertia=(900.0, 1400.0, 2100.0), rot=PR.GENERIC[0], centre=(420.0, 310.0, 555.0), velocity=(30.0, 0.0, -12.0),
             angular_velocity=(0.4, -0.9, 0.2), gain=0.49)
    d.update(kw)
    return BR.Body(**d)


def test_a_pure_linear_impulse_changes_v_alone():
    P = np.array([12.0, -30.0, 7.0])
    b = body()
    v0, w0, x0, q0 = b.v.copy(), b.w.copy(), b.x.copy(), b.q.copy()
    FR.kick(b, P, np.zeros(3))
    want = v0 - P / 3.5
    assert np.abs(b.v - want).max() <= 2 * EPS * np.abs(want).max()
    assert np.array_equal(b.w, w0) and np.array_equal(b.x, x0) and np.array_equal(b.q, q0) and b.steps == 0 and b.rejected == 0


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_moment_about_a_principal_axis_under_a_generic_pose(axis):
    """L = l R e_b changes w by -l / I_b about R e_b, whatever the other two moments"""
    R = PR.GENERIC[0]
    inertia = (900.0, 1400.0, 2100.0)
    e = R[:, axis]
    b = body()
    w0, v0 = b.w.copy(), b.v.copy()
    FR.kick(b, np.zeros(3), 2500.0 * e)
    want = w0 - 2500.0 / inertia[axis] * e
    assert np.abs(b.w - want).max() <= 16 * EPS * max(np.abs(want).max(), 2500.0 / inertia[axis])
    assert np.array_equal(b.v, v0)
    other = FR.kick(body(inertia=tuple(i * (1.0 if a == axis else 7.0) for a, i in enumerate(inertia))), np.zeros(3), 2500.0 * e)
    assert np.abs(other.w - want).max() <= 16 * EPS * max(np.abs(want).max(), 2500.0 / inertia[axis])


def test_factors_of_zero_freeze_their_axes():
    P, L = np.array([12.0, -30.0, 7.0]), np.array([1500.0, -2500.0, 500.0])
    b = body(linear_factor=(0.0, 1.0, 0.0), angular_factor=(1.0, 0.0, 1.0))
    v0, w0 = b.v.copy(), b.w.copy()
    FR.kick(b, P, L)
    assert b.v[0].tobytes() == v0[0].tobytes() and b.v[2].tobytes() == v0[2].tobytes() and b.v[1] != v0[1]
    assert b.w[1].tobytes() == w0[1].tobytes() and b.w[0] != w0[0] and b.w[2] != w0[2]


def test_a_non_finite_sum_is_skipped_and_counted():
    a, b = body(), body()
    for bad in ((np.array([0.01, np.nan, 0.0]), np.ones(3)), (np.ones(3), np.array([0.0, 0.0, np.inf])), (np.array([-np.inf, 0.0, 0.0]), np.zeros(3))):
        FR.kick(b, *bad)
    assert b.rejected == 3 and a.rejected == 0 and b.steps == 0
    assert a.state_words()[:28 * 8] == b.state_words()[:28 * 8]


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


@pytest.mark.parametrize("name", ["test_collider_friction", "test_collider_friction_san"])
def test_host_program_equals_the_restatement_bit_for_bit(name):
    """the header's kick() and advance() — the text k_body_kick_advance runs — on the sequences the program prints as hex words"""
    lines = run_program(name)
    cases, kicks, b = {}, 0, None
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
            case = t[1]
            cases[case] = 0
        elif t[0] == "kick":
            s = words(t[1:7]).view(np.float64)
            FR.kick(b, s[:3], s[3:])
            kicks += 1
        elif t[0] == "sums":
            s = words(t[1:7]).view(np.float64)
            b.advance(dt, s[:3], s[3:], int(t[7]))
        elif t[0] == "state":
            got, want = words(t[1:]).tobytes(), b.state_words()
            assert got == want, (name, case, cases[case], np.frombuffer(got, np.float64)[:28] - np.frombuffer(want, np.float64)[:28])
            cases[case] += 1
            if case == "rejected-kicks" and cases[case] == 8:
                assert b.rejected == 2                        # (a NaN and an infinity)
    assert cases == {"kick-every-step": 24, "kick-every-other-step": 12, "frozen-axes": 12, "rejected-kicks": 8, "linear-only": 6,
                     "angular-only": 6}, cases
    assert kicks == 24 + 6 + 12 + 8 + 6 + 6


# ---- 4. the argument check -----------------------------------------------------------------------------------------------------
REFUSALS = {
    "zero mu": (dict(mu=0.0), "mu <= 0 or NaN"),
    "negative mu": (dict(mu=-0.3), "mu <= 0 or NaN"),
    "NaN mu": (dict(mu=np.nan), "mu <= 0 or NaN"),
    "mu = -inf": (dict(mu=-np.inf), "mu <= 0 or NaN"),
    "infinite velocity": (dict(velocity=(30.0, np.inf, 0.0)), "non-finite velocity"),
    "NaN velocity": (dict(velocity=(30.0, -5.0, np.nan)), "non-finite velocity"),
    "infinite angular velocity": (dict(angular_velocity=(-np.inf, 0.0, 1.5)), "non-finite velocity"),
    "NaN angular velocity": (dict(angular_velocity=(0.0, 0.0, np.nan)), "non-finite velocity"),
}


def test_every_refusal_has_its_reason():
    """the host program's verdicts and reasons (the plain header, no device), and the restated check's on the same arguments"""
    lines = run_program("test_collider_friction")
    seen = {l[len("refuse "):].split(": ")[0]: l.split(": ", 1)[1] for l in lines if l.startswith("refuse ")}
    assert set(seen) == set(REFUSALS), set(seen) ^ set(REFUSALS)
    for name, (kw, reason) in REFUSALS.items():
        assert reason in seen[name], (name, seen[name])
        assert FR.args_ok(**kw) == reason, name
    assert FR.args_ok() is None and FR.args_ok(mu=np.inf) is None and FR.args_ok(mu=5e-324) is None
    assert "ok accepted stock" in lines and "ok accepted mu = inf" in lines and "ok accepted a denormal mu" in lines
