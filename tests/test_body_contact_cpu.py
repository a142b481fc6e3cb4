"""The body's contact with the scenery on the CPU (pbf_set_collider_body_contact, csrc/pbf_body_contact.hpp): the float64
restatement tests/body_contact_ref.py — the reference tests/test_body_contact_gpu.py holds the device to — against the
stand-alone host program of the header (plain and under the sanitizers) bit for bit, against closed forms of the impulse,
and, for the surface points, against collider_ref's trilinear code and the geometry of a sphere; the mode owner's walk; the
rule that pbf_hip.hip changes the mode through its events only; and the two copies of the contract's text."""
import os
import re
import subprocess

import numpy as np
import pytest

import body_contact_ref as BC
import collider_body_ref as BR
import collider_pose_ref as PR
import collider_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pbf-sph_amd")
EPS = float(np.finfo(np.float64).eps)


def read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


# ---- 1. the host program against the restatement ---------------------------------------------------------------------------
def run_program(name):
    exe = os.path.join(PKG, name)
    assert os.path.exists(exe), "build() makes it"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, out[-4000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    return r.stdout.split("\n")


def words(tokens):
    return np.array([int(t, 16) for t in tokens], np.uint64)


@pytest.mark.parametrize("name", ["test_body_contact", "test_body_contact_san"])
def test_host_program_equals_the_restatement_bit_for_bit(name):
    """the header's resolve() — the text k_contact_resolve runs — on the sequences the program prints as hex words; the _san
    twin is the same stand-alone program under the address and undefined-behaviour sanitizers"""
    lines = run_program(name)
    cases, branches, b, c, case, passes = {}, {}, None, None, None, 0
    for line in lines:
        t = line.split()
        if not t:
            continue
        if t[0] == "case":
            p = words(t[2:]).view(np.float64)
            assert len(p) == 45
            b = BR.Body(mass=p[0], inertia=p[1:4], gain=p[4], linear_damping=p[5], angular_damping=p[6], accel=p[7:10],
                        linear_factor=p[10:13], angular_factor=p[13:16], centre_min=p[16:19], centre_max=p[19:22], rot=p[22:31],
                        centre=p[31:34], velocity=p[34:37], angular_velocity=p[37:40])
            c = BC.Contact(*p[40:45], points=1234)
            case = t[1]
            cases[case], branches[case] = 0, set()
        elif t[0] == "sums":
            s = words(t[1:9]).view(np.float64)
            c.resolve(b, s[0], s[1:4], s[4:7], s[7], int(t[9]))
            branches[case].add(c.branch)
        elif t[0] == "state":
            got = words(t[1:]).tobytes()
            want = b.state_words() + c.state_words()
            assert got == want, (name, case, cases[case], np.frombuffer(got, np.float64)[:45] - np.frombuffer(want, np.float64)[:45])
            cases[case] += 1
            passes += 1
    assert cases == {"no-points": 3, "approaching": 6, "separating": 4, "friction-slides": 4, "friction-sticks": 4, "locked-axes": 5,
                     "centre-bound": 3, "cancelling": 2, "non-finite": 4}, cases
    # both branches of the friction min ran, and the cases without friction took neither
    assert "slide" in branches["friction-slides"] and "stick" not in branches["friction-slides"], branches
    assert "stick" in branches["friction-sticks"], branches
    assert branches["approaching"] == {None} and branches["separating"] == {None}
    assert c.rejected == 3 and c.contacts == 1                          # (the last case)


def test_the_mode_owner_walk_and_every_refusal():
    lines = run_program("test_body_contact")
    assert sum(l.startswith("ok mode ") for l in lines) == 14
    seen = {l[len("refuse "):].split(": ")[0]: l.split(": ", 1)[1] for l in lines if l.startswith("refuse ")}
    assert set(seen) == {"non-finite level", "infinite friction", "zero stride", "negative skin", "restitution 1.5", "negative restitution",
                         "negative friction", "correction 1.01", "negative slop", "zero iterations", "nine iterations"}
    assert all("(accepted)" not in v for v in seen.values())


# ---- 2. closed forms of the impulse -------------------------------------------------------------------------------------------
def ball(**kw):
    d = dict(mass=3.5, inertia=(1400.0,) * 3, rot=PR.GENERIC[0], centre=(420.0, 310.0, 555.0), velocity=(30.0, 140.0, -12.0),
             angular_velocity=(0.4, -0.9, 0.2))
    d.update(kw)
    return BR.Body(**d)


@pytest.mark.parametrize("e", [0.0, 0.5, 1.0])
def test_sphere_on_a_plane_restitution(e):
    """A body with isotropic inertia against a plane of normal n, the averaged contact at r (not along n, so the impulse also
    turns the body).  The contact point's normal velocity after the pass is -e times the one before: un' = un + j kn by the
    definition of kn, and j kn = -(1 + e) un up to the roundings of j — three operations — and of the ~40 operations that form
    kn, apply j to v and w and form un' again, each relative to a term no larger than U = |v| + |w| |r| + |j| (1/m + |r|^2 /
    I).  The bar is 64 eps U.  And the change of w is parallel to r x n, the direction of the torque."""
    n = np.array([0.12, -0.98, 0.05])
    n /= np.linalg.norm(n)
    r = np.array([12.0, 60.0, -7.0])
    b = ball()
    v0, w0 = b.v.copy(), b.w.copy()
    un = float((v0 + np.cross(w0, r)) @ n)
    assert un < 0
    S = 40.0
    c = BC.Contact(skin=2.0, restitution=e, correction=0.0)
    c.resolve(b, S, S * n, S * r, 1.5, 30)
    un1 = float((b.v + np.cross(b.w, r)) @ n)
    j = float(c.impulse @ n)
    U = np.linalg.norm(v0) + np.linalg.norm(w0) * np.linalg.norm(r) + abs(j) * (1 / 3.5 + float(r @ r) / 1400.0)
    print(f"e = {e}: un {un:.6f} -> {un1:.6f}, |un' + e un| = {abs(un1 + e * un) / EPS:.1f} eps, bar {64 * U:.0f} eps")
    assert abs(un1 + e * un) <= 64 * EPS * U
    assert c.contacts == 1 and c.passes == 1 and np.array_equal(c.shift, np.zeros(3)) and j > 0
    dw, axis = b.w - w0, np.cross(r, n)
    assert np.linalg.norm(dw) > 0 and float(dw @ axis) > 0
    assert np.linalg.norm(np.cross(dw, axis)) <= 64 * EPS * np.linalg.norm(dw) * np.linalg.norm(axis)
    # the linear momentum the body received is the impulse
    assert np.abs(3.5 * (b.v - v0) - c.impulse).max() <= 16 * EPS * max(np.abs(c.impulse).max(), 3.5 * np.abs(v0).max())


def test_friction_never_reverses_the_slide_and_sticking_stops_it():
    """the contact straight below the centre of an isotropic body: r x n = 0, and (I^-1 (r x t)) x r = t |r|^2 / I lies along t,
    so the tangential impulse changes the slide along t alone and the sticking impulse lt / kt ends it"""
    n, r = np.array([0.0, -1.0, 0.0]), np.array([0.0, 50.0, 0.0])
    tangential = []
    for mu in (0.0, 0.01, 50.0):
        b = ball(angular_velocity=(0.0, 0.0, 0.0))
        c = BC.Contact(restitution=0.0, friction=mu, correction=0.0).resolve(b, 10.0, 10.0 * n, 10.0 * r, 1.0, 8)
        u = b.v + np.cross(b.w, r)
        tangential.append(float(np.linalg.norm(u - (u @ n) * n)))
        assert c.branch == {0.0: None, 0.01: "slide", 50.0: "stick"}[mu]
    assert tangential[0] > tangential[1] > tangential[2] and tangential[2] <= 1e-12 * tangential[0]


# ---- 3. the surface points ---------------------------------------------------------------------------------------------------
SPHERE = dict(centre=(85.0, 80.0, 78.0), radius=52.0, origin=(0.0, 0.0, 0.0), spacing=10.0, dims=(17, 17, 17))


def sphere_phi():
    return CR.lattice_of(lambda x: CR.sphere_phi(SPHERE["centre"], SPHERE["radius"], x), SPHERE["origin"], SPHERE["spacing"], SPHERE["dims"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_evaluate_is_collider_refs_trilinear_code(dtype):
    """with scale 1 and an unbounded box project() stores w + s g for a hit and returns phi: the same bits"""
    lat = CR.Lattice(sphere_phi(), SPHERE["origin"], SPHERE["spacing"], 3.0, dtype)
    fr = CR.frame(1.0, (-np.inf,) * 3, (np.inf,) * 3, dtype)
    rng = np.random.default_rng(5)
    q = (rng.random((20000, 3)) * 180.0 - 10.0).astype(dtype)
    phi, out, hit = CR.project(lat, fr, q)
    inside, hit2, s, g, phi2 = BC.evaluate(lat, q)
    assert np.array_equal(hit, hit2) and hit.sum() > 1000 and (~inside).sum() > 100
    assert np.array_equal(phi[inside], phi2[inside])
    moved = np.stack([q[:, a] + s * g[:, a] for a in range(3)], axis=1)
    assert moved.dtype == np.dtype(dtype) and np.array_equal(out[hit], moved[hit])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("stride", [1, 2])
def test_sphere_points_lie_on_the_sphere(dtype, stride):
    """Every point lies within a derived distance of the sphere.  With h the spacing and rho the least distance of a crossed
    cell from the centre (R - h sqrt 3 at the least), every second derivative of |x| - R is at most 1 / rho, so the trilinear
    interpolant is within e_phi = (h^2 / 8) (2 / rho) of it (the Hessian's trace is 2 / rho) and its gradient within e_g = (3 /
    2) h / rho per component.  The cell centre is at most delta = h sqrt(3) / 2 + e_phi from the level set, and the step of
    that length is taken along a direction off by at most theta = sqrt(3) e_g: the point misses the sphere by at most e_phi +
    delta theta, plus the rounding of N on coordinates of the lattice's size."""
    h, R = SPHERE["spacing"], SPHERE["radius"]
    pts = BC.points(sphere_phi(), SPHERE["origin"], h, 0.0, stride, dtype)
    rho = R - h * np.sqrt(3.0)
    e_phi = (h * h / 8.0) * (2.0 / rho)
    delta, theta = h * np.sqrt(3.0) / 2.0 + e_phi, np.sqrt(3.0) * 1.5 * h / rho
    bound = e_phi + delta * theta + 64 * float(np.finfo(dtype).eps) * 170.0
    miss = np.abs(np.linalg.norm(pts.astype(np.float64) - np.array(SPHERE["centre"]), axis=1) - R)
    print(f"{np.dtype(dtype).name} stride {stride}: {len(pts)} points, worst miss {miss.max():.4f}, bound {bound:.4f}")
    assert miss.max() <= bound
    # a crossed cell is a cell: no more points than strided cells, and a closed surface's worth of them
    cells = int(np.prod([len(range(0, d - 1, stride)) for d in SPHERE["dims"]]))
    assert 4 * np.pi * (R / (h * stride)) ** 2 / 4 < len(pts) < cells
    assert pts.dtype == np.dtype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_alternating_lattice_gives_one_point_per_cell(dtype):
    """phi(i, j, k) = 0.25 (-1)^i: every cell is crossed, its centre lies on the level set, and the point is the centre"""
    dims = (6, 5, 4)
    phi = np.broadcast_to((0.25 * (-1.0) ** np.arange(dims[0]))[:, None, None], dims).copy()
    pts = BC.points(phi, (-3.0, 2.0, 0.5), 2.0, 0.0, 1, dtype)
    assert len(pts) == 5 * 4 * 3
    want = np.stack(np.meshgrid(*[o + (np.arange(d - 1) + 0.5) * 2.0 for o, d in zip((-3.0, 2.0, 0.5), dims)], indexing="ij"), -1).reshape(-1, 3)
    assert np.array_equal(pts.astype(np.float64), want)                  # (cell-index order)
    assert len(BC.points(phi, (-3.0, 2.0, 0.5), 2.0, 0.0, 2, dtype)) == 3 * 2 * 2
    assert len(BC.points(phi, (-3.0, 2.0, 0.5), 2.0, 0.3, 1, dtype)) == 0   # (no node reaches the level)
    holed = phi.copy()
    holed[2, 1, 1] = np.inf                                             # (the eight cells around an infinite node drop out)
    assert len(BC.points(holed, (-3.0, 2.0, 0.5), 2.0, 0.0, 1, dtype)) == 60 - 8


def test_a_dropped_wave_or_partial_lands_outside_the_sum_bound():
    """the GPU test's bar for a raw sum is gamma_(p-1) sum|t| with p the number of terms (it holds for any order of summation);
    losing 64 terms (a wave's round) or 1024 (a partial record) of equal sign moves the sum by far more"""
    import math
    rng = np.random.default_rng(2)
    t = 1.0 + rng.random(274625)
    p = len(t)
    bar = (p - 1) * (EPS / 2) / (1 - (p - 1) * (EPS / 2)) * math.fsum(np.abs(t))
    exact = math.fsum(t)
    assert abs(float(np.sum(t)) - exact) <= bar and abs(float(np.cumsum(t)[-1]) - exact) <= bar
    assert abs(math.fsum(t[64:]) - exact) > 1e3 * bar and abs(math.fsum(np.delete(t, slice(2048, 3072))) - exact) > 1e3 * bar


# ---- 4. one owner for the mode, one text for the contract -----------------------------------------------------------------------
HPP = read(PKG, "csrc", "pbf_body_contact.hpp")
SRC = read(PKG, "csrc", "pbf_hip.hip")
HEADER = read(ROOT, "include", "pbf_hip.h")
MODE_FIELDS = re.findall(r"^  (?:bool|uint32_t|uint64_t|double) (\w+) = [-\w]+;", HPP, re.M)
ASSIGNMENT = r"[^\n]*\bcontact\s*\.\s*(?:%s)\b\s*(?:[-+*/|&^]|<<|>>)?=(?!=)[^\n]*"
STEPPED = r"[^\n]*(?:\+\+|--)\s*\w+(?:->|\.)contact\s*\.\s*\w+[^\n]*|[^\n]*\bcontact\s*\.\s*\w+\s*(?:\+\+|--)[^\n]*"


def test_the_header_has_no_hip_and_declares_the_fields_this_test_knows():
    assert set(MODE_FIELDS) == {"on", "points", "iterations", "stride", "level", "gen"}
    assert "#include <hip" not in HPP and "__device__" not in HPP and "__global__" not in HPP and "hip_runtime" not in HPP


def test_no_field_of_the_mode_is_assigned_outside_the_header():
    code = re.sub(r"//[^\n]*", "", SRC)
    pattern = ASSIGNMENT % "|".join(MODE_FIELDS)
    hits = re.findall(pattern, code) + re.findall(STEPPED, code)
    assert not hits, hits
    assert not re.search(r"(?:->|\.)contact\s*=(?!=)", code.replace("k.contact = ctx->contact.gen;", ""))
    assert len(re.findall(r"\bbodycontact::Mode contact;", code)) == 1 and len(re.findall(r"\bbodycontact::Mode\b", code)) == 1
    for f in MODE_FIELDS:
        assert not re.search(r"(?<!&)&(?!&)\s*\w+(?:->|\.)contact\s*\.\s*%s\b" % f, code), f
    # the three events are the only members called on it besides the questions
    called = set(re.findall(r"\bcontact\s*\.\s*(\w+)\s*\(", code))
    assert called == {"configured", "rewritten", "cleared", "same_points"}, called
    # the captured steps' key has a generation of its own for it
    key = re.search(r"struct GraphKey \{(.*?)\n\};", code, re.S).group(1)
    assert re.search(r"\buint64_t contact;", key) and re.search(r"k\.contact = ctx->contact\.gen;", code)
    # the regular expression sees an assignment
    for bad in ["ctx->contact.on = true;", "ctx->contact.points=n;", "c->contact . gen |= 1;", "ctx->contact.iterations += 1;"]:
        assert re.findall(pattern, bad), bad
    for bad in ["ctx->contact.gen++;", "++ctx->contact.gen;"]:
        assert re.findall(STEPPED, bad), bad
    for ok in ["if (ctx->contact.on) f();", "k.contact = ctx->contact.gen;", "a(ctx->contact.points == 3)", "ctx->contact.cleared();"]:
        assert not re.findall(pattern, ok) and not re.findall(STEPPED, ok), ok


def contract_lines(text, leader):
    """the lines of the contract from the detection's first to the response's last, without the comment leader"""
    lines = [l[len(leader):].rstrip() for l in text.split("\n") if l.startswith(leader)]
    first = next(k for k, l in enumerate(lines) if l.lstrip().startswith("passes += 1;"))
    last = next(k for k, l in enumerate(lines) if l.lstrip().startswith("pose.trans = x"))
    return lines[first:last + 1]


def test_the_header_and_the_hpp_state_the_same_contract():
    a, b = contract_lines(HPP, "//"), contract_lines(HEADER, " *")
    assert len(a) == 25 and a == b
    for text, leader in ((HPP, "//"), (HEADER, " *")):
        body = "\n".join(l[len(leader):] for l in text.split("\n") if l.startswith(leader))
        for line in ("r_a = (R[a][0] b_0 + R[a][1] b_1) + R[a][2] b_2        w_a = r_a + x_a",
                     "in contact  =  inside && hit && d > 0 && d finite",
                     "sums over the points in contact:  S = sum d,  M_a = sum m_a,  A_a = sum d * r_a,  D = max d,  count"):
            assert line in body, line
    # what is not built is said where the interface is
    for text in (HPP, HEADER):
        flat = " ".join(text.split())
        for phrase in ("box walls", "obstacle particles", "never rotates", "per-point manifold", "swept contact", "slab mode",
                       "receives no reaction"):
            assert phrase in flat.replace("// ", "").replace("* ", ""), phrase
