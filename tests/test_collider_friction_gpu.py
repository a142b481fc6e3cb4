"""Collider friction on the device (pbf_set_collider_friction, pbf_collider_friction_reaction, include/pbf_hip.h;
k_collider_friction, csrc/pbf_collider_friction.hpp):

  1. one step with friction = the restatement (tests/collider_friction_ref.py) applied to a twin's step with the reaction
     alone, bit for bit; positions, pStar and the records are the twin's;
  2. the sum at 65, 1 025 and 262 145 particles against a float64 sum of the per-particle terms;
  3. the device body with friction equals a host loop, bit for bit over 12 steps;
  4. every launch path gives the default path's bytes; batched and replayed steps give the eager bytes; no more captures than
     without friction; a rewritten record captures nothing; stage by stage = one pbf_step;
  5. off means off;
  6. physics without a fitted number, each against its frictionless twin: a sliding block, a rotating sphere, a spinning body;
  7. refusals leave everything unchanged.

The CPU side of the restatement: tests/test_collider_friction_cpu.py.
"""
import ctypes as C

import numpy as np
import pytest

import collider_body_ref as BR
import collider_friction_ref as FR
import collider_pose_ref as PR
import collider_ref as CR
from test_collider_body_gpu import body_bytes, differing, first_step_share, stock_body
from test_collider_gpu import ERR_INVALID, ERR_STATE, IDS, VARIANTS, dt_of, solver, state_bytes
from test_collider_pose_gpu import body_lattice_through, dense_block, install, wrench_bytes
from test_extras_paths_gpu import PATHS
from test_nversion_cpu import scene

pytestmark = pytest.mark.gpu

MU = 0.6
V, W = np.array([60.0, -35.0, 80.0]), np.array([0.3, -0.8, 0.5])         # a generic contact velocity, world units


def rubbed(pkg, sc, fp64, fast, case, pose=PR.GENERIC, path=None, mu=MU, v=V, w=W):
    """a ctx with the scene, the lattice under `pose` and friction on"""
    return install(solver(pkg, fp64, fast, path).upload(**sc), case, pose).set_collider_friction(mu, v, w)


def friction_bytes(s):
    return bytes(s.collider_friction_reaction(raw=True))


def everything(s):
    out = state_bytes(s)
    out["push"] = s.collider_push().tobytes()
    out["wrench"] = wrench_bytes(s)
    out["friction"] = friction_bytes(s)
    return out


def restated(twin, dtype, p, pose, mu=MU, v=V, w=W):
    """the restatement on the downloaded state of a twin that ran the same step with the reaction alone -> (result, download)"""
    d = twin.download()
    res = FR.friction(dtype, p.scale, p.dt, mu, v, w, pose[1], d["vel"], d["pos"], np.ascontiguousarray(twin.collider_push()[:, :4]))
    assert not res["act"][d["type"] != 0].any()                # (obstacles keep the sort's zero record)
    return res, d


# ---- 1. bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("name,path", [("edges1", None), ("edges65", None), ("cloud", None), ("cloud", dict(row_major=0)), ("obstacles", None)],
                         ids=["edges1", "edges65", "cloud", "cloud-morton", "obstacles"])
def test_one_step_equals_the_restatement(pkg, name, path, fp64, fast):
    """edges1: one moving particle that starts inside the posed solid (no neighbours, one hit per iteration); the issue's "one
    particle resting on a plane" is test_one_particle_resting_on_a_plane below; the default path keeps the records in row
    order (pushRows > 0), row_major = 0 in the Morton order"""
    dtype = dt_of(fp64)
    sc = scene(name)
    case = body_lattice_through(sc, dtype, PR.GENERIC, 0.15 if name == "edges65" else 0.5)
    if name != "edges1":
        share = first_step_share(sc, dtype, case, PR.GENERIC)
        print(f"{name}: {100 * share:.1f} % of the fluid starts inside the solid")
        assert 0.1 <= share <= 0.9, share
    p = pkg.default_params(4, 1000.0)
    twin = install(solver(pkg, fp64, fast, path).upload(**sc), case, PR.GENERIC, reaction=True).step(p)
    s = rubbed(pkg, sc, fp64, fast, case, path=path).step(p)
    res, want = restated(twin, dtype, p, PR.GENERIC)
    got = s.download()
    n_fluid = int((sc["type"] == 0).sum())
    print(f"{name}: {int(res['act'].sum())} of {n_fluid} in contact, {int(res['slide'].sum())} slid")
    assert res["slide"].any() and (name == "edges1" or 0.1 <= res["act"].sum() / n_fluid <= 0.9)
    assert got["vel"].tobytes() == res["vel"].tobytes(), int((got["vel"] != res["vel"]).any(axis=1).sum())
    assert got["vel"].tobytes() != want["vel"].tobytes()
    for k in ("id", "type", "mass", "pos", "colour"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert s.pstar().tobytes() == twin.pstar().tobytes() and s.collider_push().tobytes() == twin.collider_push().tobytes()
    assert wrench_bytes(s) == wrench_bytes(twin)
    fr = s.collider_friction_reaction()
    assert (fr["hits"], fr["particles"], fr["step"]) == (int(res["slide"].sum()), int(res["act"].sum()), 1)


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_one_particle_resting_on_a_plane(pkg, fp64, fast):
    """n = 1 as the issue names it: one particle at rest, 8.5 world units inside the margin of a horizontal plane lattice (no
    neighbours, one hit per iteration), no pose ever set (t = 0) — `edges1` above is a moving particle inside a posed solid"""
    dtype = dt_of(fp64)
    sc = dict(id=np.zeros(1, np.uint64), type=np.zeros(1, np.uint8), mass=np.ones(1), pos=np.array([[500.0, 489.0, 500.0]]),
              vel=np.zeros((1, 3)), colour=np.full((1, 4), 0.5))
    lat = plane_under_the_block(dtype)
    p = pkg.default_params(4, 1000.0)

    def make(friction):
        s = solver(pkg, fp64, fast).upload(**sc)
        s.set_collider(lat.phi.astype(np.float64), CR.BLOCK_LATTICE["origin"], CR.BLOCK_LATTICE["spacing"], CR.MARGIN)
        return s.set_collider_friction(MU, V, W) if friction else s.set_collider_reaction(True)

    twin, s = make(False).step(p), make(True).step(p)
    res, want = restated(twin, dtype, p, (np.eye(3), np.zeros(3)))
    rec = twin.collider_push()
    assert rec[0, 3] >= 1 and rec[0, 1] < 0 and res["slide"].all()
    got = s.download()
    assert got["vel"].tobytes() == res["vel"].tobytes() and got["vel"].tobytes() != want["vel"].tobytes()
    assert got["pos"].tobytes() == want["pos"].tobytes() and s.pstar().tobytes() == twin.pstar().tobytes()
    fr = s.collider_friction_reaction()
    assert (fr["hits"], fr["particles"], fr["step"]) == (1, 1, 1)
    terms = FR.terms(want["mass"], p.scale, res)
    assert list(fr["impulse"]) == list(terms[0, :3]) and list(fr["angular"]) == list(terms[0, 3:])


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_no_iterations_no_contact(pkg, fp64):
    """pbf_params.iteration == 0: no delta-p launch, the records are the sort's zeros (read in the Morton order), the pass
    acts on nobody, and the step is the one with the reaction alone"""
    sc = scene("cloud")
    case = body_lattice_through(sc, dt_of(fp64), PR.GENERIC)
    p = pkg.default_params(0, 1000.0)
    twin = install(solver(pkg, fp64).upload(**sc), case, PR.GENERIC, reaction=True).steps(p, 2)
    s = rubbed(pkg, sc, fp64, False, case).steps(p, 2)
    assert not differing(state_bytes(s), state_bytes(twin)) and not s.collider_push().any()
    fr = s.collider_friction_reaction()
    assert (fr["step"], fr["hits"], fr["particles"]) == (2, 0, 0)
    assert not any(np.abs(fr[k]).any() for k in ("impulse", "angular", "abs_impulse", "abs_angular"))


# ---- 2. the sum ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", [65, 1025, 262145])
def test_the_sum_equals_a_float64_sum_of_the_terms(pkg, n, fp64):
    """every particle inside the solid (test_collider_pose_gpu's item 7) with a start velocity across the push: a second wave
    round (65), a second workgroup (1 025) and the second 256-record round of the fold (262 145)"""
    dtype = dt_of(fp64)
    sc = dense_block(n)
    n_w = PR.GENERIC[0] @ np.array([1.0, 0.0, 0.0])
    tangent = np.cross(n_w, [0.0, 0.0, 1.0])
    sc["vel"] = np.tile(0.8 * tangent / np.linalg.norm(tangent), (n, 1))
    case = PR.body_plane_case(PR.GENERIC, dtype, n_w, 5000.0, dims=(41, 41, 41))
    assert case[1].max() < 0
    p = pkg.default_params(2, 1000.0)
    twin = install(solver(pkg, fp64).upload(**sc), case, PR.GENERIC, reaction=True).step(p)
    res, d = restated(twin, dtype, p, PR.GENERIC)
    outs = [friction_bytes(rubbed(pkg, sc, fp64, False, case).step(p)) for _ in range(2)]
    assert outs[0] == outs[1]                                 # bit-identical over two runs
    s = rubbed(pkg, sc, fp64, False, case).step(p)
    assert s.download()["vel"].tobytes() == res["vel"].tobytes()
    fr = s.collider_friction_reaction()
    assert fr["particles"] == n and fr["hits"] == n and fr["step"] == 1 and res["slide"].all()
    terms = FR.terms(d["mass"], p.scale, res)
    assert np.isfinite(terms).all() and np.abs(terms).max() > 0
    for key, cols in (("impulse", slice(0, 3)), ("angular", slice(3, 6))):
        tol = (n + 16) * 2.0 ** -53 * fr["abs_" + key]
        assert (np.abs(fr[key] - terms[:, cols].sum(axis=0)) <= tol).all(), (key, fr[key], terms[:, cols].sum(axis=0), tol)
        assert (np.abs(fr["abs_" + key] - np.abs(terms[:, cols]).sum(axis=0)) <= tol).all(), key
    # a further step in which nothing touches: the solid carried far away along its own normal
    s.set_collider_pose(PR.GENERIC[0], PR.GENERIC[1] + 1e5 * n_w).step(p)
    fr = s.collider_friction_reaction()
    assert (fr["step"], fr["hits"], fr["particles"]) == (2, 0, 0)
    assert not any(np.abs(fr[k]).any() for k in ("impulse", "angular", "abs_impulse", "abs_angular"))


# ---- 3. the body ---------------------------------------------------------------------------------------------------------------
def staged_step(s, p, between=None):
    s.stage("predict", p).stage("sort", p).stage("diffuse", p)
    for _ in range(int(p.iteration)):
        s.stage("lambda", p).stage("delta", p)
    if between:
        between()
    return s.stage("finalise", p)


@pytest.mark.parametrize("fp64", [True, False], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["cloud", "obstacles"])
def test_device_body_with_friction_equals_the_host_loop(pkg, name, fp64):
    """Twin A: a body and friction on, 12 x pbf_step.  Twin B has no body: the reaction and friction on and a pose set, and
    runs each step stage by stage, because the device pass of step k reads the body AFTER the step's advance while the
    step's delta-p launches read the pose from BEFORE it.  B's exact order per step:
      predict, sort, diffuse, K x (lambda, delta); pbf_collider_reaction;
      the restated kick with the friction sums of step k - 1 (none in step 0), the restated advance with this step's
      reaction sums; pbf_set_collider_pose(the new pose); pbf_set_collider_friction(mu, the new v, the new w);
      pbf_stage_finalise (which runs the pass); pbf_collider_friction_reaction -> the sums the next step's kick takes."""
    dtype = dt_of(fp64)
    sc = scene(name)
    ref = stock_body()
    case = body_lattice_through(sc, dtype, ref.pose())
    p = pkg.default_params(4, 1000.0)
    a = install(solver(pkg, fp64).upload(**sc), case).set_collider_body(**ref.kwargs()).set_collider_friction(MU)
    b = install(solver(pkg, fp64).upload(**sc), case, ref.pose(), reaction=True).set_collider_friction(MU, ref.v, ref.w)
    last, slid, kicked = None, 0, stock_body()
    for k in range(12):
        seen = {}

        def between():
            wr = b.collider_reaction(raw=True)
            seen["wr"] = bytes(wr)
            if last is not None:
                FR.kick(ref, last["impulse"], last["angular"])
            ref.advance(float(p.dt), list(wr.impulse), list(wr.angular), int(wr.hits))
            b.set_collider_pose(*ref.pose()).set_collider_friction(MU, ref.v, ref.w)

        staged_step(b, p, between)
        last = b.collider_friction_reaction()
        a.step(p)
        got, want = state_bytes(a), state_bytes(b)
        assert not differing(got, want), (k, differing(got, want))
        assert a.collider_push().tobytes() == b.collider_push().tobytes(), k
        assert body_bytes(a) == ref.state_words(), (k, a.collider_body_state(), ref.v, ref.w)
        assert wrench_bytes(a) == seen["wr"] and friction_bytes(a) == friction_bytes(b), k
        assert last["step"] == k + 1
        slid += last["hits"]
        # (the same reaction sums without the kicks: where the body would be had friction not reached it)
        wr = a.collider_reaction()
        kicked.advance(float(p.dt), wr["impulse"], wr["angular"], wr["hits"])
    assert slid > 0 and ref.rejected == 0 and ref.steps == 12
    assert kicked.state_words() != ref.state_words()


def coupled_step(a, b, ref, p, last):
    """one step of twin A (body and friction on the device) and of twin B (the staged host loop of the test above, `last` its
    friction sums of the step before or None), compared bit for bit -> B's friction sums of this step"""
    def between():
        wr = b.collider_reaction(raw=True)
        if last is not None:
            FR.kick(ref, last["impulse"], last["angular"])
        ref.advance(float(p.dt), list(wr.impulse), list(wr.angular), int(wr.hits))
        b.set_collider_pose(*ref.pose()).set_collider_friction(MU, ref.v, ref.w)

    staged_step(b, p, between)
    a.step(p)
    assert not differing(state_bytes(a), state_bytes(b)), differing(state_bytes(a), state_bytes(b))
    assert a.collider_push().tobytes() == b.collider_push().tobytes()
    assert body_bytes(a) == ref.state_words(), (a.collider_body_state(), ref.v, ref.w)
    assert friction_bytes(a) == friction_bytes(b)
    return b.collider_friction_reaction()


@pytest.mark.parametrize("fp64", [True, False], ids=["fp64", "fp32"])
def test_the_kick_survives_an_upload_that_grows_the_capacity(pkg, fp64):
    """The partial records of a pass outlive the step.  An upload of 6 000 particles over 100 regrows their buffer (7 records
    of 112 bytes against an allocation made for 2): the step after it must still kick the body with the sums of the pass
    before it, and the observer must still return them — both twins take the same uploads."""
    dtype = dt_of(fp64)
    large = dense_block(6000)
    small = {k: v[::60].copy() for k, v in large.items()}
    ref = stock_body()
    case = body_lattice_through(large, dtype, ref.pose())
    share = first_step_share(small, dtype, case, ref.pose())
    assert 0.1 <= share <= 0.9, share
    p = pkg.default_params(4, 1000.0)
    a = install(solver(pkg, fp64).upload(**small), case).set_collider_body(**ref.kwargs()).set_collider_friction(MU)
    b = install(solver(pkg, fp64).upload(**small), case, ref.pose(), reaction=True).set_collider_friction(MU, ref.v, ref.w)
    last = coupled_step(a, b, ref, p, None)                   # (the sparse set touches the solid in its first step only)
    assert last["hits"] > 0 and np.abs(last["impulse"]).max() > 0 and np.abs(last["angular"]).max() > 0
    before = friction_bytes(a)
    a.upload(**large), b.upload(**large)
    assert friction_bytes(a) == before and friction_bytes(b) == before
    unkicked = stock_body()
    unkicked.__dict__.update({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ref.__dict__.items()})
    most = 0
    for k in range(3):
        last = coupled_step(a, b, ref, p, last)
        most = max(most, last["particles"])
        if k == 0:                                            # (and the kick of that step was not a kick with zeros)
            wr = a.collider_reaction()
            unkicked.advance(float(p.dt), wr["impulse"], wr["angular"], wr["hits"])
            assert unkicked.state_words() != ref.state_words()
    assert last["step"] == 4 and most > 100 and ref.rejected == 0


@pytest.mark.parametrize("fp64", [True, False], ids=["fp64", "fp32"])
def test_a_body_placed_while_friction_is_on_starts_as_given(pkg, fp64):
    """friction first, some steps (their sums stay pending: no body consumes them), then pbf_set_collider_body, and a body that
    is re-placed: the first body stage after either call kicks with nothing — the sums were taken against another pose and
    other velocities — so the runs equal the host loop started with last = None"""
    dtype = dt_of(fp64)
    sc = scene("cloud")
    ref = stock_body()
    case = body_lattice_through(sc, dtype, ref.pose())
    p = pkg.default_params(4, 1000.0)
    a = rubbed(pkg, sc, fp64, False, case, pose=ref.pose()).steps(p, 2)
    b = rubbed(pkg, sc, fp64, False, case, pose=ref.pose()).steps(p, 2)
    pending = a.collider_friction_reaction()
    assert pending["hits"] > 0 and np.abs(pending["angular"]).max() > 0
    a.set_collider_body(**ref.kwargs())
    assert friction_bytes(a) == friction_bytes(b)             # (the observer still returns them)
    b.set_collider_pose(*ref.pose()).set_collider_friction(MU, ref.v, ref.w)
    last = None
    for _ in range(2):
        last = coupled_step(a, b, ref, p, last)
    assert last["hits"] > 0
    ref = stock_body(centre=PR.GENERIC[1] + np.array([4.0, -3.0, 2.0]), velocity=(0.0, 0.0, 0.0))
    a.set_collider_body(**ref.kwargs())
    b.set_collider_pose(*ref.pose()).set_collider_friction(MU, ref.v, ref.w)
    last = None
    for _ in range(2):
        last = coupled_step(a, b, ref, p, last)


# ---- 4. paths, batches, graphs, stages ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_every_path_gives_the_default_paths_bytes(pkg, fp64, fast):
    sc = scene("obstacles")
    case = body_lattice_through(sc, dt_of(fp64), PR.GENERIC)
    p = pkg.default_params(4, 1000.0)

    def run(path=None):
        s = rubbed(pkg, sc, fp64, fast, case, path=path)
        for _ in range(4):
            s.step(p)
        return s

    ref = run()
    want = everything(ref)
    assert ref.collider_friction_reaction()["hits"] > 0
    for path in PATHS + [dict(pipeline=1), dict(fuse_predict=0), dict(row_major=0, gather=0)]:
        got = everything(run(path))
        assert not differing(got, want), (path, differing(got, want))


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_coop_within_the_parity_tolerance(pkg, fp64):
    """coop = 2 changes the summation order: one step from a common state, <= 1e-3 world units (fp32) / 1e-9 (fp64), as
    test_hip_parity.test_wave_cooperative_reader_within_tolerance holds it without a collider"""
    sc = scene("obstacles")
    case = body_lattice_through(sc, dt_of(fp64), PR.GENERIC)
    p = pkg.default_params(4, 1000.0)
    st = rubbed(pkg, sc, fp64, False, case).steps(p, 3).download()
    outs = [rubbed(pkg, st, fp64, False, case, path=dict(coop=coop)).step(p) for coop in (0, 2)]
    d0, d1 = outs[0].download(), outs[1].download()
    assert np.array_equal(d0["id"], d1["id"])
    d = np.linalg.norm(d0["pos"].astype(np.float64) - d1["pos"].astype(np.float64), axis=1)
    print(f"coop 2 vs 0: largest distance {d.max():.3e} world units")
    assert d.max() <= (1e-9 if fp64 else 1e-3), d.max()
    assert outs[1].collider_friction_reaction()["hits"] > 0


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_batched_and_graphed_steps_give_the_eager_bytes(pkg, fp64, fast):
    sc = scene("cloud")
    case = body_lattice_through(sc, dt_of(fp64), PR.GENERIC)
    p = pkg.default_params(4, 1000.0)
    eager = rubbed(pkg, sc, fp64, fast, case)
    slid = 0
    for _ in range(6):
        slid += eager.step(p).collider_friction_reaction()["hits"]
    want = everything(eager)
    assert slid > 0
    fused = rubbed(pkg, sc, fp64, fast, case, path=dict(graph=0)).steps(p, 6)
    assert not differing(everything(fused), want), differing(everything(fused), want)
    assert fused.graph_stats()[1] == 0
    graphed = rubbed(pkg, sc, fp64, fast, case, path=dict(graph=1)).steps(p, 6)
    assert not differing(everything(graphed), want), differing(everything(graphed), want)
    plain = install(solver(pkg, fp64, fast, dict(graph=1)).upload(**sc), case, PR.GENERIC, reaction=True).steps(p, 6)
    g, c = graphed.graph_stats(), plain.graph_stats()
    print(f"graphs: friction {g}, reaction alone {c}")
    assert 0 < g[0] <= c[0] and g[1] > 0 and g[2], (g, c)
    assert state_bytes(plain)["vel"] != want["vel"]
    # another mu and another contact velocity between two batches capture nothing, and the next batch runs with them
    graphed.set_collider_friction(2.0 * MU, -V, 0.5 * W).steps(p, 6)
    g2 = graphed.graph_stats()
    assert g2[0] == g[0] and g2[1] > g[1], (g, g2)
    eager.set_collider_friction(2.0 * MU, -V, 0.5 * W)
    for _ in range(6):
        eager.step(p)
    assert not differing(everything(graphed), everything(eager))
    assert everything(eager)["vel"] != want["vel"]


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_stage_by_stage_equals_one_step(pkg, fp64, fast):
    sc = scene("obstacles")
    case = body_lattice_through(sc, dt_of(fp64), PR.GENERIC)
    p = pkg.default_params(4, 1000.0)
    whole, staged = rubbed(pkg, sc, fp64, fast, case), rubbed(pkg, sc, fp64, fast, case)
    for _ in range(2):
        whole.step(p)
        staged_step(staged, p)
        assert not differing(everything(staged), everything(whole))
    assert whole.collider_friction_reaction()["hits"] > 0 and whole.collider_friction_reaction()["step"] == 2
    # with a body as well: pbf_stage_body consumes the pass's sums once, as the step does
    ref = stock_body()
    whole = install(solver(pkg, fp64, fast).upload(**sc), case).set_collider_body(**ref.kwargs()).set_collider_friction(MU)
    staged = install(solver(pkg, fp64, fast).upload(**sc), case).set_collider_body(**ref.kwargs()).set_collider_friction(MU)
    for _ in range(3):
        whole.step(p)
        staged_step(staged, p, lambda: staged.stage("body", p))
        assert not differing(everything(staged), everything(whole)) and body_bytes(staged) == body_bytes(whole)


# ---- 5. off means off -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_friction_set_and_cleared_is_friction_never_set(pkg, fp64, fast):
    from pbf_sph_amd import capi
    sc = scene("cloud")
    case = body_lattice_through(sc, dt_of(fp64), PR.GENERIC)
    p = pkg.default_params(4, 1000.0)
    never = install(solver(pkg, fp64, fast).upload(**sc), case, PR.GENERIC, reaction=True).steps(p, 6)
    s = rubbed(pkg, sc, fp64, fast, case)
    s.set_collider_friction(None).set_collider_friction(None)
    assert s.L.pbf_collider_friction_reaction(s.ctx, C.byref(capi.ColliderWrench())) == ERR_STATE
    s.steps(p, 6)
    assert not differing(state_bytes(s), state_bytes(never)) and s.collider_push().tobytes() == never.collider_push().tobytes()
    assert wrench_bytes(s) == wrench_bytes(never) and s.collider_reaction()["hits"] > 0
    # turned off after some steps: from there on the steps of a ctx that only has the reaction
    b = rubbed(pkg, sc, fp64, fast, case).steps(p, 3)
    c = install(solver(pkg, fp64, fast).upload(**b.download()), case, PR.GENERIC, reaction=True).steps(p, 3)
    b.set_collider_friction(None).steps(p, 3)
    assert not differing(state_bytes(b), state_bytes(c))
    assert state_bytes(b)["vel"] != state_bytes(never)["vel"]


# ---- 6. physics without a fitted number ---------------------------------------------------------------------------------------
def plane_under_the_block(dtype):
    """the horizontal plane y = 494 (gravity is +y; the solid is beyond it), 5 world units under the lowest layer of
    collider_ref.block_scene: with the margin of 13.5 that layer starts 8.5 inside"""
    lat, _ = CR.plane_case(dtype, -494.0, normal=(0.0, -1.0, 0.0), **CR.BLOCK_LATTICE)
    return lat


def tangential(dtype, vel, A, scale):
    """float64 |v - (v.n) n| of every particle with a record, n = A / |A| (the plane stands still: the relative velocity is v)"""
    a = A[:, :3].astype(np.float64)
    act = (A[:, 3] > 0) & ((a * a).sum(axis=1) > 0)
    n = a[act] / np.sqrt((a[act] * a[act]).sum(axis=1))[:, None]
    v = vel[act].astype(np.float64)
    t = v - (v * n).sum(axis=1)[:, None] * n
    return act, np.sqrt((t * t).sum(axis=1))


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_plane_a_sliding_block_is_slowed(pkg, fp64):
    """(a) the block of collider_ref.block_scene slides along x on a horizontal plane.  Per step, a twin with the reaction
    alone takes the same step from the same state (friction acts after finalise: up to the pass the two are the same step),
    so its velocity is the friction run's velocity before the pass."""
    dtype = dt_of(fp64)
    sc = CR.block_scene()
    sc["vel"] = np.tile([1.0, 0.0, 0.0], (len(sc["id"]), 1))
    lat = plane_under_the_block(dtype)
    p = pkg.default_params(4, 1000.0)
    ident = (np.eye(3), np.zeros(3))

    def make(mu):
        s = solver(pkg, fp64).upload(**sc)
        s.set_collider(lat.phi.astype(np.float64), CR.BLOCK_LATTICE["origin"], CR.BLOCK_LATTICE["spacing"], CR.MARGIN)
        return s.set_collider_reaction(True) if mu is None else s.set_collider_friction(mu)

    free = make(None).steps(p, 10).download()
    px = {}
    for mu in (MU, np.inf):
        s, before, contacts = make(mu), make(None), 0
        for k in range(10):
            state = s.download()
            s.step(p)
            pre = before.upload(**state).step(p).download()
            got = s.download()
            assert got["pos"].tobytes() == pre["pos"].tobytes() and s.collider_push().tobytes() == before.collider_push().tobytes(), k
            act, t0 = tangential(dtype, pre["vel"], before.collider_push(), p.scale)
            _, t1 = tangential(dtype, got["vel"], s.collider_push(), p.scale)
            contacts += int(act.sum())
            assert (t1 <= t0 + FR.bar_speed(dtype)).all(), (k, (t1 - t0).max())
            if mu == np.inf and act.any():
                assert t1.max() <= FR.bar_speed(dtype), (k, t1.max(), FR.bar_speed(dtype))
            assert got["vel"][~act].tobytes() == pre["vel"][~act].tobytes()
        assert contacts > 0
        px[mu] = float((got["mass"].astype(np.float64) * got["vel"][:, 0].astype(np.float64)).sum())
    twin = float((free["mass"].astype(np.float64) * free["vel"][:, 0].astype(np.float64)).sum())
    print(f"{np.dtype(dtype).name}: sum m v_x after 10 steps: {twin:.4f} free-slip, {px[MU]:.4f} with mu = {MU}, {px[np.inf]:.4f} no-slip")
    assert 0 < px[MU] < twin and 0 < px[np.inf] < twin, (px, twin)


BALL = dict(origin=(-100.0,) * 3, spacing=20.0, dims=(11, 11, 11))
RADIUS = 60.0
CENTRE = np.array([494.5, 394.5, 494.5])                      # the middle of collider_ref.block_scene


def blob_with_ball(pkg, fp64):
    """the block at rest, no gravity, and a ball lattice in the body frame (centre at the frame's origin) in its middle"""
    s = solver(pkg, fp64).upload(**CR.block_scene())
    phi = pkg.sdf_lattice(pkg.sdf_sphere((0.0, 0.0, 0.0), RADIUS), BALL["origin"], BALL["spacing"], BALL["dims"])
    p = pkg.default_params(4, 1000.0)
    p.constant_force[:] = [0.0, 0.0, 0.0]
    return s.set_collider(phi, BALL["origin"], BALL["spacing"], CR.MARGIN), p


def fluid_lz(s):
    d = s.download()
    r = d["pos"].astype(np.float64) - CENTRE
    v = d["vel"].astype(np.float64)
    return float((d["mass"].astype(np.float64) * (r[:, 0] * v[:, 1] - r[:, 1] * v[:, 0])).sum())


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["ccw", "cw"])
@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_a_rotating_sphere_drags_the_fluid_round(pkg, fp64, sign):
    """(b) a ball turning about z in a resting blob: the lattice it reads is the same under every pose, so without friction the
    fluid gains no angular momentum about the axis beyond rounding; with friction it gains some, with the sign of W"""
    wz = sign * 2.0
    lz, slid = {}, 0
    for on in (True, False):
        s, p = blob_with_ball(pkg, fp64)
        for k in range(8):
            s.set_collider_pose(PR.rotation((0.0, 0.0, 1.0), wz * k * float(p.dt)), CENTRE)
            if on:
                s.set_collider_friction(MU, (0.0, 0.0, 0.0), (0.0, 0.0, wz))
            s.step(p)
            if on:
                slid += s.collider_friction_reaction()["hits"]
        lz[on] = fluid_lz(s)
    print(f"{'fp64' if fp64 else 'fp32'} W_z = {wz}: fluid L_z about the axis {lz[True]:.6e} with friction, {lz[False]:.6e} without")
    assert slid > 0 and lz[True] * sign > 0 and abs(lz[True]) > abs(lz[False]), lz


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
def test_a_spinning_body_spins_down(pkg, fp64):
    """(c) a ball body with a frozen centre spinning about z in the blob: the kick of step k + 1 hands it the friction sums of
    step k, so w_z goes down in every step that follows a pass with a contact; without friction it only drifts (trilinear
    normals are not exactly radial)"""
    mass = 20000.0                                            # (heavy: the damped fluid never overtakes its surface)
    body = dict(mass=mass, inertia=(0.4 * mass * RADIUS ** 2,) * 3, rot=np.eye(3), centre=CENTRE, angular_velocity=(0.0, 0.0, 3.0),
                linear_factor=(0.0,) * 3)
    wz, drops = {}, 0
    for on in (True, False):
        s, p = blob_with_ball(pkg, fp64)
        s.set_collider_body(**body)
        if on:
            s.set_collider_friction(MU)
        w, slid = [3.0], 0
        for k in range(12):
            s.step(p)
            w.append(float(s.collider_body_state()["angular_velocity"][2]))
            if on:
                if slid:
                    assert w[-1] < w[-2], (k, w)
                    drops += 1
                slid = s.collider_friction_reaction()["hits"]
        assert s.collider_body_state()["rejected"] == 0
        wz[on] = w
    drop, drift = 3.0 - wz[True][-1], abs(3.0 - wz[False][-1])
    print(f"{'fp64' if fp64 else 'fp32'}: w_z fell by {drop:.6e} in 12 steps with friction ({drops} kicks); frictionless drift {drift:.3e}")
    assert drops > 0 and drop > drift and wz[True][-1] > 0, (wz, drops)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_unchanged(pkg):
    from pbf_sph_amd import capi
    from test_collider_friction_cpu import REFUSALS
    sc = scene("cloud")
    case = body_lattice_through(sc, np.float32, PR.GENERIC)
    p = pkg.default_params(4, 1000.0)

    def arg(mu=MU, velocity=V, angular_velocity=W):
        f = capi.ColliderFriction()
        f.mu = float(mu)
        f.velocity[:], f.angular_velocity[:] = [float(x) for x in velocity], [float(x) for x in angular_velocity]
        return f

    s = solver(pkg, False, path=dict(graph=1)).upload(**sc)
    L = s.L
    wr = capi.ColliderWrench()
    assert L.pbf_set_collider_friction(s.ctx, C.byref(arg())) == ERR_STATE and b"no collider" in L.pbf_last_error(s.ctx)
    assert L.pbf_set_collider_friction(s.ctx, None) == ERR_STATE
    assert L.pbf_collider_friction_reaction(s.ctx, C.byref(wr)) == ERR_STATE
    install(s, case, PR.GENERIC).set_collider_friction(MU, V, W)
    assert L.pbf_collider_friction_reaction(s.ctx, C.byref(wr)) == ERR_STATE and b"no step" in L.pbf_last_error(s.ctx)
    s.steps(p, 4)
    before, graphs = everything(s), s.graph_stats()
    assert s.collider_friction_reaction()["step"] == 4 and graphs[0] > 0

    for what, (kw, reason) in REFUSALS.items():
        assert L.pbf_set_collider_friction(s.ctx, C.byref(arg(**kw))) == ERR_INVALID, what
        assert reason.encode() in L.pbf_last_error(s.ctx), (what, L.pbf_last_error(s.ctx))
    assert L.pbf_collider_friction_reaction(s.ctx, None) == ERR_INVALID
    assert L.pbf_set_collider_reaction(s.ctx, 0) == ERR_STATE and b"friction" in L.pbf_last_error(s.ctx)
    assert L.pbf_set_collider_reaction(s.ctx, 1) == 0
    assert everything(s) == before and s.graph_stats()[0] == graphs[0]
    # and the next steps are the ones an undisturbed twin takes, replayed from the graphs captured before
    twin = rubbed(pkg, sc, False, False, case, path=dict(graph=1)).steps(p, 4).steps(p, 2)
    assert not differing(everything(s.steps(p, 2)), everything(twin))
    assert s.graph_stats()[0] == twin.graph_stats()[0]

    # a new collider, clearing included, turns friction off
    lat, phi64, origin, _ = case
    s.set_collider(phi64, origin, PR.BODY_SPACING, CR.MARGIN)
    assert L.pbf_collider_friction_reaction(s.ctx, C.byref(wr)) == ERR_STATE and b"off" in L.pbf_last_error(s.ctx)
    assert L.pbf_set_collider_reaction(s.ctx, 0) == 0
    s.set_collider_friction(MU).set_collider(None)
    assert L.pbf_collider_friction_reaction(s.ctx, C.byref(wr)) == ERR_STATE
    free = solver(pkg, False).upload(**s.download()).step(p)
    assert state_bytes(s.step(p)) == state_bytes(free)        # (and the step is the one without a collider)

    # slab mode: refused on a configured ctx
    u = install(solver(pkg, False).upload(**sc), case, PR.GENERIC).step(p)
    cut = capi.SlabCut(0, 12, 0, 0)
    assert L.pbf_slab_configure(u.ctx, C.byref(cut), 0, 0) == 0
    assert L.pbf_set_collider_friction(u.ctx, C.byref(arg())) == ERR_STATE and b"slab" in L.pbf_last_error(u.ctx)
    assert L.pbf_set_collider_friction(u.ctx, None) == ERR_STATE
    assert L.pbf_collider_friction_reaction(u.ctx, C.byref(wr)) == ERR_STATE
    s.close()
    u.close()
