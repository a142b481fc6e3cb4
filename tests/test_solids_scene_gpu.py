"""Sources and drains with the solids on: the scene stage (pbf_set_sources / pbf_set_drains, include/pbf_hip.h) changes n at
the top of every step while the collider's reaction records, the rigid body, the friction pass's pending sums, the scenery
and the body's contact with it keep state from one step to the next.

The method is a host-sequenced twin.  Run D is the product path: the solids, the sources and the drains installed, FRAMES
times pbf_steps(p, 1).  Run T has the same solids and no scene: before every step the host downloads it, applies
scene_cases.np_emit and np_drain in the ctx's dtype (the CPU suite holds them to the oracle), uploads the result and calls
pbf_step.  The header lets the pose, the body record, the contact record and pending friction sums outlive an upload, so T
is a legal run, and after every frame D and T must agree byte for byte on every downloaded field, pStar, the reaction
records, the raw reaction sums, the raw friction sums, the raw body state and the raw contact state.  The per-particle
arithmetic of each feature is pinned by its own file; this one pins that the scene stage composes with it.  include/pbf_hip.h
names no field of those records that restarts at an upload (the reaction's `step` counts sorts since the reaction was enabled,
the friction's passes since friction was turned on, the body's and the contact's counters since they were set), so nothing is
excluded from the comparison.

  1. D == T over six frames in four solid configurations, and what the scene must show for that to mean something;
  2. drains only: the count of partial records falls between a friction pass and the next body stage;
  3. one pbf_steps(p, 6) gives the bytes of frame 6;
  4. graph = 1: nothing is captured while a scene is set; after it is cleared the steps are captured, replayed and equal the eager ones;
  5. the other launch paths give the default path's bytes;
  6. depletion: while n == 0 neither the body nor the friction pass moves, and the pending kick is consumed exactly once after;
  7. capacity: a step that would exceed it fails before anything is launched and leaves every byte as it was.

The geometry and the host arithmetic are checked without a device by tests/test_solids_composed_cpu.py.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import body_contact_ref as BC
import collider_friction_ref as FR
import collider_pose_ref as PR
import scene_cases as S
import solids_scene_cases as SS
from test_body_contact_gpu import contact_bytes
from test_collider_body_gpu import body_bytes, stock_body
from test_collider_friction_gpu import MU, V, W, everything
from test_collider_gpu import ERR_INVALID, IDS, VARIANTS, dt_of, plane_through, solver
from test_collider_pose_gpu import body_lattice_through, install
from test_scenery_gpu import everything as everything_but_friction
from test_scenery_gpu import set_scenery

pytestmark = pytest.mark.gpu

CONFIGS = ["reaction", "scenery", "friction", "body"]        # (a) .. (d) of the module's item 1
# (d)'s contact: the collider's plane crosses the scenery's wall deep inside the box, so only a little of the depth is
# corrected per step and the solid stays where the fluid is
CONTACT = dict(skin=6.0, restitution=0.3, friction=0.4, correction=0.02, slop=0.5)


def solids(pkg, sc, fp64, fast, config, base=None, path=None, reserve=SS.RESERVE):
    """a ctx with `sc` uploaded and the solids of `config`; the collider's plane and the scenery's wall are laid through `base`"""
    dtype = dt_of(fp64)
    base = sc if base is None else base
    case = body_lattice_through(base, dtype, PR.GENERIC, SS.SHARE)
    s = solver(pkg, fp64, fast, path)
    if reserve:
        s.reserve(reserve)
    s.upload(**sc)
    if config == "body":
        install(s, case).set_collider_body(**stock_body().kwargs()).set_collider_friction(MU)
    else:
        install(s, case, PR.GENERIC, reaction=True)
    if config != "reaction":
        set_scenery(s, plane_through(base, dtype, SS.WALL_SHARE, SS.WALL_N)[1])
    if config == "friction":
        s.set_collider_friction(MU, V, W)
    if config == "body":
        s.set_collider_body_contact(**CONTACT)
    return s


def records_of(s, config):
    """the raw records that do not depend on the particle arrays being current"""
    out = {}
    if config in ("friction", "body"):
        out["friction"] = bytes(s.collider_friction_reaction(raw=True))
    if config == "body":
        out["body"], out["contact"] = body_bytes(s), contact_bytes(s)
    return out


def snapshot(s, config):
    """every downloaded field, pStar, the reaction records and their raw sums, and the raw records of `config`"""
    out = everything(s) if config in ("friction", "body") else everything_but_friction(s)
    out.update(records_of(s, config))
    out["n"] = s.n
    return out


def differing(got, want):
    return [k for k in want if got[k] != want[k]]


def host_scene(t, sources, drains, dtype):
    """the scene stage on the host: download, np_emit, np_drain -> (the set to upload, particles emitted, particles drained,
    mask of the downloaded particles that left)"""
    st = t.download()
    n0 = len(st["id"])
    grown = S.np_emit(st, sources, dtype) if sources else st
    kept = S.np_drain(grown, drains, dtype) if drains else grown
    gone = np.ones(len(grown["id"]), bool)
    # (np_drain is a stable erase: what is left is a subsequence, found again by walking both)
    j = 0
    for i in range(len(grown["id"])):
        if j < len(kept["id"]) and all(grown[k][i].tobytes() == kept[k][j].tobytes() for k in ("id", "pos", "vel")):
            gone[i] = False
            j += 1
    assert j == len(kept["id"])
    return kept, len(grown["id"]) - n0, len(grown["id"]) - len(kept["id"]), gone[:n0]


def acted(push):
    """the friction pass's `act` of every particle, from the step's reaction records (include/pbf_hip.h: A.w > 0 && len > 0)"""
    a = push[:, :3].astype(np.float64)
    return (push[:, 3] > 0) & ((a * a).sum(axis=1) > 0)


def run_twins(pkg, sc, fp64, fast, config, sources, drains, frames, base=None, first_without_scene=False):
    """D and T frame by frame, compared after each -> (D's snapshot of the last frame, per-frame facts)"""
    dtype = dt_of(fp64)
    p = pkg.default_params(4, 1000.0)
    d, t = solids(pkg, sc, fp64, fast, config, base), solids(pkg, sc, fp64, fast, config, base)
    facts = dict(n=[], emitted=[], drained=[], drained_after_act=0, born_pushed=0)
    act = None
    for frame in range(frames):
        scene_on = not (first_without_scene and frame == 0)
        if scene_on and frame == int(first_without_scene):
            d.set_sources(sources).set_drains(drains)
        if scene_on:
            st, emitted, drained, gone = host_scene(t, sources, drains, dtype)
            if act is not None:
                facts["drained_after_act"] += int((gone & act).sum())
            facts["emitted"].append(emitted), facts["drained"].append(drained)
            t.upload(**st)
        d.steps(p, 1)
        t.step(p)
        got, want = snapshot(d, config), snapshot(t, config)
        assert not differing(got, want), (frame, differing(got, want), got["n"], want["n"])
        facts["n"].append(d.n)
        push = d.collider_push()
        act = acted(push)
        if frame == 0 and sources:                            # (every particle with the moved inlet's tag is in its first step)
            born = d.download()["id"] == sources[0][0]
            facts["born"] = int(born.sum())
            facts["born_pushed"] = int((push[born, 3] > 0).sum())
        if config in ("friction", "body"):
            assert d.collider_friction_reaction()["step"] == frame + 1
    if config == "body":
        facts["contacts"] = d.collider_body_contact_state()["contacts"]
    return got, facts


# the product run of item 1 per (config, variant): items 3 to 5 compare against its last frame without running T again
_LAST = {}


def last_frame(pkg, fp64, fast, config):
    key = (fp64, fast, config)
    if key not in _LAST:
        sc = S.cubes_with_obstacle(pkg, fp64)
        sources, drains = SS.composed_scene(sc)
        p = pkg.default_params(4, 1000.0)
        d = solids(pkg, sc, fp64, fast, config).set_sources(sources).set_drains(drains)
        for _ in range(SS.FRAMES):
            d.steps(p, 1)
        _LAST[key] = snapshot(d, config)
    return _LAST[key]


# ---- 1. the scene stage composes with the solids ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("config", CONFIGS)
def test_product_run_equals_the_host_sequenced_twin(pkg, config, fp64, fast):
    sc = S.cubes_with_obstacle(pkg, fp64)
    sources, drains = SS.composed_scene(sc)
    got, facts = run_twins(pkg, sc, fp64, fast, config, sources, drains, SS.FRAMES)
    _LAST.setdefault((fp64, fast, config), got)
    print(f"{config} {IDS[VARIANTS.index((fp64, fast))]}: {facts}")
    assert all(e == SS.emitted_per_frame(sources) for e in facts["emitted"])               # every frame emits
    assert sum(1 for k in facts["drained"] if k > 0) >= 2                                   # at least two frames drain
    assert facts["born_pushed"] >= 1, "no particle of the moved inlet's sheet was pushed in its first step"
    assert facts["drained_after_act"] >= 1, "no particle left through a drain after the collider had acted on it"
    if config in ("friction", "body"):
        nb = [SS.records(n) for n in facts["n"]]
        assert any(b > a for a, b in zip(nb, nb[1:])), ("the count of partial records never grew between a pass and the next body stage", facts["n"])
    if config == "body":
        assert facts["contacts"] > 0


# ---- 2. drains only: fewer partial records than the pass before wrote ------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("config", ["friction", "body"])
def test_drains_only_shrink_the_count_of_partial_records(pkg, config, fp64, fast):
    """2 060 particles, one step without a scene (its pass writes three records), then the drains: the corner drain takes the 60
    extra particles at the top of the next step, whose body stage is launched with two; the outlet takes fluid the collider
    had acted on"""
    base = S.cubes_with_obstacle(pkg, fp64)
    sc, drains = SS.shrinking_scene(base, dt_of(fp64))
    _, facts = run_twins(pkg, sc, fp64, fast, config, [], drains, 4, base=base, first_without_scene=True)
    nb = [SS.records(n) for n in facts["n"]]
    print(f"{config}: n per frame {facts['n']}, drained {facts['drained']}")
    assert nb[0] == 3 and any(b < a for a, b in zip(nb, nb[1:])), facts["n"]
    assert facts["drained"][0] >= 60 and facts["drained_after_act"] >= 1


# ---- 3. batched = stepped --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("config", CONFIGS)
def test_batched_equals_stepped(pkg, config, fp64, fast):
    sc = S.cubes_with_obstacle(pkg, fp64)
    sources, drains = SS.composed_scene(sc)
    want = last_frame(pkg, fp64, fast, config)
    d = solids(pkg, sc, fp64, fast, config).set_sources(sources).set_drains(drains).steps(pkg.default_params(4, 1000.0), SS.FRAMES)
    got = snapshot(d, config)
    assert not differing(got, want), differing(got, want)
    assert 1 <= d.scene_host_syncs() <= SS.FRAMES


# ---- 4. graph mode -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
@pytest.mark.parametrize("config", ["friction", "body"])
def test_graph_mode_captures_only_after_the_scene_is_cleared(pkg, config, fp64, fast):
    sc = S.cubes_with_obstacle(pkg, fp64)
    sources, drains = SS.composed_scene(sc)
    p = pkg.default_params(4, 1000.0)
    runs = {}
    for graph in (1, 0):
        s = solids(pkg, sc, fp64, fast, config, path=dict(graph=graph)).set_sources(sources).set_drains(drains)
        for _ in range(SS.FRAMES):
            s.steps(p, 1)
        assert s.graph_stats()[:2] == (0, 0)                 # a scene forces eager steps
        got = snapshot(s, config)
        assert not differing(got, last_frame(pkg, fp64, fast, config)), (graph, differing(got, last_frame(pkg, fp64, fast, config)))
        s.set_sources([]).set_drains([])
        s.steps(p, 3).steps(p, 3)
        runs[graph] = (snapshot(s, config), s.graph_stats())
    print(f"{config}: graph stats after the scene was cleared {runs[1][1]}, eager {runs[0][1]}")
    assert runs[1][1][0] > 0 and runs[1][1][1] > 0 and runs[1][1][2], runs[1][1]
    assert runs[0][1][:2] == (0, 0)
    assert not differing(runs[1][0], runs[0][0]), differing(runs[1][0], runs[0][0])
    assert runs[1][0]["vel"] != last_frame(pkg, fp64, fast, config)["vel"]


# ---- 5. launch paths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_every_launch_path_gives_the_default_paths_bytes(pkg, fp64, fast):
    sc = S.cubes_with_obstacle(pkg, fp64)
    sources, drains = SS.composed_scene(sc)
    p = pkg.default_params(4, 1000.0)
    want = last_frame(pkg, fp64, fast, "body")
    for path in (dict(row_major=0), dict(gather=0), dict(gather=3), dict(list_max=12)):
        d = solids(pkg, sc, fp64, fast, "body", path=path).set_sources(sources).set_drains(drains)
        for _ in range(SS.FRAMES):
            d.steps(p, 1)
        got = snapshot(d, "body")
        assert not differing(got, want), (path, differing(got, want))


# ---- 6. depletion ----------------------------------------------------------------------------------------------------------------
def host_body_step(ref, contact, last, s, p):
    """the numpy loop of collider_body_ref, collider_friction_ref and body_contact_ref for the step `s` has just run, fed the
    device's own raw sums: the kick with the friction sums `last` (None: nothing pending), the advance, one contact pass"""
    st, cs = s.collider_body_state(raw=True), s.collider_body_contact_state(raw=True)
    if last is not None:
        FR.kick(ref, last["impulse"], last["angular"])
    ref.advance(float(p.dt), list(st.impulse), list(st.angular), int(st.hits))
    contact.resolve(ref, cs.depth_sum, list(cs.push), list(cs.arm), cs.depth_max, 1 if cs.depth_max > 0 else 0)


@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_depletion_keeps_the_pending_kick_for_the_step_that_refills(pkg, fp64, fast):
    """Configuration (d) on a block without obstacle particles.  Two steps; a drain that takes all fluid and two steps with
    n == 0 (pbf_step returns before the body stage: the body's bytes, the contact's and the friction pass's count stay); the
    drain cleared, one inlet set, and a step that refills.  D equals T, which uploaded an empty set and then the emitted
    sheet.  The body of every step that ran equals the numpy loop in which the friction sums of step 2 kick exactly once, in
    the refilling step: a loop that skips that kick, and one that repeats it a step later, both differ."""
    dtype = dt_of(fp64)
    sc = SS.depletion_scene(dtype)
    assert not (sc["type"] == 1).any()
    p = pkg.default_params(4, 1000.0)
    source = [SS.composed_scene(sc)[0][0]]
    empty = {k: v[:0] for k, v in sc.items()}
    d, t = solids(pkg, sc, fp64, fast, "body"), solids(pkg, sc, fp64, fast, "body")
    ref = stock_body()
    contact = BC.Contact(CONTACT["skin"], CONTACT["restitution"], CONTACT["friction"], CONTACT["correction"], CONTACT["slop"],
                         points=len(d.collider_body_contact_points()))
    last = None
    for k in range(2):
        d.steps(p, 1), t.step(p)
        assert not differing(snapshot(d, "body"), snapshot(t, "body")), k
        host_body_step(ref, contact, last, d, p)
        assert body_bytes(d) == ref.state_words() and contact_bytes(d) == contact.state_words(), k
        last = d.collider_friction_reaction()
    assert last["hits"] > 0 and np.abs(last["impulse"]).max() > 0 and last["step"] == 2
    before = records_of(d, "body")
    d.set_drains([((500.0, 500.0, 500.0), 2000.0)])
    for k in range(2):
        d.steps(p, 1)
        assert d.n == 0 and records_of(d, "body") == before, k
        assert d.collider_friction_reaction()["step"] == 2
    t.upload(**empty).step(p)
    assert t.n == 0 and records_of(t, "body") == before
    d.set_drains([]).set_sources(source)
    d.steps(p, 1)
    t.upload(**S.np_emit(empty, source, dtype)).step(p)
    got, want = snapshot(d, "body"), snapshot(t, "body")
    assert d.n == SS.emitted_per_frame(source) and not differing(got, want), differing(got, want)
    unkicked, c2 = copy.deepcopy(ref), copy.deepcopy(contact)
    host_body_step(unkicked, c2, None, d, p)
    host_body_step(ref, contact, last, d, p)
    st = d.collider_body_state()
    assert body_bytes(d) == ref.state_words(), (st["velocity"], ref.v, st["angular_velocity"], ref.w)
    assert contact_bytes(d) == contact.state_words()
    assert unkicked.state_words() != ref.state_words()        # (the kick was not a kick with zeros)
    stale, now = last, d.collider_friction_reaction()
    assert now["step"] == 3
    d.steps(p, 1)                                             # the step after takes the refilling step's sums, not step 2's again
    twice, c3 = copy.deepcopy(ref), copy.deepcopy(contact)
    host_body_step(ref, contact, now, d, p)
    FR.kick(twice, stale["impulse"], stale["angular"])
    host_body_step(twice, c3, now, d, p)
    assert body_bytes(d) == ref.state_words() and twice.state_words() != ref.state_words()


# ---- 7. capacity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64,fast", VARIANTS, ids=IDS)
def test_a_step_beyond_the_capacity_fails_before_anything_is_launched(pkg, fp64, fast):
    """sources only: the count is 2 000 + 28 k after frame k; a reserve of 2 066 holds two frames and refuses the third"""
    sc = S.cubes_with_obstacle(pkg, fp64)
    sources, _ = SS.composed_scene(sc)
    per = SS.emitted_per_frame(sources)
    reserve = len(sc["id"]) + 2 * per + 10
    p = pkg.default_params(4, 1000.0)
    d = solids(pkg, sc, fp64, fast, "body", reserve=reserve).set_sources(sources)
    d.steps(p, 1).steps(p, 1)
    assert d.n == len(sc["id"]) + 2 * per
    before = snapshot(d, "body")
    assert d.L.pbf_step(d.ctx, C.byref(p)) == ERR_INVALID and b"capacity" in d.L.pbf_last_error(d.ctx)
    assert d.L.pbf_steps(d.ctx, C.byref(p), 3) == ERR_INVALID
    after = snapshot(d, "body")
    assert not differing(after, before), differing(after, before)
    # and the ctx goes on once the inlets are closed: the step of a twin that never tried
    twin = solids(pkg, sc, fp64, fast, "body", reserve=reserve).set_sources(sources)
    twin.steps(p, 1).steps(p, 1).set_sources([]).steps(p, 1)
    d.set_sources([]).steps(p, 1)
    assert not differing(snapshot(d, "body"), snapshot(twin, "body"))
