"""What the collider entry points refuse, and what they take as a no-op (include/pbf_hip.h; the modes and their rules:
pbf-sph_amd/csrc/pbf_collider_state.hpp): the return code and the text of pbf_last_error, byte for byte, for every refusal
that depends on which of lattice / pose / reaction / body / friction is on; and the calls that change nothing — clearing what
is clear, enabling what is enabled — return PBF_OK, leave the state's bytes alone and capture no graph.

The expected texts are literals, written down from the source before the modes were given one owner: a characterisation of
what a caller sees, not of how the library keeps its flags.  One tiny scene (a 4 096-particle dam break, an 8 x 8 x 8 lattice
of a box on the floor, fp32).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_STATE = 0, -1, -4

NO_COLLIDER = "%s: no collider set (pbf_set_collider)"
POSE_OWNED = "pbf_set_collider_pose: a body is on and owns the pose (re-place it through pbf_set_collider_body)"
KEEP_FOR_BODY = "pbf_set_collider_reaction: a body is on and needs the records (pbf_set_collider_body(ctx, NULL) first)"
KEEP_FOR_FRICTION = "pbf_set_collider_reaction: friction is on and needs the records (pbf_set_collider_friction(ctx, NULL) first)"
REACTION_OFF = "pbf_collider_reaction: not enabled (pbf_set_collider_reaction)"
REACTION_NO_STEP = "pbf_collider_reaction: no step since the reaction was enabled or the arrays last changed"
FRICTION_OFF = "pbf_collider_friction_reaction: friction is off (pbf_set_collider_friction)"
FRICTION_NO_STEP = "pbf_collider_friction_reaction: no step since friction was turned on"
STAGE_NO_BODY = "pbf_stage_body: no body set (pbf_set_collider_body)"
STATE_NO_BODY = "pbf_collider_body_state: no body set (pbf_set_collider_body)"
BODY_NO_SORT = "the collider body needs a sort since the reaction records were enabled"
FRICTION_NO_SORT = "the collider friction needs a sort since the reaction records were enabled"


class Scene:
    def __init__(self, pkg):
        from pbf_sph_amd import capi
        self.pkg, self.capi = pkg, capi
        self.sc, self.side = pkg.scene_dambreak(4096, False)
        self.p = pkg.default_params(4, self.side)
        s = self.side
        self.spacing = s / 7.0
        self.phi = capi.sdf_lattice(capi.sdf_box((0.3 * s, 0.0, 0.3 * s), (0.7 * s, 0.3 * s, 0.7 * s)), (0.0, 0.0, 0.0), self.spacing, (8, 8, 8))
        self.pose = capi.ColliderPose()
        self.pose.rot[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
        self.pose.trans[:] = [0.01 * s, 0.0, 0.0]
        self.body = capi.collider_body(mass=1.0e6)
        self.friction = capi.ColliderFriction()
        self.friction.mu = 0.5
        self.wrench, self.state = capi.ColliderWrench(), capi.ColliderBodyState()

    def solver(self, lattice=True, graph=False):
        s = self.pkg.Solver(h=0.1, fp64=False)
        if graph:
            s.set_option("graph", 1)
        s.upload(**self.sc)
        return self.install(s) if lattice else s

    def install(self, s):
        return s.set_collider(self.phi, (0.0, 0.0, 0.0), self.spacing, 0.1 * self.spacing)


@pytest.fixture(scope="module")
def scene(pkg):
    return Scene(pkg)


def refused(s, rc, code, text):
    got = s.L.pbf_last_error(s.ctx)
    assert rc == code and got == text.encode(), (rc, got)


def everything(s):
    out = {k: v.tobytes() for k, v in s.download().items()}
    out["pstar"] = s.pstar().tobytes()
    return out


def test_without_a_collider(scene):
    """pose, body, friction and sample, set or cleared, and the reaction's observer with the reaction on"""
    s = scene.solver(lattice=False)
    L, p = s.L, scene.p
    pts = np.zeros((1, 3))
    for _ in range(2):                                          # (before any step and after one)
        refused(s, L.pbf_set_collider_pose(s.ctx, C.byref(scene.pose)), ERR_STATE, NO_COLLIDER % "pbf_set_collider_pose")
        refused(s, L.pbf_set_collider_pose(s.ctx, None), ERR_STATE, NO_COLLIDER % "pbf_set_collider_pose")
        refused(s, L.pbf_set_collider_body(s.ctx, C.byref(scene.body)), ERR_STATE, NO_COLLIDER % "pbf_set_collider_body")
        refused(s, L.pbf_set_collider_body(s.ctx, None), ERR_STATE, NO_COLLIDER % "pbf_set_collider_body")
        refused(s, L.pbf_set_collider_friction(s.ctx, C.byref(scene.friction)), ERR_STATE, NO_COLLIDER % "pbf_set_collider_friction")
        refused(s, L.pbf_set_collider_friction(s.ctx, None), ERR_STATE, NO_COLLIDER % "pbf_set_collider_friction")
        refused(s, L.pbf_collider_sample(s.ctx, C.byref(p), 1, pts.ctypes.data, None, None, None), ERR_STATE, NO_COLLIDER % "pbf_collider_sample")
        refused(s, L.pbf_collider_reaction(s.ctx, C.byref(scene.wrench)), ERR_STATE, REACTION_OFF)
        refused(s, L.pbf_collider_friction_reaction(s.ctx, C.byref(scene.wrench)), ERR_STATE, FRICTION_OFF)
        refused(s, L.pbf_collider_body_state(s.ctx, C.byref(scene.state)), ERR_STATE, STATE_NO_BODY)
        refused(s, L.pbf_stage_body(s.ctx, C.byref(p)), ERR_STATE, STAGE_NO_BODY)
        s.step(p)
    # the reaction may be on without a lattice; its observer then names the lattice, step or no step
    assert L.pbf_set_collider_reaction(s.ctx, 1) == OK
    refused(s, L.pbf_collider_reaction(s.ctx, C.byref(scene.wrench)), ERR_STATE, NO_COLLIDER % "pbf_collider_reaction")
    s.step(p)
    refused(s, L.pbf_collider_reaction(s.ctx, C.byref(scene.wrench)), ERR_STATE, NO_COLLIDER % "pbf_collider_reaction")
    refused(s, L.pbf_collider_reaction(s.ctx, None), ERR_INVALID, "pbf_collider_reaction: out == NULL")
    s.close()


def test_the_observers_before_any_step(scene):
    s = scene.solver()
    L, p = s.L, scene.p
    refused(s, L.pbf_collider_reaction(s.ctx, C.byref(scene.wrench)), ERR_STATE, REACTION_OFF)
    refused(s, L.pbf_collider_friction_reaction(s.ctx, C.byref(scene.wrench)), ERR_STATE, FRICTION_OFF)
    refused(s, L.pbf_collider_body_state(s.ctx, C.byref(scene.state)), ERR_STATE, STATE_NO_BODY)
    refused(s, L.pbf_stage_body(s.ctx, C.byref(p)), ERR_STATE, STAGE_NO_BODY)
    s.set_collider_reaction(True)
    refused(s, L.pbf_collider_reaction(s.ctx, C.byref(scene.wrench)), ERR_STATE, REACTION_NO_STEP)
    s.set_collider_friction(0.5)
    refused(s, L.pbf_collider_friction_reaction(s.ctx, C.byref(scene.wrench)), ERR_STATE, FRICTION_NO_STEP)
    refused(s, L.pbf_collider_reaction(s.ctx, C.byref(scene.wrench)), ERR_STATE, REACTION_NO_STEP)
    refused(s, L.pbf_collider_friction_reaction(s.ctx, None), ERR_INVALID, "pbf_collider_friction_reaction: out == NULL")
    refused(s, L.pbf_collider_body_state(s.ctx, None), ERR_INVALID, "pbf_collider_body_state: out == NULL")
    s.steps(p, 2)
    assert s.collider_reaction()["step"] == 2 and s.collider_friction_reaction()["step"] == 2
    # turned off and on again: the pass count starts over, and so does the wait for a step; the reaction's records stay
    s.set_collider_friction(None).set_collider_friction(0.5)
    refused(s, L.pbf_collider_friction_reaction(s.ctx, C.byref(scene.wrench)), ERR_STATE, FRICTION_NO_STEP)
    assert s.collider_reaction()["step"] == 2
    # a replaced lattice turns friction off; the reaction stays on and its records are the last step's
    scene.install(s)
    refused(s, L.pbf_collider_friction_reaction(s.ctx, C.byref(scene.wrench)), ERR_STATE, FRICTION_OFF)
    assert s.collider_reaction()["step"] == 2
    # the reaction off and on again: no records until the next sort
    s.set_collider_reaction(False).set_collider_reaction(True)
    refused(s, L.pbf_collider_reaction(s.ctx, C.byref(scene.wrench)), ERR_STATE, REACTION_NO_STEP)
    s.step(p)
    assert s.collider_reaction()["step"] == 1
    s.close()


def test_what_a_body_or_friction_forbids(scene):
    s = scene.solver()
    L, p = s.L, scene.p
    s.step(p)
    # a stage that needs the records, asked for between enabling them and the next sort (nothing is launched)
    s.set_collider_body(mass=1.0e6)
    refused(s, L.pbf_stage_body(s.ctx, C.byref(p)), ERR_STATE, BODY_NO_SORT)
    s.steps(p, 2)
    refused(s, L.pbf_set_collider_pose(s.ctx, C.byref(scene.pose)), ERR_STATE, POSE_OWNED)
    refused(s, L.pbf_set_collider_pose(s.ctx, None), ERR_STATE, POSE_OWNED)
    refused(s, L.pbf_set_collider_reaction(s.ctx, 0), ERR_STATE, KEEP_FOR_BODY)
    refused(s, L.pbf_collider_friction_reaction(s.ctx, C.byref(scene.wrench)), ERR_STATE, FRICTION_OFF)
    s.set_collider_friction(0.5)
    refused(s, L.pbf_set_collider_reaction(s.ctx, 0), ERR_STATE, KEEP_FOR_BODY)      # (both on: the body is named)
    s.steps(p, 2)
    assert s.collider_body_state()["steps"] == 4 and s.collider_friction_reaction()["step"] == 2
    s.set_collider_body(None)
    refused(s, L.pbf_set_collider_reaction(s.ctx, 0), ERR_STATE, KEEP_FOR_FRICTION)
    refused(s, L.pbf_collider_body_state(s.ctx, C.byref(scene.state)), ERR_STATE, STATE_NO_BODY)
    refused(s, L.pbf_stage_body(s.ctx, C.byref(p)), ERR_STATE, STAGE_NO_BODY)
    # the body left its pose behind as an ordinary one: it may be set and cleared again
    assert L.pbf_set_collider_pose(s.ctx, C.byref(scene.pose)) == OK and L.pbf_set_collider_pose(s.ctx, None) == OK
    s.set_collider_friction(None)
    assert L.pbf_set_collider_reaction(s.ctx, 0) == OK
    # friction alone, turned on after a step: the records it reads come with the next sort
    s.set_collider_friction(0.5)
    refused(s, L.pbf_stage_finalise(s.ctx, C.byref(p)), ERR_STATE, FRICTION_NO_SORT)
    refused(s, L.pbf_set_collider_reaction(s.ctx, 0), ERR_STATE, KEEP_FOR_FRICTION)
    s.step(p)
    assert s.collider_friction_reaction()["step"] == 1
    s.close()


def test_no_ops_change_nothing_and_capture_nothing(scene):
    """two contexts take the same steps; one of them is also asked to clear what is clear and enable what is enabled"""
    p = scene.p
    s, twin = scene.solver(graph=True), scene.solver(graph=True)
    L = s.L

    def same():
        assert s.graph_stats() == twin.graph_stats(), (s.graph_stats(), twin.graph_stats())
        a, b = everything(s), everything(twin)
        assert a == b, [k for k in a if a[k] != b[k]]

    for t in (s, twin):
        t.steps(p, 4)
    assert s.graph_stats()[0] > 0 and s.graph_stats()[2]
    assert L.pbf_set_collider_pose(s.ctx, None) == OK           # a static lattice: everything is off
    assert L.pbf_set_collider_reaction(s.ctx, 0) == OK
    assert L.pbf_set_collider_body(s.ctx, None) == OK
    assert L.pbf_set_collider_friction(s.ctx, None) == OK
    for t in (s, twin):
        t.steps(p, 2)
    same()
    assert s.graph_stats()[1] > 0

    for t in (s, twin):                                         # body and friction on (with them the reaction and a pose)
        t.set_collider_body(mass=1.0e6).set_collider_friction(0.5).steps(p, 4)
    captured = s.graph_stats()[0]
    assert L.pbf_set_collider_reaction(s.ctx, 1) == OK
    for t in (s, twin):
        t.steps(p, 2)
    same()
    assert s.graph_stats()[0] == captured
    assert s.collider_body_state(raw=True).steps == twin.collider_body_state(raw=True).steps == 6
    assert bytes(s.collider_friction_reaction(raw=True)) == bytes(twin.collider_friction_reaction(raw=True))

    for t in (s, twin):                                         # the reaction alone, the body's last pose kept
        t.set_collider_friction(None).set_collider_body(None).steps(p, 4)
    captured = s.graph_stats()[0]
    assert L.pbf_set_collider_reaction(s.ctx, 1) == OK
    assert L.pbf_set_collider_body(s.ctx, None) == OK
    assert L.pbf_set_collider_friction(s.ctx, None) == OK
    for t in (s, twin):
        t.steps(p, 2)
    same()
    assert s.graph_stats()[0] == captured
    assert bytes(s.collider_reaction(raw=True)) == bytes(twin.collider_reaction(raw=True))
    s.close()
    twin.close()
