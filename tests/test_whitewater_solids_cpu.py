"""Whitewater against the solids without a device: the restatement (tests/whitewater_solids_ref.py) reaches every branch of the
contract on the shared cases, the response has the properties the contract promises within bars counted from its roundings,
each mutation is told from the contract, and the ctypes structures and symbols agree with the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import collider_pose_ref as PR
import collider_ref as CR
import scenery_ref as SR
import whitewater_solids_ref as WS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float64, np.float32]
IDS = ["fp64", "fp32"]
V_BODY, W_BODY = (40.0, -25.0, 10.0), (0.3, -0.2, 0.5)       # world units and radians per time


def wedge(dtype, n=600, **kw):
    plane, ball, pose, fr = SR.wedge_case(dtype)
    x, v, nF, alive = WS.wedge_pool(dtype, n)
    return WS.collide(dtype, fr, x, v, alive, nF, collider=ball, scenery=plane, **kw), (x, v, nF, alive, fr, plane, ball)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_cases_reach_every_branch(dtype):
    r, (x, v, nF, alive, fr, plane, ball) = wedge(dtype, e=0.5, f=0.25, absorb=True)
    h1, h2 = r["hit1"], r["hit2"]
    groups = {"collider only": h1 & ~h2, "scenery only": h2 & ~h1, "both": h1 & h2, "no hit": alive & ~h1 & ~h2,
              "receding": (r["first"]["act"] & ~r["first"]["go"]) | (r["second"]["act"] & ~r["second"]["go"]),
              "nF == 0 with a hit": r["absorbed"], "dead on entry": ~alive}
    lat, cfr, cx = WS.cover_case(dtype)
    n = len(cx)
    c = WS.collide(dtype, cfr, cx, np.full((n, 3), -1.0, dtype), np.ones(n, bool), np.ones(n, np.int64), scenery=lat, e=0.5, f=0.25)
    groups["hit && len == 0"] = c["hit2"] & ~c["second"]["act"]
    print({k: int(g.sum()) for k, g in groups.items()})
    for name, g in groups.items():
        assert g.sum() >= 5, name
    # without a hit every bit is kept; with one the particle ends outside both solids' margins or on a face of the box
    quiet = ~(h1 | h2)
    assert r["pos"][quiet].tobytes() == x[quiet].tobytes() and r["vel"][quiet].tobytes() == v[quiet].tobytes()
    keep = ~r["first"]["go"] & ~r["second"]["go"]
    assert r["vel"][keep].tobytes() == v[keep].tobytes() and (keep & (h1 | h2)).sum() >= 5
    z = groups["hit && len == 0"]
    assert c["pos"][z].tobytes() == cx[z].tobytes() and (c["vel"][z] == -1).all() and (c["pos"][~z & c["hit2"]][:, 1] == 0).all()
    # the scenery has the last word: nobody is left under the plane by more than the plane's own bar
    moved = (h1 | h2) & ~CR.on_face(fr, r["pos"] / fr[0])
    phi = CR.plane_phi(CR.PLANE_N, SR.WEDGE_PLANE_D, r["pos"][moved].astype(np.float64))
    assert moved.sum() >= 50 and phi.min() >= CR.MARGIN - CR.plane_bar_world(dtype)
    # the counts, and absorb = 0 kills nobody
    assert WS.counts(r) == dict(hit_collider=int(h1.sum()), hit_scenery=int(h2.sum()), absorbed=int(r["absorbed"].sum()))
    assert not (h1 & ~alive).any() and not (r["alive"] & r["absorbed"]).any()
    r0, _ = wedge(dtype, e=0.5, f=0.25, absorb=False)
    assert np.array_equal(r0["alive"], alive) and r0["pos"].tobytes() == r["pos"].tobytes()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_response_has_the_contracts_properties(dtype):
    """on the ball alone, moving (V, W): the relative normal velocity after a response is -e un; f = 1, e = 0 leaves no relative
    velocity; e = f = 0 against a solid at rest keeps the tangential part.  The bars: whitewater_solids_ref's docstring."""
    plane, ball, pose, fr = SR.wedge_case(dtype)
    x, v, nF, alive = WS.wedge_pool(dtype, 900)
    F = np.float64

    def run(e, f, V=None, W=None):
        r = WS.collide(dtype, fr, x, v, alive, nF, collider=ball, V=V, W=W, e=e, f=f)
        go = r["first"]["go"]
        assert go.sum() >= 30
        n, un, ut = (r["first"][k][go].astype(F) for k in ("n", "un", "ut"))
        rel = r["vel"][go].astype(F) - r["vb"][go].astype(F)
        S = np.sqrt((v[go].astype(F) ** 2).sum(1)) + np.sqrt((r["vb"][go].astype(F) ** 2).sum(1))
        return rel, n, un, ut, S

    for e, f in ((0.0, 0.0), (0.5, 0.25), (1.0, 1.0), (0.3, 1.0)):
        rel, n, un, ut, S = run(e, f, V_BODY, W_BODY)
        err = np.abs((rel * n).sum(1) + e * un) / S
        print(dtype.__name__, "e", e, "f", f, "normal: worst", err.max() / (np.finfo(dtype).eps / 2), "units of", WS.NORMAL_UNITS)
        assert (err <= WS.bar_speed(dtype, WS.NORMAL_UNITS, 1.0)).all()
        want = (1.0 - f) * ut - (e * un)[:, None] * n
        assert (np.abs(rel - want).max(1) / S <= WS.bar_speed(dtype, WS.TANGENT_UNITS, 1.0)).all()
    rel, n, un, ut, S = run(0.0, 1.0, V_BODY, W_BODY)
    assert (np.abs(rel).max(1) / S <= WS.bar_speed(dtype, WS.TANGENT_UNITS, 1.0)).all()          # sticks: no relative velocity
    rel, n, un, ut, S = run(0.0, 0.0)
    tang = rel - (rel * n).sum(1)[:, None] * n
    assert (np.abs(tang - ut).max(1) / S <= WS.bar_speed(dtype, WS.TANGENT_UNITS + WS.NORMAL_UNITS, 1.0)).all()   # slides on


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mutation", WS.MUTATIONS)
def test_mutations_are_caught(dtype, mutation):
    """each mutation changes the bytes of at least 5 particles of the wedge under a moving ball"""
    good, _ = wedge(dtype, e=0.5, f=0.25, V=V_BODY, W=W_BODY)
    bad, _ = wedge(dtype, e=0.5, f=0.25, V=V_BODY, W=W_BODY, mutation=mutation)
    differ = (good["pos"] != bad["pos"]).any(1) | (good["vel"] != bad["vel"]).any(1)
    print(mutation, int(differ.sum()))
    assert differ.sum() >= 5


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_posed_and_edge_lattices(dtype):
    """the posed contract is the one collider_pose_ref states (a plane in a body frame under the generic pose), and on the edge
    lattices a point outside, NaN included, keeps its bits and is not counted"""
    pose64 = PR.GENERIC
    lat, _, _, fr = PR.body_plane_case(pose64, dtype)
    pose = PR.pose_of(*pose64, dtype)
    x, v, nF, alive = WS.wedge_pool(dtype, 300)
    r = WS.collide(dtype, fr, x, v, alive, nF, collider=lat, pose=pose, V=V_BODY, W=W_BODY, t=pose[1], e=0.2, f=0.1)
    _, q1, hit = PR.project(lat, fr, pose, x / fr[0])
    assert (hit & alive).sum() >= 20 and np.array_equal(r["hit1"], hit & alive)
    assert r["q1"].tobytes() == q1.tobytes()
    same_t = WS.collide(dtype, fr, x, v, alive, nF, collider=lat, pose=pose, V=V_BODY, W=W_BODY, t=None, e=0.2, f=0.1)
    assert (same_t["vel"] != r["vel"]).any()          # (the arm is taken about the pose's t)
    for dims in CR.EDGE_LATTICES:
        elat, efr, pts, names = CR.edge_case(dims, dtype, n_random=200)
        ex = pts.astype(dtype)
        ev = np.ones_like(ex)
        er = WS.collide(dtype, efr, ex, ev, np.ones(len(ex), bool), np.zeros(len(ex), np.int64), collider=elat, e=1.0, f=1.0, absorb=True)
        phi, _, hit = CR.project(elat, efr, ex / efr[0])
        assert np.array_equal(er["hit1"], hit) and np.array_equal(er["absorbed"], hit)
        out = ~hit
        assert er["pos"][out].tobytes() == ex[out].tobytes() and (er["vel"][out] == 1).all()
        for name in ("nan", "+inf", "-inf", "mixed"):
            assert not hit[names.index(name)]


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pbf_hip.h")).read(), flags=re.S)


def test_abi(pkg):
    """the two symbols are exported and the ctypes structures are the header's: 2 doubles + 2 words = 24 bytes, 5 words = 40"""
    from pbf_sph_amd import capi
    assert C.sizeof(capi.WhitewaterSolids) == 2 * 8 + 2 * 4 == 24 and C.sizeof(capi.WhitewaterSolidsStats) == 5 * 8 == 40
    code = header()
    body = re.search(r"typedef struct pbf_whitewater_solids \{(.*?)\} pbf_whitewater_solids;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", body) == [n for n, _ in capi.WhitewaterSolids._fields_]
    body = re.search(r"struct pbf_whitewater_solids_stats \{(.*?)\};", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", body) == [n for n, _ in capi.WhitewaterSolidsStats._fields_]
    for f in ("pbf_set_whitewater_solids", "pbf_whitewater_solids_stats"):
        assert f in capi.exported_symbols() and hasattr(C.CDLL(pkg.LIB_PATH), f)
    assert callable(pkg.Solver.set_whitewater_solids) and callable(pkg.Solver.whitewater_solids_stats)
    assert pkg.lib().pbf_set_whitewater_solids(None, None) == -1 and pkg.lib().pbf_whitewater_solids_stats(None, None) == -1


def test_settings_check_restated():
    assert WS.settings_ok(0, 0) and WS.settings_ok(1, 1) and WS.settings_ok(0.5, 0.25)
    for bad in (dict(restitution=-0.1), dict(restitution=1.5), dict(restitution=float("nan")), dict(friction=-1e-9),
                dict(friction=2.0), dict(friction=float("nan")), dict(reserved=1)):
        assert not WS.settings_ok(**bad), bad
