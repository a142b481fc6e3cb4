"""Whitewater against the solids on the device (pbf_set_whitewater_solids): the pass byte for byte against its NumPy
restatement (tests/whitewater_solids_ref.py) under every instantiation the host can choose, the children, a spray particle
that comes to rest on a plane, off is off, every gather path, the counts and the refusals, the shim and the CLI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import collider_pose_ref as PR
import collider_ref as CR
import scenery_ref as SR
import test_whitewater_gpu as TW
import whitewater_ref as WR
import whitewater_solids_ref as WS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = TW.H
ERR_INVALID, ERR_STATE = -1, -4
V_BODY, W_BODY = (40.0, -25.0, 10.0), (0.3, -0.2, 0.5)
CFG0 = dict(k_ta=0.0, k_wc=0.0, tau_ta=(0, 1), tau_wc=(0, 1), tau_k=(0, 1), k_b=2.0, k_d=0.8, spray_below=6, bubble_from=20)


def install(s, which, lat, spacing):
    """a collider_ref.Lattice as the collider or the scenery (its nodes are values of N already)"""
    getattr(s, "set_" + which)(lat.phi.astype(np.float64), origin=lat.origin.astype(np.float64), spacing=spacing, margin=float(lat.margin))


def clear(s):
    s.set_collider(None)
    s.set_scenery(None)


def plane_points(rng, n, normal, d, spread=60.0):
    """n points of the stock box within `spread` world units of the plane n.w = d"""
    nn = np.asarray(normal, np.float64)
    nn = nn / np.sqrt((nn * nn).sum())
    w = rng.random((n, 3)) * 800.0 + 100.0
    return w + ((rng.random(n) - 0.5) * 2 * spread - (w @ nn - d))[:, None] * nn


def ball_points(rng, n):
    return SR.wedge_centre() + (rng.random((n, 3)) - 0.5) * 2.4 * SR.WEDGE_BALL_R


# name -> (where a third of the pool goes, what to install): the instantiations of k_ww_solids
def setups(s, dtype):
    plane, ball, _, _ = SR.wedge_case(dtype)
    body_lat, _, _, _ = PR.body_plane_case(PR.GENERIC, dtype)
    pose = PR.pose_of(*PR.GENERIC, dtype)
    rng = np.random.default_rng(31)
    world = lambda n: plane_points(rng, n, PR.WORLD_N, PR.WORLD_D)
    wedge = lambda n: np.concatenate([ball_points(rng, n - n // 3), plane_points(rng, n // 3, CR.PLANE_N, SR.WEDGE_PLANE_D)])

    def static():
        install(s, "collider", ball, SR.WEDGE_SPACING)
        return dict(collider=ball)

    def posed():
        install(s, "collider", body_lat, PR.BODY_SPACING)
        s.set_collider_pose(*PR.GENERIC)
        return dict(collider=body_lat, pose=pose)

    def body():
        install(s, "collider", body_lat, PR.BODY_SPACING)
        s.set_collider_body(mass=50.0, rot=PR.GENERIC[0], centre=PR.GENERIC[1], velocity=V_BODY, angular_velocity=W_BODY)
        st = s.collider_body_state()
        at = PR.pose_of(st["rot"], st["centre"], dtype)
        return dict(collider=body_lat, pose=at, V=st["velocity"], W=st["angular_velocity"], t=at[1])

    def friction_posed():
        got = posed()
        s.set_collider_friction(0.5, velocity=V_BODY, angular_velocity=W_BODY)
        return dict(got, V=V_BODY, W=W_BODY, t=pose[1])

    def friction_static():
        got = static()
        s.set_collider_friction(0.5, velocity=V_BODY, angular_velocity=W_BODY)
        return dict(got, V=V_BODY, W=W_BODY)

    def scenery():
        install(s, "scenery", plane, SR.WEDGE_SPACING)
        return dict(scenery=plane)

    def both():
        return dict(static(), **scenery())

    def both_body():          # (the wedge's plane lies wholly inside the body plane's solid: the ball is the scenery here)
        got = body()
        install(s, "scenery", ball, SR.WEDGE_SPACING)
        return dict(got, scenery=ball)

    def both_friction():
        return dict(friction_static(), **scenery())

    balls = lambda n: ball_points(rng, n)
    return {"static": (balls, static), "posed": (world, posed), "body": (world, body), "friction+pose": (world, friction_posed),
            "friction": (balls, friction_static), "scenery": (wedge, scenery),
            "both": (wedge, both), "body+scenery": (lambda n: np.concatenate([world(n // 2), balls(n - n // 2)]), both_body),
            "friction+scenery": (wedge, both_friction)}


def pool_for(s, p, n, dtype, where):
    """test_whitewater_gpu.advect_pool with a third of it (85 of 257, from the particles placed in the fluid) moved in and around
    the solids; smaller pools keep the same mix"""
    pool = TW.advect_pool(s, p, 257, dtype)
    k = 85
    pool["pos"][15:15 + k] = np.clip(where(k), 0.0, float(p.max_bound[0])).astype(dtype)
    pool["pos"][15] = (SR.wedge_centre() + 5.0).astype(dtype)          # (inside the wedge's ball: a pool of one still hits)
    if n < 257:
        pick = np.concatenate([np.arange(15, 15 + k)[::3], np.arange(0, 15), np.arange(100, 257)])[:n]
        pool = {key: v[pick].copy() for key, v in pool.items()}
    return pool


def expected(s, p, pool, cfg, dtype, solids, **setting):
    pts = np.where(np.isfinite(pool["pos"]), pool["pos"], 1e9).astype(np.float64)
    smp = s.sample(p, pts, velocity=True)
    return WS.step(pool, smp, cfg, p, dtype, **solids, **setting)


def check_bytes(got, want, what=""):
    a = want["alive"]
    for k in ("pos", "vel", "life", "kind"):
        assert got[k].tobytes() == np.ascontiguousarray(want[k][a]).tobytes(), (what, k)


# ---- 1. bit for bit ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("absorb", [0, 1])
@pytest.mark.parametrize("fp64", [True, False], ids=TW.IDS)
def test_bit_for_bit_under_every_instantiation(pkg, fp64, absorb):
    """one resident state, one pool; the solids change between whitewater steps (rates 0: no children)"""
    s, p = TW.stepped(pkg, "dam8192", fp64)
    dtype = np.float64 if fp64 else np.float32
    cfg = dict(CFG0, capacity=257)
    s.whitewater_configure(**cfg)
    s.set_whitewater_solids(restitution=0.5, friction=0.25, absorb=bool(absorb))
    steps = 0
    for name, (where, make) in setups(s, dtype).items():
        clear(s)
        solids = make()
        pool = pool_for(s, p, 257, dtype, where)
        s.whitewater_upload(**pool)
        want = expected(s, p, pool, cfg, dtype, solids, e=0.5, f=0.25, absorb=bool(absorb))
        st = s.whitewater_step(p)
        steps += 1
        got, cnt = s.whitewater_download(), s.whitewater_solids_stats()
        c = WS.counts(want)
        print(name, "fp64" if fp64 else "fp32", "absorb", absorb, c, "alive", int(want["alive"].sum()), "responses",
              int(want["first"]["go"].sum()), int(want["second"]["go"].sum()))
        assert c["hit_collider"] + c["hit_scenery"] >= 10, name
        if "collider" in solids:
            assert c["hit_collider"] >= 5 and want["first"]["go"].sum() >= 3, name
        if "scenery" in solids:
            assert c["hit_scenery"] >= 5 and want["second"]["go"].sum() >= 3, name
        assert c["absorbed"] >= 3 if absorb else c["absorbed"] == 0, name
        check_bytes(got, want, name)
        assert cnt == dict(c, born_inside=0, step=steps), name
        assert st["alive"] == want["alive"].sum() and st["died"] == 257 - st["alive"] and st["emitted"] == 0
        if "scenery" not in solids:      # the collider alone: pbf_collider_sample at the advected points, under the stated select
            adv = want["advected"]
            smp = s.collider_sample(p, adv["pos"].astype(np.float64))
            hit = smp["hit"].astype(bool) & adv["alive"]
            lo, hi = np.array(list(p.min_bound), dtype), np.array(list(p.max_bound), dtype)
            moved = np.fmin(hi, np.fmax(lo, smp["moved"] * dtype(p.scale)))
            mine = np.where(hit[:, None], moved, adv["pos"])
            assert np.array_equal(hit, want["hit1"]) and mine[want["alive"]].tobytes() == got["pos"].tobytes(), name


# ---- 2. children ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp64", [True, False], ids=TW.IDS)
def test_children_are_born_outside(pkg, fp64):
    s, p = TW.stepped(pkg, "cubes2048", fp64)
    dtype = np.float64 if fp64 else np.float32
    lat, _ = SR.scenery_plane_through(TW.make_scene(pkg, "cubes2048", fp64), dtype)
    install(s, "scenery", lat, CR.BLOCK_LATTICE["spacing"])
    cfg = TW.configured(s, p, 1 << 16, k_ta=400.0, k_wc=400.0, seed=3)
    plain_stats = s.whitewater_step(p)
    plain = s.whitewater_download()
    s.set_whitewater_solids()
    s.whitewater_configure(**{**cfg, "capacity": (1 << 16) + 1})       # (another capacity: an empty pool, frame 0 again)
    stats = s.whitewater_step(p)
    got, cnt = s.whitewater_download(), s.whitewater_solids_stats()
    assert stats == plain_stats and stats["emitted"] > 257
    fr = CR.frame(p.scale, list(p.min_bound), list(p.max_bound), dtype)
    want, inside = WS.children(dtype, fr, plain["pos"], scenery=lat)
    print("children", stats["emitted"], "born inside", int(inside.sum()), cnt)
    assert inside.sum() >= 20 and cnt == dict(hit_collider=0, hit_scenery=0, absorbed=0, born_inside=int(inside.sum()), step=1)
    assert got["pos"].tobytes() == want.tobytes()
    assert got["pos"][~inside].tobytes() == plain["pos"][~inside].tobytes()
    for k in ("vel", "life", "kind", "parent_id"):
        assert got[k].tobytes() == plain[k].tobytes(), k
    phi, _, _ = CR.project(lat, fr, got["pos"] / fr[0])
    low = phi.astype(np.float64) - float(lat.margin)
    print("lowest phi - margin", low.min(), "bar", CR.plane_bar_world(dtype), "on a face", int(CR.on_face(fr, got["pos"] / fr[0]).sum()))
    assert (low >= -CR.plane_bar_world(dtype)).all()


# ---- 3. resting spray -------------------------------------------------------------------------------------------------------

def far_from_the_fluid(s):
    """the point of a coarse grid over [150, 750]^3 that is farthest from every fluid particle.  50 steps of sliding down the
    tilted plane from rest are 0.5 * (0.23 * 9.8) * (50 dt)^2 * scale = 220 world units towards +x and +z: the particle stays
    well off the walls of the 1100 box, where the box would win over the plane"""
    fl = s.download()["pos"].astype(np.float64)
    g = np.stack(np.meshgrid(*[np.arange(150.0, 751.0, 75.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    d = np.sqrt(((g[:, None, :] - fl[None, ::7, :]) ** 2).sum(-1)).min(1)
    return g[d.argmax()], float(d.max())


@pytest.mark.parametrize("fp64", [True, False], ids=TW.IDS)
def test_spray_comes_to_rest_on_a_plane(pkg, fp64):
    s, p = TW.stepped(pkg, "dam8192", fp64)
    dtype = np.float64 if fp64 else np.float32
    at, room = far_from_the_fluid(s)
    assert room > 250.0                            # (50 steps of free fall from rest are 950 world units: the plane stops it long before)
    n = np.asarray(CR.PLANE_N) / np.linalg.norm(CR.PLANE_N)
    d = float(at @ n) - CR.MARGIN - 10.0           # the particle starts 10 world units above the margin (gravity is +y, n_y < 0)
    lat, fr = CR.plane_case(dtype, d=d, dims=(25, 25, 25), spacing=50.0, origin=(-50.0, -50.0, -50.0))      # (over the whole box)
    install(s, "scenery", lat, 50.0)
    cfg = dict(CFG0, capacity=1)
    s.whitewater_configure(**cfg)
    s.set_whitewater_solids(restitution=0.0, friction=0.0)
    start = dict(pos=at[None, :].astype(dtype), vel=np.zeros((1, 3), dtype), life=np.full(1, 100.0, dtype))
    s.whitewater_upload(**start)
    hits, worst = 0, 0.0
    pfr = CR.frame(p.scale, list(p.min_bound), list(p.max_bound), dtype)
    for k in range(50):
        pool = {key: v for key, v in s.whitewater_download().items() if key in ("pos", "vel", "life")}
        want = expected(s, p, pool, cfg, dtype, dict(scenery=lat), e=0.0, f=0.0)
        st = s.whitewater_step(p)
        got, cnt = s.whitewater_download(), s.whitewater_solids_stats()
        assert st["alive"] == 1 and want["advected"]["nF"][0] == 0 and cnt["step"] == k + 1
        check_bytes(got, want, k)
        height = CR.plane_phi(CR.PLANE_N, d, got["pos"].astype(np.float64))[0]
        assert height >= CR.MARGIN - CR.plane_bar_world(dtype), (k, height)
        if cnt["hit_scenery"]:
            hits += 1
            assert want["second"]["go"][0]
            nk = want["second"]["n"][0].astype(np.float64)
            speed = float(np.sqrt((want["advected"]["vel"][0].astype(np.float64) ** 2).sum()))
            vn = abs(float(got["vel"][0].astype(np.float64) @ nk))
            worst = max(worst, vn / speed)
            assert vn <= WS.bar_speed(dtype, WS.NORMAL_UNITS, speed), (k, vn, speed)
    print("hits", hits, "worst normal speed / speed", worst, "bar", WS.bar_speed(dtype, WS.NORMAL_UNITS, 1.0))
    assert hits >= 30
    # absorb: gone with the first hit
    s.set_whitewater_solids(restitution=0.0, friction=0.0, absorb=True)
    s.whitewater_upload(**start)
    for k in range(50):
        st = s.whitewater_step(p)
        cnt = s.whitewater_solids_stats()
        if cnt["hit_scenery"]:
            assert cnt["absorbed"] == 1 and st["died"] == 1 and st["alive"] == 0 and s.whitewater_count == 0
            break
        assert st["alive"] == 1 and st["died"] == 0 and cnt["absorbed"] == 0
    else:
        raise AssertionError("the particle never reached the plane")
    assert 2 <= k <= 20


# ---- 4. off is off ----------------------------------------------------------------------------------------------------------

def solids_in_the_fluid(pkg, s, name, fp64):
    """a plane through the scene's fluid as scenery and a ball about its centroid as the collider -> (plane, ball)"""
    dtype = np.float64 if fp64 else np.float32
    sc = TW.make_scene(pkg, name, fp64)
    lat, _ = SR.scenery_plane_through(sc, dtype)
    c = sc["pos"][sc["type"] == 0].astype(np.float64).mean(0)
    B = CR.BLOCK_LATTICE
    ball = CR.Lattice(CR.lattice_of(lambda x: CR.sphere_phi(c, 90.0, x), B["origin"], B["spacing"], B["dims"]), B["origin"], B["spacing"],
                      CR.MARGIN, dtype)
    install(s, "scenery", lat, B["spacing"])
    install(s, "collider", ball, B["spacing"])
    return lat, ball


def sequence(pkg, mode, options=None, frames=5, timing=False):
    """cubes2048 with the two solids, whitewater at rates that emit; mode: "never", "cleared" (set, then NULL), "on", or
    "bare" (on, no lattice installed) / "bare-off" -> (pool bytes per frame, counts per frame, solver)"""
    K, steps, side = TW.SCENES["cubes2048"]
    s = pkg.Solver(h=H, flags=pkg.FLAG_STAGE_TIMING if timing else 0)
    for k, v in (options or {}).items():
        s.set_option(k, v)
    p = pkg.default_params(K, side)
    s.upload(**TW.make_scene(pkg, "cubes2048", False))
    if not mode.startswith("bare"):
        solids_in_the_fluid(pkg, s, "cubes2048", False)
    s.steps(p, steps)
    if mode == "cleared":
        s.set_whitewater_solids(restitution=0.5, friction=0.5)
    TW.configured(s, p, 4096, k_ta=200.0, k_wc=200.0, seed=7)
    if mode == "cleared":
        s.set_whitewater_solids(off=True)
    if mode in ("on", "bare"):
        s.set_whitewater_solids(restitution=0.5, friction=0.5)
    out, cnt = [], []
    for _ in range(frames):
        s.step(p)
        s.whitewater_step(p)
        out.append(TW.pool_bytes(s))
        if mode in ("on", "bare"):
            cnt.append(s.whitewater_solids_stats())
    return out, cnt, s


def test_set_then_cleared_is_never_set(pkg):
    from pbf_sph_amd import capi
    never, _, a = sequence(pkg, "never", timing=True)
    cleared, _, b = sequence(pkg, "cleared", timing=True)
    assert never == cleared and len(never[-1]) > 500 * 37
    assert {k: v[1] for k, v in a.stage_times().items()} == {k: v[1] for k, v in b.stage_times().items()}
    assert b.L.pbf_whitewater_solids_stats(b.ctx, C.byref(capi.WhitewaterSolidsStats())) == ERR_STATE
    on, cnt, c = sequence(pkg, "on", timing=True)
    assert on != never and sum(x["hit_collider"] + x["hit_scenery"] + x["born_inside"] for x in cnt) > 0
    assert {k: v[1] for k, v in a.stage_times().items()} == {k: v[1] for k, v in c.stage_times().items()}


def test_on_without_a_lattice_is_off(pkg):
    off, _, _ = sequence(pkg, "bare-off")
    on, cnt, _ = sequence(pkg, "bare")
    assert on == off and len(on[-1]) > 500 * 37
    assert cnt == [dict(hit_collider=0, hit_scenery=0, absorbed=0, born_inside=0, step=k + 1) for k in range(5)]


@pytest.mark.parametrize("graph", [0, 1])
def test_a_fluid_step_never_notices(pkg, graph):
    def run(with_ww):
        K, _, side = TW.SCENES["dam8192"]
        s = pkg.Solver(h=H, flags=0 if graph else pkg.FLAG_STAGE_TIMING)      # (eager: the stages' call counts are the launches)
        s.set_option("graph", graph)
        p = pkg.default_params(K, side)
        s.upload(**TW.make_scene(pkg, "dam8192", False))
        solids_in_the_fluid(pkg, s, "dam8192", False)
        if with_ww:
            s.whitewater_configure(capacity=4096, k_ta=50.0, k_wc=50.0, tau_ta=(0.0, 0.5), tau_wc=(0.0, 0.5), tau_k=(0.0, 0.01))
            s.set_whitewater_solids(restitution=0.3, friction=0.3, absorb=True)
        for _ in range(10):
            s.steps(p, 1)
            if with_ww:
                s.whitewater_step(p)
        return s.download(), s.graph_stats(), s

    (a, ga, sa), (b, gb, sb) = run(True), run(False)
    assert all(np.array_equal(a[k], b[k]) for k in a) and ga == gb
    if not graph:
        calls = {k: v[1] for k, v in sa.stage_times().items()}
        assert calls == {k: v[1] for k, v in sb.stage_times().items()} and sum(calls.values()) > 0
    assert sa.whitewater_solids_stats()["step"] == 10
    if graph:
        assert ga[1] > 0


# ---- 5. paths ---------------------------------------------------------------------------------------------------------------

def test_same_sequence_same_bytes_on_every_gather_kernel(pkg):
    base, cnt, _ = sequence(pkg, "on")
    assert len(base[-1]) > 500 * 37 and sum(x["hit_collider"] + x["hit_scenery"] for x in cnt) > 0 and sum(x["born_inside"] for x in cnt) > 0
    again, cnt2, _ = sequence(pkg, "on")
    assert again == base and cnt2 == cnt
    for options in ({"gather": 0}, {"gather": 3}, {"row_major": 0}, {"gather": 0, "row_major": 0}):
        other, cnt3, _ = sequence(pkg, "on", options)
        assert other == base and cnt3 == cnt, options


# ---- 6. stats and refusals --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("capacity", [1, 65, 257])
def test_counts_follow_the_installed_lattices(pkg, capacity):
    s, p = TW.stepped(pkg, "dam8192", False)
    dtype = np.float32
    cfg = dict(CFG0, capacity=capacity)
    s.whitewater_configure(**cfg)
    s.set_whitewater_solids(restitution=1.0, friction=1.0, absorb=True)
    plane, ball, _, _ = SR.wedge_case(dtype)
    rng = np.random.default_rng(31)
    where = lambda n: np.concatenate([ball_points(rng, n - n // 3), plane_points(rng, n // 3, CR.PLANE_N, SR.WEDGE_PLANE_D)])
    pool = pool_for(s, p, capacity, dtype, where)
    install(s, "collider", ball, SR.WEDGE_SPACING)
    install(s, "scenery", plane, SR.WEDGE_SPACING)
    seen = []
    for step, solids in enumerate((dict(collider=ball, scenery=plane), dict(scenery=plane), dict()), 1):
        s.whitewater_upload(**pool)
        want = expected(s, p, pool, cfg, dtype, solids, e=1.0, f=1.0, absorb=True)
        st = s.whitewater_step(p)
        check_bytes(s.whitewater_download(), want, step)
        cnt = s.whitewater_solids_stats()
        assert cnt == dict(WS.counts(want), born_inside=0, step=step) and st["died"] == capacity - want["alive"].sum()
        seen.append(cnt)
        if step == 1:
            s.set_collider(None)
        if step == 2:
            s.set_scenery(None)
    print(capacity, seen)
    assert seen[2] == dict(hit_collider=0, hit_scenery=0, absorbed=0, born_inside=0, step=3) and seen[1]["hit_collider"] == 0
    if capacity > 1:
        assert seen[0]["hit_collider"] > 0 and seen[0]["hit_scenery"] > 0 and seen[1]["hit_scenery"] > 0 and seen[0]["absorbed"] > 0
    else:
        assert seen[0]["hit_collider"] + seen[0]["hit_scenery"] == 1


def test_refusals(pkg):
    from pbf_sph_amd import capi
    s, p = TW.stepped(pkg, "cubes2048", False)
    L, SolidsCfg, Stats = s.L, capi.WhitewaterSolids, capi.WhitewaterSolidsStats
    st = Stats()
    stats = lambda: L.pbf_whitewater_solids_stats(s.ctx, C.byref(st))
    assert stats() == ERR_STATE                                       # never set
    s.whitewater_configure(**dict(CFG0, capacity=65))
    pts = np.random.default_rng(1).random((40, 3)) * 300 + 100
    s.whitewater_upload(pts)
    kept = TW.pool_bytes(s)
    for bad in (dict(restitution=-0.1), dict(restitution=1.5), dict(restitution=float("nan")), dict(friction=-1e-9), dict(friction=2.0),
                dict(friction=float("nan")), dict(reserved=1)):
        assert not WS.settings_ok(**bad)
        c = SolidsCfg(bad.get("restitution", 0.0), bad.get("friction", 0.0), 0, bad.get("reserved", 0))
        assert L.pbf_set_whitewater_solids(s.ctx, C.byref(c)) == ERR_INVALID, bad
        assert stats() == ERR_STATE and TW.pool_bytes(s) == kept      # (the ctx unchanged: still off)
    s.set_whitewater_solids(restitution=1.0, friction=0.0)
    assert stats() == ERR_STATE                                       # set, no whitewater step since
    assert L.pbf_whitewater_solids_stats(s.ctx, None) == ERR_INVALID
    s.whitewater_step(p)
    assert stats() == 0 and st.step == 1
    c = SolidsCfg(2.0, 0.0, 0, 0)
    assert L.pbf_set_whitewater_solids(s.ctx, C.byref(c)) == ERR_INVALID and stats() == 0 and st.step == 1      # a refused change: still on
    s.set_whitewater_solids(restitution=0.2, friction=0.4, absorb=True)                                          # a change keeps the count
    s.whitewater_step(p)
    assert stats() == 0 and st.step == 2
    s.set_whitewater_solids(None)
    assert stats() == ERR_STATE
    s.set_whitewater_solids()
    assert stats() == ERR_STATE                                       # on again: the count starts again
    s.whitewater_step(p)
    assert stats() == 0 and st.step == 1
    # the setting outlives the solids and the pool's capacity
    lat, _ = SR.scenery_plane_through(TW.make_scene(pkg, "cubes2048", False), np.float32)
    install(s, "scenery", lat, CR.BLOCK_LATTICE["spacing"])
    s.set_scenery(None)
    s.whitewater_configure(**dict(CFG0, capacity=257))
    s.whitewater_step(p)
    assert stats() == 0 and st.step == 2


# ---- 7. shim and CLI --------------------------------------------------------------------------------------------------------

def test_shim(pkg):
    r = subprocess.run([os.path.join(ROOT, "pbf-sph_amd", "test_whitewater_solids_shim")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr


def test_benchmark_flag(pkg, tmp_path):
    BIN = os.path.join(ROOT, "pbf-sph_amd", "benchmark")
    out = tmp_path / "out"
    common = ["--resident", "--scene", "dam-break", "--particles", "8192", "--solver-iter", "2", "--no-surface", "-n", "12", "-w", "4",
              "-o", str(out)]
    r = subprocess.run([BIN, *common, "--whitewater=300,300,20000", "--scenery=plane:0,-1,0,-1000", "--whitewater-solids=0.2,0.5,1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"Whitewater solids\s+: last frame: (\d+) hit the collider, (\d+) hit the scenery, (\d+) absorbed, (\d+) born inside \((\d+) steps\)",
                  r.stdout)
    assert m and int(m.group(1)) == 0 and int(m.group(5)) >= 12, r.stdout
    assert (out / "whitewater.ply").exists()
    r = subprocess.run([BIN, *common, "--whitewater-solids"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--whitewater-solids needs --whitewater" in r.stderr
    r = subprocess.run([BIN, *common, "--whitewater=1,1", "--whitewater-solids=1.5"], capture_output=True, text=True, timeout=300)
    assert "--whitewater-solids: restitution and friction in [0, 1]" in r.stdout + r.stderr and "Whitewater solids" not in r.stdout
