"""Whitewater without a device: the float64 restatement (tests/whitewater_ref.py) against closed forms, the hash against
words computed by hand, the ctypes structures against the header, and the refusals that need no context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import whitewater_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 0.1
CFG = dict(k_ta=100.0, k_wc=100.0, tau_ta=(0.0, 1.0), tau_wc=(0.0, 1.0), tau_k=(0.0, 1.0), spray_below=6, bubble_from=20)


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pbf_hip.h")).read(), flags=re.S)


def test_head_on_pair_traps_air():
    """two particles approaching head-on: cos = -1, so I_ta = 2 |v_ij| W with W = 1 - r / h; receding: 0"""
    for v, r in ((1.0, 0.05), (0.25, 0.08), (3.0, 0.0125)):
        down, ps = WR.mutate_head_on(v, r, H)
        out = WR.potentials(down, ps, np.zeros(2, np.uint32), 10, H, CFG, 0.01, 0, np.float64)
        want = 2.0 * (2.0 * v) * (1.0 - r / H)
        assert np.allclose(out["I_ta"], want, rtol=1e-14, atol=0)
        assert np.allclose(out["E_k"], 0.5 * v * v, rtol=1e-15) and list(out["nbr"]) == [2, 2]
        down["vel"] = -down["vel"]
        assert np.allclose(WR.potentials(down, ps, np.zeros(2, np.uint32), 10, H, CFG, 0.01, 0, np.float64)["I_ta"], 0.0, atol=1e-15)
    # beyond h the pair does not see each other; at rest nothing is trapped and nothing is emitted
    down, ps = WR.mutate_head_on(1.0, 0.11, H)
    assert not WR.potentials(down, ps, np.zeros(2, np.uint32), 10, H, CFG, 0.01, 0, np.float64)["I_ta"].any()
    down, ps = WR.mutate_head_on(0.0, 0.05, H)
    out = WR.potentials(down, ps, np.zeros(2, np.uint32), 10, H, CFG, 0.01, 0, np.float64)
    assert not out["I_ta"].any() and not out["n_d"].any()


def test_flat_sheet_has_no_curvature():
    """a flat sheet, two lattice layers thick (a single symmetric layer has n = 0 exactly): away from the rim every normal
    of the top layer is along z, its neighbours' normals are parallel to it, and the layer below lies on the normal's own
    side: kappa = 0"""
    m = 15
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2) * 0.04
    ps = np.concatenate([g + 1.0, np.full((len(g), 1), 1.0), np.zeros((len(g), 1))], 1)
    lower = ps.copy()
    lower[:, 2] -= 0.04
    allp = np.concatenate([ps, lower])
    n = len(allp)
    down = dict(mass=np.ones(n), type=np.zeros(n, np.uint8), vel=np.tile([0.0, 0.0, 1.0], (n, 1)), id=np.arange(n, dtype=np.uint64))
    out = WR.potentials(down, allp, np.zeros(n, np.uint32), 10, H, CFG, 0.01, 0, np.float64)
    ij = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2)
    inner = ((ij >= 6) & (ij <= m - 7)).all(1)
    top = np.concatenate([inner, np.zeros(len(g), bool)])
    nrm = out["normal"][top]
    assert np.abs(nrm[:, :2]).max() <= 1e-9 * np.abs(nrm[:, 2]).min() and (np.abs(nrm[:, 2]) > 0).all()
    assert np.abs(out["kappa"][top]).max() <= 1e-12
    assert not out["I_ta"][top].any()          # rigid motion traps nothing


def test_hash_words_by_hand():
    """splitmix64's published first outputs for seed 0 (state += gamma, then the finaliser) and the 24-bit unit"""
    assert WR.mix(0) == 0xE220A8397B1DCDAF
    assert WR.mix(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert WR.mix(2 * 0x9E3779B97F4A7C15 & WR.M64) == 0x06C45D188009454F
    w = WR.mix(7 ^ WR.mix(42) ^ WR.mix((3 << 32) + 2 * 4 + 1))
    assert WR.unit(7, 42, 3, 2, 1) == (w >> 40) / 16777216.0
    us = [WR.unit(1, i, 0, 0, 0) for i in range(2000)]
    assert 0.0 <= min(us) and max(us) < 1.0 and abs(np.mean(us) - 0.5) < 0.03
    assert all(np.float32(x) == x for x in us)
    assert WR.unit(1, 5, 0, 0, 0) != WR.unit(2, 5, 0, 0, 0) != WR.unit(1, 5, 1, 0, 0)


def test_phi_counts_and_classes():
    tau = (1.0, 3.0)
    assert list(WR.phi(np.array([0.0, 1.0, 2.0, 3.0, 9.0]), tau)) == [0.0, 0.0, 0.5, 1.0, 1.0]
    ids = np.arange(50, dtype=np.uint64)
    c = WR.counts(np.full(50, 2.25, np.float32), 9, ids, 4, np.float32)
    assert set(c) <= {2, 3} and (c == 3).any() and (c == 2).any()
    assert list(WR.counts(np.array([np.nan, 1e9], np.float32), 9, ids[:2], 4, np.float32)) == [0, 1024]
    assert list(WR.classify([0, 5, 6, 19, 20, 99], 6, 20)) == [0, 0, 1, 1, 2, 2]


def test_struct_layout_matches_the_header(pkg):
    from pbf_sph_amd import capi
    assert C.sizeof(capi.Whitewater) == 2 * 8 + 2 * 8 + 4 * 16 + 2 * 8 + 2 * 4 == 120
    assert C.sizeof(capi.WhitewaterStats) == 7 * 8
    code = header()
    body = re.search(r"typedef struct pbf_whitewater \{(.*?)\} pbf_whitewater;", code, flags=re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d\])?\s*[,;]", body)
    assert names == [n for n, _ in capi.Whitewater._fields_]
    body = re.search(r"typedef struct pbf_whitewater_stats \{(.*?)\} pbf_whitewater_stats;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d\])?\s*[,;]", body) == [n for n, _ in capi.WhitewaterStats._fields_]
    assert re.search(r"PBF_BUF_WHITEWATER = 7,", code) and pkg.BUF_WHITEWATER == 7
    assert re.search(r"PBF_WW_SPRAY = 0, PBF_WW_FOAM = 1, PBF_WW_BUBBLE = 2", code)
    assert (pkg.WW_SPRAY, pkg.WW_FOAM, pkg.WW_BUBBLE) == (WR.SPRAY, WR.FOAM, WR.BUBBLE) == (0, 1, 2)
    assert re.search(r"#define PBF_ABI_VERSION 1\b", code)
    for f in ("configure", "upload", "step", "count", "download"):
        assert "pbf_whitewater_" + f in capi.exported_symbols() and hasattr(C.CDLL(pkg.LIB_PATH), "pbf_whitewater_" + f)
    for m in ("whitewater_configure", "whitewater_step", "whitewater_download", "whitewater_upload"):
        assert callable(getattr(pkg.Solver, m))


def test_refusals_without_a_context(pkg):
    L = pkg.lib()
    w = pkg.whitewater_config(capacity=16, tau_ta=(0, 1), tau_wc=(0, 1), tau_k=(0, 1))
    assert (w.spray_below, w.bubble_from, w.k_d) == (6, 20, 0.8)
    p = pkg.default_params(2, 1000.0)
    st = pkg.WhitewaterStats()
    assert L.pbf_whitewater_configure(None, C.byref(w)) == -1
    assert L.pbf_whitewater_step(None, C.byref(p), C.byref(st)) == -1
    assert L.pbf_whitewater_upload(None, 0, None, None, None) == -1
    assert L.pbf_whitewater_download(None, None, None, None, None, None) == -1
    assert L.pbf_whitewater_count(None) == 0


# ---- the ambiguity cap on the oracle's state -----------------------------------------------------------------------------

def oracle_state(name):
    """the oracle's float64 state of the GPU test's scenes: cubes2048 after 5 steps (K = 4), dam8192 after 30 (K = 2),
    cubes2048 with every fifth particle an obstacle and unequal masses after 3 (K = 2)"""
    import oracle_lib as O
    K, steps, side = {"cubes2048": (4, 5, 1000.0), "dam8192": (2, 30, 1100.0), "obstacles2048": (2, 3, 1000.0)}[name]
    sc = O.scene_dambreak(8192, True)[0] if name == "dam8192" else O.scene_cubes(2048, True)
    if name == "obstacles2048":
        sc["type"][::5] = 1
        sc["mass"] = 0.5 + np.random.default_rng(17).random(len(sc["id"]))
    q = O.make_params(iteration=K, mode=O.JACOBI, sort=O.SORT_STABLE, max_bound=(side,) * 3)
    o = O.Oracle(True)
    o.set_particles(**sc)
    for _ in range(steps):
        o.step(q)
    return dict(down=o.get_particles(), pstar=o.pstar().astype(np.float64), keys=o.keys().astype(np.uint32),
                table_size=len(o.table()), dt=q.dt)



@pytest.mark.parametrize("name", ["cubes2048", "dam8192", "obstacles2048"])
def test_the_restatement_leaves_out_at_most_two_percent(name):
    """with the fp32 windows (the wider ones) the particles with an ambiguous candidate or test stay within the cap the
    GPU test allows, on the oracle's state of its scenes; and the scenes have something to measure"""
    st = oracle_state(name)
    out = WR.potentials(st["down"], st["pstar"], st["keys"], st["table_size"], float(np.float32(H)), CFG, st["dt"], 0, np.float32)
    fluid = st["down"]["type"] == 0
    share = out["ambiguous"].sum() / fluid.sum()
    print(name, "ambiguous", int(out["ambiguous"].sum()), "of", int(fluid.sum()), f"= {share:.4%}",
          "I_ta > 0:", int((out["I_ta"] > 0).sum()), "I_wc > 0:", int((out["I_wc"] > 0).sum()))
    assert share <= 0.02
    assert (out["I_ta"] > 0).sum() > 100 and (out["E_k"] > 0).sum() > 100
