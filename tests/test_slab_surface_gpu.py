"""pbf_surface in slab mode, held to the float64 field and to the global mesh: several ranks share one GPU (gloo, the
host-callback transport), each extracts its part of the global lattice after pbf_slab_step.

Per case of mc_scenes.SLAB_PARAMS, precision and parameter set:
  1. every rank's lattice has the global sample on y and z and, on x, the planes tests/test_slab_surface_cpu.py's
     owned_planes gives it (restated from the field kernel's node-cell expression) plus the plane received from the right;
  2. that received plane is the right-hand neighbour's first plane, byte for byte;
  3. the global lattice assembled from the ranks' own planes lies within tests/nversion_mc.py's derived bound of the
     all-pairs float64 evaluation on the merged owned particles of the final download — the conditions of
     tests/test_mc_field_gpu.py, nothing wider;
  4. the ranks' meshes, concatenated in rank order, equal the oracle's emit stage on that assembled lattice bit for bit;
  5. a parameter set that leaves an interior rank without a node plane is refused by every rank with PBF_ERR_INVALID, without
     an exchange, and the next set passes 1 to 4;
  6. after the download, pbf_surface and pbf_surface_indexed return PBF_ERR_STATE on every rank.
tests/test_slab_surface_cpu.py proves that 3 catches a missing ghost layer and a shifted plane.
"""
import numpy as np
import pytest

import mc_scenes as M
import nversion_mc as NM
from test_slab_cpu import launch
from test_slab_surface_cpu import plane_ranges

pytestmark = pytest.mark.gpu

PBF_ERR_INVALID, PBF_ERR_STATE = -1, -4
KEYS = ("id", "type", "mass", "pos", "vel", "colour")


def merged(parts, prefix=""):
    cat = {k: np.concatenate([p[prefix + k] for p in parts]) for k in KEYS}
    o = np.argsort(cat["id"], kind="stable")
    return {k: v[o] for k, v in cat.items()}


def lat_nodes(s, mc, fp64):
    return M.lattice_of(s, mc, fp64).n_nodes


def spec_of(sets):
    return ";".join(("!" if mc[0] == "!" else "") + ",".join(repr(float(v)) for v in mc if v != "!") for mc in sets)


def check_set(oracle, s, case, fp64, parts, i, mc, st, cells):
    dtype = np.float64 if fp64 else np.float32
    world = len(parts)
    lat = M.lattice_of(s, mc, fp64)
    assert int(lat.extent[0]) == case["extent_x"]
    sample_x, rng = plane_ranges(case["columns"], mc[0], case["extent_x"], dtype)
    assert sample_x == lat.sample[0]
    per = int(lat.sample[1] * lat.sample[2])
    own_pn, own_c, tris = [], [], []
    # 1. the shape of every rank's lattice
    for r, (x0, n) in enumerate(rng):
        smp = [int(v) for v in parts[r][f"surf{i}_sample"]]
        extra = 1 if r + 1 < world and x0 + n < sample_x else 0
        assert smp[1:] == [int(lat.sample[1]), int(lat.sample[2])], (r, smp)
        assert smp[0] == n + extra, (r, smp, n, extra)
        pn, c = parts[r][f"surf{i}_pn"], parts[r][f"surf{i}_c"]
        assert pn.dtype == dtype and pn.shape == c.shape == (smp[0] * per, 4)
        own_pn.append(pn[:n * per]), own_c.append(c[:n * per])
        assert int(parts[r][f"surf{i}_rounds"]) <= 3, "the colour round and the two halves of one plane"
        tris.append(len(parts[r][f"surf{i}_vs"]) // 3)
    assert sum(n for _, n in rng) == lat.sample[0]
    # 2. the received plane is the neighbour's first one, byte for byte (normals and colours may be NaN)
    for r, (x0, n) in enumerate(rng[:-1]):
        if x0 + n < sample_x:
            assert rng[r + 1][1] > 0
            for key, own in (("pn", own_pn), ("c", own_c)):
                got = parts[r][f"surf{i}_{key}"][n * per:]
                assert got.tobytes() == own[r + 1][:per].tobytes(), (r, key)
    # 3. the assembled global lattice against the float64 evaluation
    pn, c = np.concatenate(own_pn), np.concatenate(own_c)
    rep = NM.compare(pn, c, st["pos"], st["colour"], st["type"], cells, lat, mc[2], mc[3], dtype)
    tag = f"RATIO slab {case['scene']} cuts {case['cuts']} {mc} {'f64' if fp64 else 'f32'}"
    print(tag, NM.summary(rep), "triangles per rank", tris)
    assert rep["pattern_bad"] == 0, (mc, NM.summary(rep))
    assert rep["worst"] <= 1, (mc, NM.summary(rep))
    assert rep["left_out"] <= 0.01 * rep["with_hits"], (mc, NM.summary(rep))
    if fp64:
        assert rep["rv_bar"] <= 1, "fp64 must also meet 1e-12 of the sum of |terms|"
    far = ~rep["ev"]["evaluated"]
    if "early" in rep["ev"]:
        far[rep["ev"]["early"]] = False
    assert (pn[far, 0] == 0).all() and np.isnan(pn[far, 1:]).all() and np.isnan(c[far]).all()
    # 4. the concatenated meshes against the oracle's emit stage on the assembled lattice
    o = oracle.Oracle(fp64, device_pow=True)
    o.set_particles(**st)
    q = M.oracle_params(s)
    o.predict(q)                                            # (the grid's origin, which the emit stage's coordinates start from)
    e = o.surface(q, oracle.OracleMc(*mc), lattice=(lat.sample, pn, c))
    assert len(e["vs"]) >= 3 * 80, "a non-trivial mesh"
    for k in ("vs", "ns", "cs"):
        got = np.concatenate([parts[r][f"surf{i}_{k}"] for r in range(world)])
        assert got.dtype == e[k].dtype and np.array_equal(got, e[k], equal_nan=True), (k, len(got), len(e[k]))
    return rep, tris


CASES = [(n, d) for n, c in M.SLAB_PARAMS.items() for d in c["fp64"]]


@pytest.mark.parametrize("name,fp64", CASES, ids=[f"{n}-{'f64' if d else 'f32'}" for n, d in CASES])
def test_slab_surface_within_derived_bound_and_equal_to_the_global_mesh(pkg, oracle, tmp_path, name, fp64):
    case = M.SLAB_PARAMS[name]
    s = M.make(case["scene"])
    world = len(case["columns"]) - 1
    dtype = np.float64 if fp64 else np.float32
    args = ("--engine", "hipc", "--scene", "mc:" + case["scene"], "--cuts", case["cuts"]) + (("--fp64",) if fp64 else ())
    parts = launch(world, str(tmp_path / "run"), *args, "--steps", str(s["frames"]), "--surface", spec_of(case["sets"]),
                   timeout=300)
    assert all(list(p["cuts"]) == list(case["columns"]) for p in parts)
    st = merged(parts)
    assert st["pos"].dtype == dtype and np.array_equal(st["id"], np.sort(s["sc"]["id"]))
    if s["frames"] == 1:
        before = M.cast(s["sc"], dtype)
    else:  # the state before the last step: the same run, one step shorter (bit for bit the same run: test_slab_gpu.py)
        before = merged(launch(world, str(tmp_path / "before"), *args, "--steps", str(s["frames"] - 1), timeout=300))
    cells = M.predict_time_cells(before, s, st["id"])
    fluid = st["type"] != NM.OBSTACLE
    ext = M.lattice_of(s, case["sets"][0], fp64).extent
    assert (cells[fluid] >= 0).all() and (cells[fluid] < ext).all(), "a particle outside the grid"
    refused_before = False
    for i, mc in enumerate(case["sets"]):
        if mc[0] == "!":  # 5. refused by every rank alike, nothing exchanged
            for r in range(world):
                assert int(parts[r][f"surf{i}_rc"]) == PBF_ERR_INVALID and int(parts[r][f"surf{i}_rounds"]) == 0, r
            refused_before = True
            continue
        rep, tris = check_set(oracle, s, case, fp64, parts, i, mc, st, cells)
        refused_before = False
        # a rank that owns no particle and got no copy: its planes are far nodes, and it emits nothing
        owner = np.searchsorted(case["columns"], cells[:, 0], side="right") - 1
        for r in range(world):
            lo, hi = case["columns"][r], case["columns"][r + 1]
            if not ((cells[:, 0] >= lo - 1) & (cells[:, 0] <= hi)).any():
                assert not (owner == r).any() and len(parts[r]["id"]) == 0
                pn, c = parts[r][f"surf{i}_pn"], parts[r][f"surf{i}_c"]
                nan = np.ones(len(pn), bool)
                if "early" in rep["ev"] and r == world - 1:  # the (extent, extent, extent) node keeps its zeros: the last one
                    assert rep["ev"]["early"] == lat_nodes(s, mc, fp64) - 1 and (pn[-1] == 0).all() and (c[-1] == 0).all()
                    nan[-1] = False
                assert len(pn) > 0 and (pn[:, 0] == 0).all() and np.isnan(pn[nan, 1:]).all() and np.isnan(c[nan]).all()
                assert tris[r] == 0
    assert not refused_before, "a set follows the refused one"
    if name == "blob-empty":
        assert len(parts[1]["id"]) == 0 == len(parts[2]["id"])
    if name == "faces-4":
        assert any(mc[0] == "!" for mc in case["sets"]) and len(parts[2]["id"]) > 50
    if name == "obstacles-3":
        assert ((st["type"] == NM.OBSTACLE) & (cells[:, 0] == 5)).sum() > 50
        assert ((st["type"] == NM.OBSTACLE) & (cells[:, 0] == 6)).sum() > 50
    # 6. the download dropped the copies: both entry points refuse, and nothing is exchanged
    for r in range(world):
        assert list(parts[r]["after_rc"]) == [PBF_ERR_STATE, PBF_ERR_STATE] and int(parts[r]["after_rounds"]) == 0, r


def test_download_between_slab_steps(pkg, tmp_path):
    """A download between two slab steps drops the copies and flips the arrays; the next step starts without old copies
    and must arrive where the undisturbed run does, bit for bit — and what the download returned is the 2-step run."""
    args = ("--engine", "hipc", "--scene", "cubes2048", "--cuts", "x:210,700")
    peek = launch(3, str(tmp_path / "peek"), *args, "--steps", "5", "--peek-at", "2", timeout=300)
    plain = launch(3, str(tmp_path / "plain"), *args, "--steps", "5", timeout=300)
    two = launch(3, str(tmp_path / "two"), *args, "--steps", "2", timeout=300)
    for r in range(3):
        assert len(plain[r]["id"]) > 0
        for k in KEYS:
            assert np.array_equal(peek[r][k], plain[r][k]), (r, k)
            assert np.array_equal(peek[r]["peek_" + k], two[r][k]), (r, k)
