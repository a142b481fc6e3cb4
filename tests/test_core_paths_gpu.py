"""Every arithmetic variant of the solver core — fp32 / fp64, PRECISE / PBF_FLAG_FAST_MATH, one lane per particle / option
`coop` — held stage by stage and particle by particle to tests/core_ref.py's bars (validated on the CPU by
tests/test_core_ref_cpu.py), through the staged API only: predict, sort, then two iterations of lambda, delta.

  a. lambda and the delta-p move under the DERIVED bar alone, FAST included (every FAST case measured stays below it, so the
     inherited fast-math allowance is not used here; each case prints what it needs), on eight scenes — the seven of the
     opt-in passes' file and cubes1024's start lattice, the one with lists on either side of the 40 row slots
     (core_ref.SCENES); `split_build = 5` makes lambda list-driven, so that
     k_gather_from_lists_coop<N, LambdaOp, K> runs too — with obstacles (begin() false inside a live group), NBR_OVERFLOW
     particles (lane 0 walks alone), lists that end inside a two-entry trip and n that is no multiple of BLOCK / COOP;
  b. under FAST every other launch path gives the default FAST path's bytes (same op code, same candidate
     order), no collider, no extras;
  c. every variant of (a) gives the same bytes when run twice.

cubes1024 takes its three warm steps on the default PRECISE solver of the same type, whose state every variant then uploads:
the pStar after the sort, hence the pairs and the first lambda reference, are shared by all variants of a type.
"""
import time

import numpy as np
import pytest

import core_ref as CR
import extras_ref as ER
import nversion as NV
from sample_ref import key_cells
from test_nversion_cpu import scene

pytestmark = pytest.mark.gpu

H = 0.1
OVERFLOW = 0xFFFFFFFF
ARITHMETIC = [(False, False), (False, True), (True, False), (True, True)]   # (fp64, PBF_FLAG_FAST_MATH)
ARITHMETIC_IDS = ["fp32", "fp32-fast", "fp64", "fp64-fast"]
# (coop, split_build): 5 = a list build of its own, lambda AND delta-p list-driven; 8 (default) = lambda rides on the build
READERS = [(0, 5), (2, 5), (4, 5), (8, 5), (2, 8), (4, 8), (8, 8)]
READER_IDS = [f"coop{c}-split{s}" for c, s in READERS]

_START, _FIRST, _SORTED, _LAMBDA0 = {}, {}, {}, {}


def params(pkg, name):
    p = pkg.default_params(CR.ITERATIONS, 1000.0)
    for c in range(3):
        p.constant_force[c] = CR.SCENES[name][1][c]
    return p


def start_state(pkg, name, fp64):
    """the scene after its warm steps on the default PRECISE solver: what every variant uploads"""
    if (name, fp64) not in _START:
        sc = scene(CR.base(name)) if name != "two_tier" else two_tier_scene()
        warm = CR.SCENES[name][0] if name in CR.SCENES else 0
        if warm:
            sc = pkg.Solver(h=H, fp64=fp64).upload(**sc).steps(params(pkg, name), warm).download()
        _START[name, fp64] = sc
    return _START[name, fp64]


def solver(pkg, fp64, fast, coop=0, split=8, flags=0, **options):
    s = pkg.Solver(h=H, fp64=fp64, flags=(pkg.FLAG_FAST_MATH if fast else 0) | flags)
    if coop:
        s.set_option("coop", coop)
    if split != 8:
        s.set_option("split_build", split)
    for k, v in options.items():
        s.set_option(k, v)
    return s


def staged(pkg, name, fp64, fast, coop, split, **options):
    """-> the solver after predict and sort, its parameters"""
    p = params(pkg, name)
    s = solver(pkg, fp64, fast, coop, split, **options).upload(**start_state(pkg, name, fp64))
    return s.stage("predict", p).stage("sort", p), p


def hold_case(pkg, name, fp64, fast, coop, split, **options):
    """(a) for one case -> (records of core_ref.hold_iterations, list lengths after the first build, first lambdas)"""
    dtype = np.float64 if fp64 else np.float32
    s, p = staged(pkg, name, fp64, fast, coop, split, **options)
    st = s.download()
    keys, ids = s.keys(), st["id"]
    assert keys.max() < len(s.table())
    want = _SORTED.setdefault((name, fp64), (keys, ids, s.pstar()[:, :3].copy()))
    assert np.array_equal(keys, want[0]) and np.array_equal(ids, want[1]), "keys and sorted ids are every variant's"
    ps0 = s.pstar()[:, :3]
    assert np.array_equal(ps0, want[2])
    obstacle = st["type"] == 1
    h = ER.kernel_inputs(dtype, H, p.dt)[0]
    cells = NV.predict_cells(ps0.astype(np.float64), h, p.scale, list(p.min_bound))
    kc = key_cells(keys).astype(np.int64)
    assert np.array_equal(cells - cells.min(0), kc - kc.min(0))
    seen = {}

    def stage_lambda():
        s.stage("lambda", p)
        got = s.pstar()
        seen.setdefault("counts", s.nbr_counts())
        seen.setdefault("lambda", got[:, 3].copy())
        assert not got[obstacle, 3].any(), "an obstacle's lambda is 0"
        assert np.array_equal(got[obstacle, :3], seen.get("pstar", ps0)[obstacle]), "an obstacle keeps its pStar"
        return got[:, 3]

    def stage_delta():
        before = s.pstar()
        s.stage("delta", p)
        got = s.pstar()
        assert np.array_equal(got[obstacle], before[obstacle]), "an obstacle keeps pStar and lambda bit for bit"
        seen["pstar"] = got[:, :3].copy()
        return got[:, :3]

    first = _FIRST.setdefault((name, fp64, fast), {})
    out = CR.hold_iterations(stage_lambda, stage_delta, ps0, st["mass"], obstacle, cells, dtype, h, p.scale, list(p.min_bound),
                             list(p.max_bound), fast=fast, first=first)
    return out, seen["counts"], seen["lambda"]


def report(tag, out):
    for record in ("lambda", "move"):
        rows = [s for s in out if s["record"] == record]
        print(f"{tag} {record}: worst error / derived bar {max(s['derived'] for s in rows):.3f}, "
              f"largest error {max(s['err'] for s in rows):.3e}")
    amb = max(s["ambiguous"] for s in out)
    print(f"{tag}: ambiguous particles {amb}")
    return amb


def assert_lists(name, counts):
    """the case got where it claims to be"""
    if name == "pile":
        assert (counts == OVERFLOW).sum() >= 100, (counts == OVERFLOW).sum()
    if name == "cubes1024":                                      # spread out after its warm steps: nothing spills (at most 26 within h)
        assert (counts <= 40).all(), counts.max()
    if name == "cubes1024_start":                                # lists in the rows alone and lists that took a chunk
        spill, rows = ((counts > 40) & (counts <= 160)).sum(), (counts <= 40).sum()
        assert spill > 0 and rows > 0, (spill, rows)


def first_lambda_one_lane(pkg, name, fp64, fast):
    """lambda of the first iteration from the one-lane list-driven reader (coop = 0, split_build = 5)"""
    if (name, fp64, fast) not in _LAMBDA0:
        s, p = staged(pkg, name, fp64, fast, 0, 5)
        _LAMBDA0[name, fp64, fast] = s.stage("lambda", p).pstar()[:, 3].copy()
    return _LAMBDA0[name, fp64, fast]


@pytest.mark.parametrize("coop,split", READERS, ids=READER_IDS)
@pytest.mark.parametrize("fp64,fast", ARITHMETIC, ids=ARITHMETIC_IDS)
@pytest.mark.parametrize("name", list(CR.SCENES))
def test_lambda_and_move_within_the_bars_per_particle(pkg, name, fp64, fast, coop, split):
    t0 = time.perf_counter()
    tag = f"{name} {ARITHMETIC_IDS[ARITHMETIC.index((fp64, fast))]} coop={coop} split_build={split}"
    out, counts, lam = hold_case(pkg, name, fp64, fast, coop, split)
    amb = report(tag, out)
    n_fluid = len(counts) - int((start_state(pkg, name, fp64)["type"] == 1).sum())
    assert amb <= ER.AMBIGUOUS_CAP * n_fluid and amb == 0
    assert len(out) == 2 * CR.ITERATIONS and all(s["ratio"] < 1.0 for s in out), out
    assert_lists(name, counts)
    if coop and split == 5 and name.startswith("cubes1024"):     # the cooperative lambda kernel did run: another order
        assert not np.array_equal(lam, first_lambda_one_lane(pkg, name, fp64, fast))
    print(f"{tag}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("fast", [False, True], ids=["fp32", "fp32-fast"])
@pytest.mark.parametrize("name", ["pile", "cubes1024_start"])
def test_walking_particles_in_a_cooperative_group(pkg, name, fast):
    """nbr_chunks = 1: the chunk pool runs dry, so every list beyond the 40 row slots but one is marked NBR_OVERFLOW and lane 0
    of its group walks the cells alone while its group mates idle into the shuffle"""
    out, counts, _ = hold_case(pkg, name, False, fast, 4, 5, nbr_chunks=1)
    report(f"{name} {'fp32-fast' if fast else 'fp32'} coop=4 split_build=5 nbr_chunks=1", out)
    assert all(s["ratio"] < 1.0 for s in out), out
    assert ((counts > 40) & (counts <= 160)).sum() <= 1
    assert (counts == OVERFLOW).sum() >= (100 if name == "pile" else 1), (counts == OVERFLOW).sum()
    if name == "cubes1024_start":
        assert (counts <= 40).sum() > 0


# ------------------------------------------------------------------------------------------ b

def two_tier_scene():
    """`pile` inside `cubes1024`: lists within the 40 row slots, lists that spill into a chunk and lists beyond 160"""
    a, b = scene("cubes1024"), scene("pile")
    out = {k: np.concatenate([np.asarray(a[k], np.float64 if k not in ("id", "type") else a[k].dtype),
                              np.asarray(b[k], np.float64 if k not in ("id", "type") else b[k].dtype)]) for k in a}
    out["id"] = np.arange(len(out["id"]), dtype=np.uint64)
    return out


def state_bytes(s):
    out = {k: v.tobytes() for k, v in s.download().items()}
    out["pstar"] = s.pstar().tobytes()
    return out


PATHS = [dict(gather=0), dict(gather=3), dict(row_major=0), dict(split_build=0), dict(split_build=4), dict(split_build=5),
         dict(split_build=5, list_max=16), dict(split_build=5, list_max=24), dict(list_max=16), dict(list_max=24),
         dict(pipeline=0), dict(pipeline=1), dict(flags="NO_LDS"), dict(fuse_diffuse=1)]


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32-fast", "fp64-fast"])
@pytest.mark.parametrize("name", ["obstacles", "two_tier"])
def test_fast_paths_give_the_default_fast_paths_bytes(pkg, name, fp64):
    sc = start_state(pkg, name, fp64)
    p = pkg.default_params(CR.ITERATIONS, 1000.0)

    def run(path, how="step"):
        path = dict(path)
        flags = pkg.FLAG_NO_LDS if path.pop("flags", None) else 0
        s = solver(pkg, fp64, True, flags=flags, **path).upload(**sc)
        if how == "steps":
            s.steps(p, 3)
        else:
            for _ in range(3):
                s.step(p)
        return s

    if name == "two_tier":                                       # all three kinds of list are there, after the first build
        probe = solver(pkg, fp64, True, split=5).upload(**sc).stage("predict", p).stage("sort", p).stage("lambda", p)
        cnt = probe.nbr_counts()
        assert (cnt == OVERFLOW).sum() >= 100 and ((cnt > 40) & (cnt <= 160)).sum() > 0 and (cnt <= 40).sum() > 0
    want = state_bytes(run({}))
    precise = solver(pkg, fp64, False).upload(**sc)
    for _ in range(3):
        precise.step(p)
    assert state_bytes(precise)["pstar"] != want["pstar"], "FAST is another arithmetic"
    for path in PATHS:
        got = state_bytes(run(path))
        differ = [k for k in want if got[k] != want[k]]
        assert not differ, (path, differ)
    got = state_bytes(run({}, "steps"))
    assert not [k for k in want if got[k] != want[k]], "steps(p, 3) against three step(p)"
    s = run(dict(graph=1), "steps")
    got = state_bytes(s)
    assert not [k for k in want if got[k] != want[k]], "graph = 1 through steps()"
    assert s.graph_stats()[0] > 0, s.graph_stats()


# ------------------------------------------------------------------------------------------ c

@pytest.mark.parametrize("fp64,fast", ARITHMETIC, ids=ARITHMETIC_IDS)
def test_run_to_run(pkg, fp64, fast):
    for coop, split in READERS:
        if not coop and not fast:
            continue                                             # (PRECISE, one lane: test_hip_parity.py's determinism test)
        runs = []
        for _ in range(2):
            got = b""
            for name in ("cubes1024", "cubes1024_start"):
                s, p = staged(pkg, name, fp64, fast, coop, split)
                for _ in range(CR.ITERATIONS):
                    s.stage("lambda", p).stage("delta", p)
                got += s.pstar().tobytes()
            runs.append(got)
        assert runs[0] == runs[1], (coop, split)
