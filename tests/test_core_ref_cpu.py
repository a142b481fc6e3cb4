"""The bars of tests/core_ref.py, validated before a device sees them.

  * The fp32 and the fp64 ORACLE with device_pow=True — to which the PRECISE kernels are bit-equal (tests/test_hip_parity.py
    section A) — stay below the bar at every non-ambiguous particle, for lambda and for the delta-p move, on both solver
    iterations, on the eight scenes of tests/test_core_paths_gpu.py.  A worst error / bar above 1 means a count in core_ref's
    docstring is wrong.
  * core_ref.Coop, the cooperative order restated in N at K = 2, 4, 8, stays below the same bar: the running-sum part holds for
    any order.
  * Six mutations of the evaluation are at least 100 bars out at some particle of every scene they apply to: the bar bites.
"""
import numpy as np
import pytest

import core_ref as CR
import extras_ref as ER
import nversion as NV
import oracle_lib as O
from sample_ref import key_cells
from test_nversion_cpu import scene

LO, HI = [0.0, 0.0, 0.0], [1000.0, 1000.0, 1000.0]


def sorted_oracle(name, fp64):
    """the oracle after the scene's warm steps, predict and sort -> (oracle, params, pStar, mass, obstacle, cells)"""
    warm, force = CR.SCENES[name]
    q = O.make_params(iteration=CR.ITERATIONS, force=force)
    o = O.Oracle(fp64, device_pow=True)
    o.set_particles(**scene(CR.base(name)))
    for _ in range(warm):
        o.step(q)
    o.predict(q).sort(q).grid_table(q)
    st = o.get_particles()
    ps = o.pstar().astype(np.float64)
    assert o.keys().max() < len(o.table()), "every particle must lie inside the grid for the all-pairs equivalence"
    h = ER.kernel_inputs(o.dtype, q.h, q.dt)[0]
    cells = NV.predict_cells(ps, h, q.scale, LO)
    kc = key_cells(o.keys()).astype(np.int64)
    assert np.array_equal(cells - cells.min(0), kc - kc.min(0)), "the float64 cells are the cells the walk bins into"
    return o, q, ps, st["mass"].astype(np.float64), st["type"] == 1, cells


def stages(o, q):
    return (lambda: o.lambda_(q).lambdas()), (lambda: o.delta(q).pstar())


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", list(CR.SCENES))
def test_oracle_and_cooperative_order_stay_inside_the_bars(name, fp64):
    o, q, ps, mass, obstacle, cells = sorted_oracle(name, fp64)
    dtype = o.dtype
    h = ER.kernel_inputs(dtype, q.h, q.dt)[0]
    fluid = ~obstacle
    coop = {}

    def restated(it, P, lam, ps_it, ref_lambda, ref_move):
        E = CR.Coop(ps_it, mass, obstacle, q.h, P.cells, dtype)
        for K in (2, 4, 8):
            keep = fluid & ~ref_lambda[2]
            coop["lambda", it, K] = ER.worst(E.lambdas(K), ref_lambda[0], ref_lambda[1], keep)[0]
            new = E.delta(lam, q.scale, LO, HI, K).astype(np.float64)
            coop["move", it, K] = ER.worst(new - ps_it, ref_move[0], ref_move[1], keep)[0]
            assert np.array_equal(new[obstacle], ps_it[obstacle])

    seen = CR.hold_iterations(*stages(o, q), ps, mass, obstacle, cells, dtype, h, q.scale, LO, HI, each=restated)
    for record in ("lambda", "move"):
        walk = max(s["ratio"] for s in seen if s["record"] == record)
        tree = max(v for k, v in coop.items() if k[0] == record)
        print(f"{name} {dtype.__name__} {record}: worst error / bar — oracle {walk:.3f}, cooperative order {tree:.3f}; "
              f"largest error {max(s['err'] for s in seen if s['record'] == record):.3e}")
    amb = max(s["ambiguous"] for s in seen)
    print(f"{name} {dtype.__name__}: ambiguous particles {amb} of {int(fluid.sum())} (at most {ER.AMBIGUOUS_CAP:.0%} by condition)")
    assert amb <= ER.AMBIGUOUS_CAP * fluid.sum()
    assert amb == 0                                              # what is found on these scenes
    assert all(s["ratio"] < 1.0 for s in seen), seen
    assert all(v < 1.0 for v in coop.values()), coop
    assert len(seen) == 2 * CR.ITERATIONS and len(coop) == 6 * CR.ITERATIONS
    if len(ps) > 1:                                              # the bars bound something: the move is not trivially zero
        assert any(s["err"] > 0 for s in seen) or fp64


def test_a_result_that_is_not_finite_is_outside_every_bar():
    for bad in (np.nan, np.inf):
        o, q, ps, mass, obstacle, cells = sorted_oracle("edges65", False)
        h = ER.kernel_inputs(np.float32, q.h, q.dt)[0]
        lam_stage, delta_stage = stages(o, q)

        def broken():
            lam = lam_stage().copy()
            lam[7] = bad
            return lam
        with np.errstate(invalid="ignore"):
            seen = CR.hold_iterations(broken, delta_stage, ps, mass, obstacle, cells, np.float32, h, q.scale, LO, HI)
        assert not any(s["ratio"] <= 1.0 for s in seen if s["record"] == "lambda"), seen


def test_an_obstacle_that_moves_is_outside_every_bar():
    o, q, ps, mass, obstacle, cells = sorted_oracle("obstacles", False)
    h = ER.kernel_inputs(np.float32, q.h, q.dt)[0]
    lam_stage, delta_stage = stages(o, q)

    def nudged():
        new = delta_stage().copy()
        k = np.flatnonzero(obstacle)[3]
        new[k, 1] = np.nextafter(new[k, 1], np.float32(2.0))
        return new
    seen = CR.hold_iterations(lam_stage, nudged, ps, mass, obstacle, cells, np.float32, h, q.scale, LO, HI)
    # (the second iteration starts from the nudged pStar, which the oracle keeps: only the first move is out)
    assert seen[0]["ratio"] <= 1.0 and seen[1]["ratio"] == np.inf and seen[1]["derived"] <= 1.0, seen


# ---- mutations ---------------------------------------------------------------------------------------------------------------

def mutated_move(ps, lam, h, scale, obstacle, cells, mode):
    """nversion.delta with one thing wrong -> the move"""
    r, g = NV.pair_tables(ps, h, cells)
    p6dq = float(NV.poly6(np.array(NV.CorrDeltaQ * h), h))
    corr = 0.0 if mode == "no_corr" else -NV.CorrK * (NV.poly6(r, h) / p6dq) ** NV.CorrN
    factor = (lam[:, None] + (lam[:, None] if mode == "lambda_a" else lam[None, :]) + corr) / NV.RHO
    terms = g * factor[..., None]
    has = np.ones(len(ps), bool)
    if mode == "drop_nearest":
        rr = np.where((r >= NV.EPSILON) & (r <= h), r, np.inf)
        j = rr.argmin(1)
        rows = np.arange(len(ps))
        has = np.isfinite(rr[rows, j])
        terms[rows, j] = 0.0
    new = np.minimum(np.asarray(HI), np.maximum(np.asarray(LO), (ps + terms.sum(1)) * scale)) / scale
    return np.where(obstacle[:, None], 0.0, new - ps), has


MUTATIONS = {  # name -> the scenes it applies to
    "delta-p drops the nearest spiky neighbour": [s for s in CR.SCENES if s != "edges1"],
    "lambda_b read as lambda_a": [s for s in CR.SCENES if s != "edges1"],
    "corr omitted": [s for s in CR.SCENES if s != "edges1"],
    "an obstacle neighbour left out of rho": ["obstacles", "pile"],
    "the last butterfly stage skipped": [s for s in CR.SCENES if s != "edges1"],
    "a padding entry counted as valid": list(CR.SCENES),
}


@pytest.mark.parametrize("name", list(CR.SCENES))
def test_the_bars_notice_six_mutations(name):
    """fp32, the wider bar.  Each mutation must put at least one non-ambiguous particle 100 bars out (the bar
    tests/test_extras_ref_cpu.py asserts) in at least one of the two iterations; every figure is printed."""
    o, q, ps0, mass, obstacle, cells = sorted_oracle(name, False)
    h = ER.kernel_inputs(np.float32, q.h, q.dt)[0]
    fluid = ~obstacle
    out = {}

    def mutate(it, P, lam, ps, ref_lambda, ref_move):
        keep = fluid & ~ref_lambda[2]

        def far(record, got, ref, rows=None):
            k = keep if rows is None else keep & rows
            out[record, it] = ER.worst(got, ref[0], ref[1], k)[0]

        for record, mode in (("delta-p drops the nearest spiky neighbour", "drop_nearest"), ("lambda_b read as lambda_a", "lambda_a"),
                             ("corr omitted", "no_corr")):
            got, rows = mutated_move(ps, lam, h, q.scale, obstacle, P.cells, mode)
            far(record, got, ref_move, rows)
        r, _ = NV.pair_tables(ps, h, P.cells)
        rho = (mass[:, None] * np.where(obstacle[None, :], 0.0, NV.poly6(r, h))).sum(1)
        _, grad = NV.pair_tables(ps, h, P.cells)
        nv = (grad * NV.RHO_RECIP).sum(1)
        far("an obstacle neighbour left out of rho",
            np.where(obstacle, 0.0, -(rho / NV.RHO - 1.0) / ((nv * nv).sum(-1) + NV.CFM_EPSILON)), ref_lambda)
        E = CR.Coop(ps, mass, obstacle, q.h, P.cells, np.float32)
        for K in (2, 4, 8):
            new = E.delta(lam, q.scale, LO, HI, K, skip_last_stage=True).astype(np.float64)
            out["the last butterfly stage skipped", it, K, "move"] = ER.worst(new - ps, ref_move[0], ref_move[1], keep)[0]
            out["the last butterfly stage skipped", it, K, "lambda"] = ER.worst(E.lambdas(K, skip_last_stage=True), ref_lambda[0],
                                                                                ref_lambda[1], keep)[0]
            out["a padding entry counted as valid", it, K] = ER.worst(E.lambdas(K, padding_valid=True), ref_lambda[0],
                                                                      ref_lambda[1], keep)[0]

    CR.hold_iterations(*stages(o, q), ps0, mass, obstacle, cells, np.float32, h, q.scale, LO, HI, each=mutate)
    for key in sorted(out, key=str):
        applies = name in MUTATIONS[key[0]]
        print(f"{name} {key}: error / bar {out[key]:.3g}" + ("" if applies else "   (does not apply to this scene)"))
    # over the two iterations: on `pile` the first has every list at 320 entries — no short last trip at any K — and the second
    # has thrown the fluid out of the obstacles' reach, so each of those two mutations applies in one iteration only
    best = {}
    for key, ratio in out.items():
        rest = (key[0],) + tuple(key[2:])
        best[rest] = max(best.get(rest, 0.0), ratio)
    for key, ratio in best.items():
        if name in MUTATIONS[key[0]]:
            assert ratio > 100.0, (key, ratio)
