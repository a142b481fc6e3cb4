"""k_mc_mark_near + k_mc_field against the oracle BIT FOR BIT, and the two full pipelines' meshes with them.

With influence 0.5 the device takes sqrt(len) where the reference takes pow(len, 0.5); the oracle's second documented
substitution (oracle_lib.Oracle(device_sqrt=True)) does the same, and everything else in Oracle::mc_field is the
device's arithmetic in the device's order.  So nothing is left for a tolerance to absorb: a wrong candidate order, a
tail slot folded twice, a divide that is an ulp off or a contraction the compiler was not to make all change a bit.
tests/test_mc_field_gpu.py bounds the same field independently (by rounding counts); the pow branch (influence 0.75,
1.0) stays tolerance-held there and in tests/test_mc.py: a libm pow has no bit contract.

Scenes: every scene of tests/mc_scenes.py (clamp folds and nodes outside the grid, obstacles, a particle on a node —
the wave-wide fall-back to the compiler's divide and the strict threshold —, blob, cloud) x its influence-0.5 sets
(resolutions 2 and 3) x fp32 / fp64, and one particle alone (lattice blocks of 4 x 4 x 4 lanes that are mostly empty).
`faces` at resolution 2 has a lattice of 21 x 19 x 17 nodes: no axis is a multiple of the 4-node lane block (at
resolution 3 it is 31 x 28 x 25).

HITS / INFINITE were derived on the CPU from the oracle alone (the counts are the same in fp32 and fp64): nodes with at
least one hit (v > 0), floors a little under the counts found (6765, 21655 / 4417, 15051 / 1170, 3957 / 4498, 15424 /
3982, 13649 / one particle: 114, 34), and nodes whose v is infinite — a particle ON the node, the fall-back's case:
on_node's one, at either resolution (at 3 the node rounds onto the particle), none anywhere else.
"""
import numpy as np
import pytest

import mc_closed_forms as CF
import mc_scenes as M
import oracle_lib as O
import test_mc_nversion_cpu as T
from test_hip_parity import assert_state_equal
from test_mc import bits_equal

pytestmark = pytest.mark.gpu

ONE_SETS = [CF.ONE_MC, (2.0, 3.125, 25.0, 0.5)]
HITS = {("faces", 2.0): 6000, ("faces", 3.0): 20000, ("obstacles", 2.0): 4000, ("obstacles", 3.0): 14000,
        ("on_node", 2.0): 1000, ("on_node", 3.0): 3500, ("blob", 2.0): 4000, ("blob", 3.0): 14000,
        ("cloud", 2.0): 3500, ("cloud", 3.0): 12000, ("one", 3.0): 100, ("one", 2.0): 30}
INFINITE = {("on_node", 2.0): 1, ("on_node", 3.0): 1}


def sets_of(name):
    sets = ONE_SETS if name == "one" else [mc for mc in M.PARAMS[name] if mc[3] == 0.5]
    assert sorted(mc[0] for mc in sets) == [2.0, 3.0]
    return sets


def oracle_of(name, fp64):
    if name == "one":
        return T.oracle_state(None, fp64, scene=dict(CF.ONE, sc=CF._particle(CF.ONE_POS)))
    return T.oracle_state(name, fp64)


CASES = [(n, fp64) for n in M.NAMES + ("one",) for fp64 in (False, True)]


@pytest.mark.parametrize("name,fp64", CASES, ids=[f"{n}-{'f64' if d else 'f32'}" for n, d in CASES])
def test_device_field_and_mesh_equal_the_oracles_bit_for_bit(pkg, name, fp64):
    s, o, q, st, _ = oracle_of(name, fp64)
    sol = pkg.Solver(h=s["h"], fp64=fp64)
    try:
        sol.upload(**M.cast(s["sc"], sol.dtype))
        p = M.device_params(pkg, s)
        for _ in range(s["frames"]):
            sol.step(p)
        assert_state_equal(sol.download(), st, name)
        for mc in sets_of(name):
            g = sol.surface(p, pkg.McParams(*mc))
            o.set_device_sqrt(True)
            try:
                w = o.surface(q, O.OracleMc(*mc))
            finally:
                o.set_device_sqrt(False)
            what = f"{name} {mc} {'f64' if fp64 else 'f32'}"
            assert np.array_equal(g["sample"], w["sample"]), what
            if name == "faces" and mc[0] == 2.0:
                assert all(int(v) % 4 != 0 for v in w["sample"]), w["sample"]
            # not vacuous: counted on the ORACLE's field
            v = w["pn"][:, 0]
            hits, infinite = int((v > 0).sum()), int(np.isinf(v).sum())
            print(f"BITS {what}: sample {[int(x) for x in w['sample']]}, {hits} nodes with hits, {infinite} infinite, "
                  f"{len(w['vs']) // 3} triangles")
            assert hits >= HITS[(name, mc[0])], (what, hits)
            assert name == "one" or hits >= 300
            assert infinite == INFINITE.get((name, mc[0]), 0), (what, infinite)
            bits_equal(g["pn"], w["pn"], what + " pn")
            bits_equal(g["c"], w["c"], what + " c")
            assert len(g["vs"]) == len(w["vs"]) and len(w["vs"]) % 3 == 0 and len(w["vs"]) >= 3 * 50, (what, len(g["vs"]), len(w["vs"]))
            for k in ("vs", "ns", "cs"):
                assert np.array_equal(g[k], w[k], equal_nan=True), (what, k)
    finally:
        sol.close()
