"""pbf_selftest_divides: the trimmed divides swept on the device at the operands their later callers hand them —
k_mc_field's per-candidate denominator, surface tension's radial / r — and, for every category (the four of
pbf_selftest_math included), HOW MANY operands the sweep visited: a range filter that excluded everything would read
"no mismatch" too.  The fp32 categories are exhaustive in the divisor, and their ranges are monotone in the bit pattern,
so a bisection over bit patterns gives the exact count the device must report.

Test time, measured on an MI355X with `pytest --durations`: test_ranged_sqrt_and_divide_are_the_ieee_ones takes 0.39 s
at the parent commit when it is the first test of its process to launch a kernel (0.01 s when it is not) and its fp64
twin 0.10 s; the tests below take 0.07 s (fp32, not first; 0.14 s when first, with 8 numerators) and 0.20 s (fp64) with
NUMERATORS = 32 pseudo-random numerators per divisor.  8 and 32 numerators cost the same within 0.02 s of a whole
process's 0.4 s, so 32 it is; the fp64 sweep draws one numerator per divisor over the existing categories' 10240
rounds, which is what makes it twice its twin.
"""
import math

import numpy as np
import pytest

NUMERATORS = 32
NAMES = ["sqrt", "(h-r)^2/r", "x/poly6(0.3h)", "x/RHO", "field a/d", "field a/d, tiny a, guarded", "radial/r",
         "field a/d, tiny a, div_ranged alone"]
F = np.float32


def first_true(pred):
    """The smallest bit pattern b in [0, 0x7F800000] (+0 .. +inf, ascending in value) whose float satisfies the monotone
    predicate."""
    lo, hi = 0, 0x7F800000
    assert pred(np.uint32(hi).view(F)) and not pred(np.uint32(lo).view(F))
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        if pred(np.uint32(mid).view(F)):
            hi = mid
        else:
            lo = mid
    return hi


def count(ge, gt):
    """How many positive fp32 x satisfy ge(x) and not gt(x)."""
    return first_true(gt) - first_true(ge)


def expected_fp32(numerators, h_own=0.1):
    with np.errstate(all="ignore"):
        root = lambda x: np.sqrt(x, dtype=F)
        sqrt_n = count(lambda x: x >= F(2.0 ** -75), lambda x: x > F(3.0e38))
        hs = [F(h_own), F(0.05), F(0.2), F(0.0999999)]
        assert max(hs) <= F(0.2)
        pair_n = sum(count(lambda x: root(x) >= F(1e-8), lambda x: root(x) > hk) for hk in hs)
        mid_n = 2 + 2 * count(lambda x: x >= F(1e-30), lambda x: x > F(1e30))
        divisors = count(lambda d: d > F(1e-18), lambda d: d > F(64.0))
        roots = count(lambda x: root(x) >= F(1e-8), lambda x: root(x) > F(0.2))
    return [sqrt_n, pair_n, mid_n, 2 ** 32, divisors * (2 + numerators), divisors * (6 + numerators),
            roots * (1 + numerators), divisors * (6 + numerators)], divisors


def test_bisection_counts_a_range_it_can_enumerate():
    """first_true / count against brute force on one binade and a half."""
    lo, hi = F(0.75), F(2.0)
    bits = np.arange(F(0.5).view(np.uint32), F(4.0).view(np.uint32), dtype=np.uint32).view(F)
    assert count(lambda x: x >= lo, lambda x: x > hi) == int(((bits >= lo) & (bits <= hi)).sum()) == 2 ** 22 + 2 ** 23 + 1


@pytest.mark.gpu
def test_trimmed_divides_at_their_callers_operands_fp32(pkg):
    """Every fp32 divisor of the field's range x (25, 1, NUMERATORS hashed numerators), the same divisors x the tiny
    numerators in the call site's guarded form, every fp32 r of surface tension's range x (0, NUMERATORS hashed
    numerators): not one quotient differs from the compiler's IEEE divide, and each category visited exactly the
    number of operands computed here.  Category 7, div_ranged alone on the tiny numerators, must differ at least once
    per divisor (-0 / d comes out as +0): the sweep sees a wrong divide when there is one."""
    want, divisors = expected_fp32(NUMERATORS)
    s = pkg.Solver(h=0.1)
    try:
        bad, seen = s.selftest_divides(NUMERATORS)
    finally:
        s.close()
    for k, name in enumerate(NAMES):
        print(f"SWEEP f32 [{k}] {name}: {int(bad[k])} mismatches, visited {int(seen[k])}, host count {want[k]}")
    assert [int(v) for v in seen] == want
    assert bad[0] == 0 and bad[1] == 0 and bad[2] <= 1 and bad[3] == 0, bad
    assert bad[4] == 0 and bad[5] == 0 and bad[6] == 0, bad
    assert bad[7] >= divisors, bad


@pytest.mark.gpu
def test_trimmed_divides_at_their_callers_operands_fp64(pkg):
    """The fp64 forms over 10240 rounds x 2^20 threads pseudo-random operands per category.  Every category but [1]
    keeps every draw, so its visited count is rounds x threads exactly; [1] (k_selftest_math64's (h - r)^2 / r) drops
    the draws whose r falls below 1e-8: half of its draws are log-uniform in (2^-26.5 h, h), of which the share
    log2(h / 1e-8) / 26.5 stays, and the uniform half loses 1e-8 / h of its draws (h = one of four, equally often).
    The binomial spread of 1.07e10 draws is 3e-6 of them; the count must lie within 1e-4."""
    rounds, threads = 10240, 4096 * 256
    n = rounds * threads
    s = pkg.Solver(h=0.1, fp64=True)
    try:
        bad, seen = s.selftest_divides(NUMERATORS)
    finally:
        s.close()
    kept = 0.0
    for hk in (0.1, 0.05, 0.2, 0.0999999):
        log_kept = math.log2(hk / 1e-8) / 26.5
        kept += 0.25 * (0.5 * log_kept + 0.5 * (1.0 - 1e-8 / hk))
    for k, name in enumerate(NAMES):
        print(f"SWEEP f64 [{k}] {name}: {int(bad[k])} mismatches, visited {int(seen[k])} of {n} draws")
    print(f"SWEEP f64 [1] expected share kept {kept:.6f}, seen {int(seen[1]) / n:.6f}")
    assert all(int(seen[k]) == n for k in (0, 2, 3, 4, 5, 6, 7)), seen
    assert abs(int(seen[1]) - kept * n) <= 1e-4 * n, (seen[1], kept * n)
    assert not bad[:7].any(), bad
    assert bad[7] > 0, bad
