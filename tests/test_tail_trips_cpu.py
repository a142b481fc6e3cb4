"""The width schedule of the row build's test trips (pbf_kernels.hpp k_build_rows_op, narrowest_trip), restated in Python:
full trips, then a last trip cut to the longest lane's remainder in steps of a granule.  A schedule that leaves a gap
loses candidates; one that starts a trip at or beyond the longest lane's length spins or reads past the padding the full
trip was sized for; one that overshoots by a granule or more has not removed the padding it is there to remove."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = (ROOT / "pbf-sph_amd" / "csrc" / "pbf_kernels.hpp").read_text()


def widest_partial_trip(full, step):
    return 0 if step >= full else (full - 1) // step * step


def narrowest_trip(left, full, step):
    """left: what the wave's longest lane has left, in units (more(k) = left > k)"""
    tw = step
    while tw < full and left > tw:
        tw += step
    return min(tw, full)


def voted_loop(lmax, full, step, unit=1):
    """The build's test trips (unit = 2 slots per pair load; unit = 1: the helper by itself): every pass votes.
    Returns the (start, width) of every trip in slots."""
    partial, t, trips = widest_partial_trip(full, step), 0, []
    while t < lmax:                                            # __any(t < L)
        left = -(-(lmax - t) // unit)                          # more(k) = __any(t + unit * k < L)  <=>  left > k
        w = full if (partial == 0 or left > partial) else narrowest_trip(left, full, step)
        trips.append((t, unit * w))
        t += unit * w
    return trips


def test_source_matches_the_restatement():
    body = SRC[SRC.index("__device__ __forceinline__ void narrowest_trip("):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"if constexpr \(TW >= FULL\) \{\s*trip\(std::integral_constant<uint32_t, FULL>\{\}\);", body)
    assert re.search(r"if \(more\(TW\)\)\s*narrowest_trip<FULL, STEP, TW \+ STEP>\(more, trip\);\s*else\s*"
                     r"trip\(std::integral_constant<uint32_t, TW>\{\}\);", body)
    assert "return STEP >= FULL ? 0u : (FULL - 1u) / STEP * STEP; }" in SRC
    # the build's test trips: votes in pair loads, a trip advances by its own width
    assert "auto more = [&](uint32_t pairs) { return __any(t + 2 * pairs < L) != 0; };" in SRC
    assert "off += 16u * TW, b0 += 2 * TW, t += 2 * TW;" in SRC
    assert re.search(r"if \(PARTIAL == 0u \|\| more\(PARTIAL\)\)\s*trip\(std::integral_constant<uint32_t, uint32_t\(W\)>\{\}\);\s*"
                     r"else\s*narrowest_trip<uint32_t\(W\), TAIL>\(more, trip\);\s*"
                     r"\} while \(__any\(t < L\) && !__any\(cur >= lfull\)\);", SRC)


def check(trips, lmax, granule):
    end = 0
    for start, width in trips:
        assert start == end, "gap or overlap"
        assert start < lmax, "a trip that starts at or beyond the longest lane's length"
        assert width > 0
        end = start + width
    assert lmax <= end < lmax + granule, "the last trip overshoots by a granule or more"


# every granularity of every full width; the granularity equal to the full width is the fixed-width loop
@pytest.mark.parametrize("w", [2, 4])
def test_build_test_trips(w):
    for tail in range(1, w + 1):
        for full_trips in range(3):
            for rem in range(41):
                lmax = full_trips * 2 * w + rem                # slots; a trip of TW pair loads covers 2 TW of them
                trips = voted_loop(lmax, w, tail, unit=2)
                check(trips, lmax, 2 * tail)
                assert all(width in {2 * min(k * tail, w) for k in range(1, w + 1)} for _, width in trips)
                # only the last trip is narrower than the widest one the site can choose below the full width
                assert all(width == 2 * w for _, width in trips[:-1])


@pytest.mark.parametrize("full", [2, 4, 8])
def test_narrowest_trip_in_single_units(full):
    for tail in range(1, full + 1):
        for rem in range(41):
            trips = voted_loop(rem, full, tail)
            check(trips, rem, tail)
            assert all(width == full for _, width in trips[:-1])


def test_the_schedules_at_the_default_widths():
    """What the build executes for the run lengths of a settled sheet (a row run is ~21 slots)."""
    assert [w for _, w in voted_loop(21, 4, 1, unit=2)] == [8, 8, 6]
    assert [w for _, w in voted_loop(17, 4, 1, unit=2)] == [8, 8, 2]
    assert [w for _, w in voted_loop(17, 4, 2, unit=2)] == [8, 8, 4]
    assert [w for _, w in voted_loop(23, 4, 4, unit=2)] == [8, 8, 8]
    assert [w for _, w in voted_loop(6, 4, 2)] == [4, 2]
