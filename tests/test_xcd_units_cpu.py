"""The workgroup -> unit -> (chunk, tid) map of the row iteration kernels at workgroup widths below a chunk (pbf_kernels.hpp
xcd_unit / iter_unit): restated in numpy.  A unit is WG lanes of a 256-lane chunk, the grid counts units.  Checked for 1, 2
and 4 units per chunk: the units are a bijection of [0, grid) with one ascending contiguous run per XCD (so the units of a
chunk and neighbouring chunks meet in one L2), the lanes of all units cover the particles [0, 256 chunks) exactly once — a
lane that two units claim would write one list twice, one that none claims would leave a particle without a list — and the
lanes at or beyond n, all in the last chunk, are the ones the kernels' `i >= c.n` drops."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = (ROOT / "pbf-sph_amd" / "csrc" / "pbf_kernels.hpp").read_text()
BLOCK = 256
GRIDS = list(range(1, 71)) + [255, 256, 257, 4001, 16000, 16001, 65535]


def xcd_unit(block, grid, xcds=8):
    k, q, r = block % xcds, grid // xcds, grid % xcds
    return k * q + np.minimum(k, r) + block // xcds


def iter_unit(block, thread, grid, per_chunk):
    """(chunk, tid) of lane `thread` of workgroup `block`"""
    wg = BLOCK // per_chunk
    u = xcd_unit(block, grid)
    return u // per_chunk, (u % per_chunk) * wg + thread


def test_source_matches_the_restatement():
    body = SRC[SRC.index("__device__ inline uint32_t xcd_unit()"):]
    body = body[:body.index("}\n") + 1]
    assert re.search(r"k = blockIdx\.x % NUM_XCD, q = g / NUM_XCD, r = g % NUM_XCD", body)
    assert re.search(r"return k \* q \+ min\(k, r\) \+ blockIdx\.x / NUM_XCD;", body)
    body = SRC[SRC.index("__device__ inline IterUnit iter_unit()"):]
    body = body[:body.index("}\n") + 1]
    assert "constexpr uint32_t PER_CHUNK = uint32_t(BLOCK) / WG;" in body
    assert "return IterUnit{u / PER_CHUNK, (u % PER_CHUNK) * WG + threadIdx.x};" in body
    assert "if constexpr (PER_CHUNK == 1) return IterUnit{xcd_chunk(), threadIdx.x};" in body  # one unit per chunk: the chunk map itself
    assert "static_assert(BLOCK == 256" in body
    # the kernels form the particle index from (chunk, tid) and drop the lanes past the end
    for kernel in ("k_build_rows_op", "k_gather_from_lists"):
        text = SRC[SRC.index(f"void {kernel}("):]
        text = text[:text.index("if (i >= c.n) return;")]
        assert "iter_unit<uint32_t(WG)>()" in text and "* BLOCK + " in text, kernel


@pytest.mark.parametrize("per_chunk", [1, 2, 4])
@pytest.mark.parametrize("grid", GRIDS)
def test_units_bijection_and_contiguous_runs(grid, per_chunk):
    b = np.arange(grid, dtype=np.int64)
    u = xcd_unit(b, grid)
    assert np.array_equal(np.sort(u), b)  # every unit exactly once
    for k in range(8):  # one contiguous, ascending run per XCD
        mine = u[b % 8 == k]
        if len(mine):
            assert np.array_equal(mine, np.arange(mine[0], mine[0] + len(mine)))


@pytest.mark.parametrize("per_chunk", [1, 2, 4])
@pytest.mark.parametrize("grid", GRIDS)
def test_lanes_cover_the_chunks_once(grid, per_chunk):
    if grid % per_chunk:
        grid += per_chunk - grid % per_chunk  # (the host launches whole chunks: chunks x units per chunk)
    chunks, wg = grid // per_chunk, BLOCK // per_chunk
    b = np.repeat(np.arange(grid, dtype=np.int64), wg)
    t = np.tile(np.arange(wg, dtype=np.int64), grid)
    chunk, tid = iter_unit(b, t, grid, per_chunk)
    assert tid.min() >= 0 and tid.max() < BLOCK and chunk.min() >= 0 and chunk.max() < chunks
    i = chunk * BLOCK + tid
    assert np.array_equal(np.sort(i), np.arange(BLOCK * chunks))  # every lane of every chunk exactly once
    # the units of a chunk sit on one XCD unless the chunk straddles the boundary between two XCDs' runs: at most 7 chunks do
    ub = np.arange(grid, dtype=np.int64)
    uchunk = xcd_unit(ub, grid) // per_chunk
    lo, hi = np.full(chunks, 8), np.full(chunks, -1)
    np.minimum.at(lo, uchunk, ub % 8)
    np.maximum.at(hi, uchunk, ub % 8)
    assert (lo != hi).sum() <= 7
    # a particle count that ends inside the last chunk: the lanes the kernels drop are exactly the indices from n on, and they all
    # belong to the last chunk
    for n in {BLOCK * (chunks - 1) + 1, BLOCK * chunks - 63, BLOCK * chunks - 1, BLOCK * chunks}:
        live = i < n
        assert live.sum() == n and np.array_equal(np.sort(i[live]), np.arange(n))
        assert np.all(chunk[~live] == chunks - 1)
