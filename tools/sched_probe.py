"""(GPU box) how unevenly the 64 lanes of a wave are loaded in the list build / the list-driven delta-p on the settled
dam-break, what a per-workgroup schedule (lanes take the particles of their 256 / 1024-block in order of list
length) would recover, and what the rounding of the longest lane's length to a whole trip costs at every last-trip
granularity (csrc/pbf_kernels.hpp narrowest_trip).  Row-slot order (the default working set).
  python tools/sched_probe.py [nominal=1048576] [frames=205]
row_run_lengths() and cost() need numpy only (tests/test_tail_trips_gpu.py uses them on a read-back)."""
import importlib.util, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BUILD_W, READER_W, DRAIN_W = 4, 8, 4            # full trips: pair loads (2 slots each), list entries, survivors
ROW_SLOTS = 40                                   # NBR_ROWS: the reader's head loop covers min(count, 40)


def compact(k):  # every third bit
    k = k & 0x09249249
    k = (k | k >> 2) & 0x030C30C3; k = (k | k >> 4) & 0x0300F00F; k = (k | k >> 8) & 0x030000FF; k = (k | k >> 16) & 0x3FF
    return k


def row_run_lengths(keys):
    """keys: the sorted Morton keys.  -> (order, L): order[j] = the Morton index of row slot j, L[j, r] = the length of the
    (dy, dz) row run r (three x cells) that row slot j walks."""
    keys = np.asarray(keys).astype(np.int64)
    x, y, z = compact(keys), compact(keys >> 1), compact(keys >> 2)
    P = 1 << int(np.ceil(np.log2(max(x.max(), y.max(), z.max()) + 2)))
    lin = (z * P + y) * P + x
    order = np.argsort(lin, kind="stable"); lin = lin[order]; x, y, z = x[order], y[order], z[order]
    occ = np.bincount(lin, minlength=P ** 3 + 2 * P * P).astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(occ)])
    L = np.zeros((len(keys), 9), np.int64)
    for r in range(9):
        yy, zz = y + r % 3 - 1, z + r // 3 - 1
        ok = (yy >= 0) & (yy < P) & (zz >= 0) & (zz < P)
        base = (np.clip(zz, 0, P - 1) * P + np.clip(yy, 0, P - 1)) * P
        L[:, r] = np.where(ok, cs[base + np.minimum(x + 2, P)] - cs[base + np.maximum(x - 1, 0)], 0)
    return order, L


def wave_maxima(cnt, L):
    """The longest lane's run length per (wave, row) and list length per wave; the last wave may be partial."""
    n = len(cnt); nw = (n + 63) // 64; pad = nw * 64 - n
    l = np.concatenate([L, np.zeros((pad, 9), np.int64)]).reshape(nw, 64, 9).max(1)
    c = np.concatenate([cnt, np.zeros(pad, np.int64)]).reshape(nw, 64).max(1)
    return l, c


def voted_slots(lmax, full, step):
    """Executed slots of a loop whose every pass votes (the build's test trips in pair loads, its drain): full trips, then
    the narrowest of step, 2 step, .. (< full), full that covers what is left."""
    lmax = np.asarray(lmax, np.int64)
    if step >= full:
        return (lmax + full - 1) // full * full
    partial = (full - 1) // step * step
    whole = np.maximum(lmax - partial + full - 1, 0) // full        # passes that find more than `partial` left
    left = lmax - whole * full                                      # (<= partial; may be <= 0: the loop is over)
    return whole * full + np.where(left > 0, (left + step - 1) // step * step, 0)


def reader_slots(head, full, step):
    """The reader's head loop: the full-width loop while a whole trip is left, then one last trip."""
    head = np.asarray(head, np.int64)
    if step >= full:
        return (head + full - 1) // full * full
    whole = head // full
    return whole * full + np.minimum((head - whole * full + step - 1) // step * step, full)


def cost(cnt, L, perm_block=None):
    """perm_block: None (identity) or the block size inside which lanes take particles sorted by list length"""
    n = len(cnt)
    idx = np.arange(n)
    if perm_block:
        nb = n // perm_block * perm_block
        blk = cnt[:nb].reshape(-1, perm_block)
        o = np.argsort(blk, axis=1, kind="stable") + (np.arange(nb // perm_block) * perm_block)[:, None]
        idx = np.concatenate([o.ravel(), np.arange(nb, n)])
    nw = n // 64
    c = cnt[idx][: nw * 64].reshape(nw, 64); l = L[idx][: nw * 64].reshape(nw, 64, 9)
    lmax, cmax = l.max(1), c.max(1)
    trips = ((lmax + 7) // 8).sum(1)            # test trips of 8 candidates: per row, the longest lane's
    flush = (cmax + 3) // 4 * 4                 # drained slots per lane: the longest lane's
    out = {"test_slots_per_lane": float(trips.mean() * 8), "candidates_per_lane": float(l.sum(2).mean()),
           "drain_slots_per_lane": float(flush.mean()), "hits_per_lane": float(c.mean()),
           "test_efficiency": float(l.sum(2).mean() / (trips.mean() * 8)), "drain_efficiency": float(c.mean() / flush.mean())}
    # the same walk with the last trip cut to the longest lane's remainder, per granularity (the full width = the fixed loop)
    pairs = (lmax + 1) // 2
    out["test_slots_per_lane_by_last_trip"] = {f"{2 * g}_slots": float(2 * voted_slots(pairs, BUILD_W, g).sum(1).mean())
                                                for g in (4, 2, 1)}
    out["test_slots_per_lane_by_last_trip"]["sum_of_wave_maxima"] = float(lmax.sum(1).mean())
    head = np.minimum(cmax, ROW_SLOTS)          # (lists beyond the rows: the chunk's loop is not the head loop's)
    out["reader_slot_steps_per_lane_by_last_trip"] = {f"{g}_entries": float(reader_slots(head, READER_W, g).mean()) for g in (8, 4, 2)}
    out["reader_slot_steps_per_lane_by_last_trip"]["mean_of_wave_maxima"] = float(head.mean())
    out["reader_active_lanes"] = float(np.minimum(c, ROW_SLOTS).mean() / reader_slots(head, READER_W, 8).mean())
    # (one drain of the whole list: a lane of more than LMAX = 32 survivors drains in two batches, each rounded)
    out["drain_slots_per_lane_by_last_trip"] = {f"{g}_survivors": float(voted_slots(cmax, DRAIN_W, g).mean()) for g in (4, 2, 1)}
    return out


def main():
    spec = importlib.util.spec_from_file_location("pbf_sph_amd", os.path.join(ROOT, "pbf-sph_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(ROOT, "pbf-sph_amd")])
    pkg = importlib.util.module_from_spec(spec); sys.modules["pbf_sph_amd"] = pkg; spec.loader.exec_module(pkg)
    nominal = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 205
    sc, side = pkg.scene_dambreak(nominal, False)
    s = pkg.Solver(h=0.1); s.upload(**sc); p = pkg.default_params(4, side)
    s.steps(p, frames)
    cnt = s.nbr_counts().astype(np.int64); cnt = np.where(cnt == 0xFFFFFFFF, 65, cnt)   # row-slot order
    _, L = row_run_lengths(s.keys())                                                        # Morton order in
    out = {"n": len(cnt), "frame": frames, "identity": cost(cnt, L), "sorted_in_256": cost(cnt, L, 256),
           "sorted_in_1024": cost(cnt, L, 1024), "sorted_in_4096": cost(cnt, L, 4096)}
    out["note"] = "sorted_* use this iteration's own lengths (an upper bound on what a schedule from the previous iteration gives)"
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
