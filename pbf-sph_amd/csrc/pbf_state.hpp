// pbf_state.hpp — which buffer currently holds the truth: the context's derived validity flags and buffer-role indices,
// and the events that move them.  No HIP in here (plain C++17): host/test_state.cpp walks the state machine without a
// device.  pbf_hip.hip reads the fields and predicates freely; it changes them through the events ONLY
// (tests/test_ctx_state_cpu.py holds it to that).
#pragma once

#include <cstdint>

namespace pbf {

struct DerivedState {
  int cur = 0;                 // which of the two particle-array sets is live
  int pcur = 0;                // which pstar buffer is live
  int rcur = 0;                // which rowPstar buffer is live
  uint32_t countedTableN = 0;  // the table size `count` was built for (predict and sort must agree on the grid)
  bool sorted = false;         // keys/table valid for the current arrays
  bool counted = false;        // cell histogram of the current keys is in `count` (set by predict, consumed by sort)
  bool bricksValid = false;    // ctx->bricks lists the non-empty bricks of the current table
  bool rowColValid = false;    // rowCol holds the colours of col4[cur] (set by the sort, consumed by the diffusion)
  bool rowsValid = false;      // the row arrays describe this step's sorted set (built by the sort)
  bool rowsCurrent = false;    // rowPstar[rcur] holds the current {pStar, lambda} (false once a Morton-path stage has moved on)
  bool pstarInRows = false;    // the current {pStar, lambda} live in rowPstar[rcur] ONLY: pstar[pcur] is stale (materialise_pstar)
  bool nbrValid = false;       // the lists describe pstar[pcur] as it is now
  bool nbrRows = false;        // the current neighbour lists hold ROW slots (built by k_build_rows_op); implies nbrValid
  bool qposValid = false;      // qpos is the quantised copy of pstar[pcur] (written by the sort, delta-p and the slab refresh)
  bool omegaValid = false;     // pstar[2] holds the vorticity of the last extras pass (PBF_BUF_OMEGA), same order as the arrays
  bool surfaceValid = false;   // surfB holds the record of the last surface-tension pass; invalidated with omegaValid
  bool prePredicted = false;   // pbf_steps: the next step's predict has already been done (k_finalise_predict)

  // ---- questions the stages ask ---------------------------------------------------------------
  bool rows_usable() const { return rowsValid && rowsCurrent; }                    // lambda may run on the row-major copy
  bool delta_on_rows() const { return nbrValid && nbrRows && rows_usable(); }      // list-driven delta-p on the row-major copy
  bool delta_from_lists() const { return nbrValid && !nbrRows; }                   // list-driven delta-p in Morton order
  bool diffuse_on_rows() const { return rowColValid && rowsValid; }                // k_diffuse_rows has its inputs
  bool pstar_in_live_rows() const { return pstarInRows && rowsCurrent; }           // the slab refresh reads / writes rowPstar[rcur]

  // ---- events ---------------------------------------------------------------------------------
  // A new particle set in array set `set` (uploads, sources / drains): nothing derived survives.  The histogram has been
  // dropped before (drop_histogram: `count` must be zeroed on the device as well).
  void arrays_replaced(int set) {
    *this = DerivedState{};
    cur = pcur = set;
  }
  // pStar of the current arrays has just been written into pstar[cur] and their keys counted (k_predict, or, `ahead` of the
  // next step, k_finalise_predict): everything the last sort built is stale.
  void predicted(uint32_t tableN, bool ahead) {
    pcur = cur;
    drop_lists();
    sorted = bricksValid = rowColValid = rowsValid = rowsCurrent = pstarInRows = qposValid = false;
    omegaValid = surfaceValid = false;
    histogram_current(tableN);
    prePredicted = ahead;
  }
  // a step asks whether its predict was done ahead, and thereby uses it up (also: a failed pbf_steps forgets it)
  bool take_prediction() {
    const bool was = prePredicted;
    prePredicted = false;
    return was;
  }
  void histogram_dropped() { counted = false; }
  // `count` describes the current keys (predict; the slab assembly after it has appended migrants and copies)
  void histogram_current(uint32_t tableN) {
    counted = true, countedTableN = tableN;
    sorted = false;
  }
  // The sort has scattered the arrays into the other set and consumed the histogram.  {pStar, lambda}: pstar[pcur] with its
  // quantised copy, or — `rows` — rowPstar[0] ONLY (with `rowDiffuse` also the colours); the brick list is not built yet.
  void sorted_now(bool rows, bool rowDiffuse) {
    cur = 1 - cur, pcur = cur, rcur = 0;
    sorted = true, counted = false;
    drop_lists();
    rowsValid = rowsCurrent = pstarInRows = rows;
    rowColValid = rowDiffuse;
    qposValid = !rows;
    bricksValid = false;
  }
  void bricks_listed() { bricksValid = true; }
  void quantised() { qposValid = true; }  // k_quantise: qpos follows pstar[pcur] again
  // The colours moved on (col4 swapped): the row-order copy is the pre-diffusion state.  `parked`: the per-cell sums went
  // through pStar's idle Jacobi partner and the list lengths.
  void diffused(bool parked) {
    rowColValid = false;
    omegaValid = surfaceValid = false;
    if (parked) drop_lists();
  }
  // lambda is in: pstar[pcur] (materialised before), or — `rows` — rowPstar[rcur] ONLY; `lists`: the launch left its
  // survivors behind for delta-p
  void lambda_done(bool lists, bool rows) {
    nbrValid = lists, nbrRows = lists && rows;
    if (rows) pstarInRows = true;
    else rowsCurrent = false;
  }
  // delta-p wrote the new pStar into rowPstar[newIndex] (`rows`; the Morton-order quantised copy is stale now) or
  // pstar[newIndex] (its epilogue keeps a valid qpos current): the lists are stale, and the buffer the last vorticity pass
  // left its result in may be the one written
  void pstar_moved(bool rows, int newIndex) {
    drop_lists();
    omegaValid = surfaceValid = false;
    if (rows) rcur = newIndex, pstarInRows = true, qposValid = false;
    else pcur = newIndex, rowsCurrent = false;
  }
  void materialised() { pstarInRows = false; }  // k_rows_to_morton: pstar[pcur] is current too
  // positions and velocities are final; the caller has swapped the live pStar buffer into pstar[cur], so that a later sort
  // scatters pstar[cur] -> pstar[1 - cur]
  void finalised() {
    pcur = cur;
    drop_lists();
  }
  void extras_done(bool omega, bool surface) {
    if (omega) omegaValid = true;
    if (surface) surfaceValid = true;
  }
  // The survivors of a select (slab migration, dropping the ghost copies, drains) were compacted into the other array set
  // (`flipped`), or the keys' frame changed (pbf_slab_configure): the table no longer describes the arrays.  Nothing else
  // is touched: what may be read back after a slab step depends on it.
  void compacted(bool flipped) {
    if (flipped) cur = 1 - cur, pcur = cur;
    sorted = false;
  }

  // What of this state identifies a step for hipGraph replay (GraphKey): the roles and the flags a step's launch sequence
  // depends on, written into `k` — zeroed by the caller, who compares bytes.  The rest is restored after a replay, not
  // compared.
  void step_key(DerivedState &k) const {
    k.cur = cur, k.pcur = pcur, k.countedTableN = countedTableN;
    k.sorted = sorted, k.counted = counted, k.nbrValid = nbrValid, k.qposValid = qposValid;
  }

 private:
  void drop_lists() { nbrValid = nbrRows = false; }
};

}  // namespace pbf
