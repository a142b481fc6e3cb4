// pbf_collider_state.hpp — which solids are installed (the collider's lattice, the scenery's), which collider features are on,
// what the reaction records of the current step describe, and the events that move either.  The buffers, the mailboxes and the
// lattices' geometry (pbf_solid_lattice.hpp) stay in pbf_ctx; this is only what decides which kernels and which launch
// sequence a step runs, and what an observer may believe.  No HIP in here (plain C++17):
// host/test_collider_state.cpp walks it without a device.  pbf_hip.hip reads the fields and questions freely; it changes
// them through the events ONLY (tests/test_collider_state_cpu.py holds it to that).
//
// The rules, in one place:
//   posed, body, friction  =>  a lattice is installed        (a new lattice, clearing included, starts without them)
//   body      =>  reaction and posed                         (the body owns the pose; turned off, it leaves it behind)
//   friction  =>  reaction
//   lattice and scenery  =>  reaction                        (the pair's kernels write the records; the scenery alone is static)
//   the reaction may be on without a lattice, and stays on across a replaced or cleared solid
//   frictionRan  =>  friction
//   reaction off  =>  pushAt == 0 and pushRows == -1
//
// `gen` is part of a captured step's key (GraphKey::collider).  An event that changes which kernels or which launch sequence a
// step runs bumps it and returns true: the caller then destroys the captured graphs, none of which can be asked for again.
// (Should destroying them fail, the event stands: the key has moved on, so no stale graph is ever replayed.)  An event that
// only rewrites a record on the device — a pose update, a re-placed body, a rewritten friction record — returns false.
#pragma once

#include <cstdint>

namespace pbf {

struct ColliderState {
  bool lattice = false;      // pbf_set_collider / pbf_set_collider_mesh: a lattice is installed
  bool scenery = false;      // pbf_set_scenery / pbf_set_scenery_mesh: the static lattice beside it is installed
  bool posed = false;        // pbf_set_collider_pose (or a body, now or before): the kernels read the pose record
  bool reaction = false;     // pbf_set_collider_reaction: delta-p writes the records, the sort clears them
  bool body = false;         // pbf_set_collider_body: stage_body runs after the iterations
  bool friction = false;     // pbf_set_collider_friction: stage_friction runs after finalise
  bool frictionRan = false;  // a friction pass has run since friction was turned on
  uint64_t gen = 0;          // the generation of the launch sequence
  uint64_t pushAt = 0;       // the order epoch of the sort that cleared the records (0: no sort since enabling)
  int pushRows = -1;         // the delta-p launches since that sort indexed them by row slot (1) or Morton index (0); -1: none ran

  // ---- questions --------------------------------------------------------------------------------
  // which DeltaOp delta-p runs; the values are pbf_kernels.hpp's ColliderMode (pbf_hip.hip asserts it).  With the reaction on
  // and no pose set the kernels run the identity pose.  The scenery alone runs the static kernels on its own lattice.
  enum DeltaMode : int { DELTA_OFF = 0, DELTA_STATIC = 1, DELTA_POSED = 2, DELTA_REACT = 3, DELTA_REACT_SCENERY = 4 };
  DeltaMode delta_mode() const {
    if (!lattice) return scenery ? DELTA_STATIC : DELTA_OFF;
    return scenery ? DELTA_REACT_SCENERY : reaction ? DELTA_REACT : posed ? DELTA_POSED : DELTA_STATIC;
  }
  // the lattice the static kernels read is the scenery's, not the collider's
  bool static_reads_scenery() const { return scenery && !lattice; }
  // the step's records are indexed by row slot: their readers go through rowSlotOf
  bool records_by_row() const { return pushRows > 0; }
  // the records describe the arrays as they are: cleared by the sort of the current order, and that order still stands
  bool records_current(uint64_t orderEpoch, bool sorted) const { return pushAt == orderEpoch && sorted; }
  // the friction pass has left sums for its observer
  bool friction_sums_ready() const { return frictionRan; }
  // the REACT kernels read the pose record although no pose is set: it must hold the identity
  bool needs_identity_pose() const { return reaction && !posed; }
  // who needs the records and so forbids turning the reaction off (the body is named first, the pair of solids last)
  enum Holder { HELD_BY_NONE, HELD_BY_BODY, HELD_BY_FRICTION, HELD_BY_SCENERY };
  Holder why_reaction_must_stay() const {
    return body ? HELD_BY_BODY : friction ? HELD_BY_FRICTION : lattice && scenery ? HELD_BY_SCENERY : HELD_BY_NONE;
  }
  // Installing this solid (`present`; clearing never does) would complete the pair with the reaction off.  The entry point
  // then enables the reaction first — the record buffers must exist before the event, which is why the caller does it.
  enum Solid { COLLIDER, SCENERY };
  bool install_needs_reaction(Solid which, bool present) const { return present && !reaction && (which == COLLIDER ? scenery : lattice); }

  // ---- events: the entry points -------------------------------------------------------------------
  // A lattice was installed (`present`) or cleared.  Drops the pose, the body and friction with its pass; keeps the reaction
  // and what its records describe.  (Before there was this struct frictionRan outlived the lattice; nothing could read it
  // until friction_set() had reset it.)  Refused (nothing changes) where install_needs_reaction().
  bool installed(bool present) {
    if (install_needs_reaction(COLLIDER, present)) return false;
    lattice = present;
    posed = body = friction = frictionRan = false;
    return bump();
  }
  // The scenery was installed (`present`) or cleared: a replay never runs on a replaced or freed lattice, so gen always
  // moves.  The collider's pose, body, friction and records are left alone.  Refused where install_needs_reaction().
  bool scenery_installed(bool present) {
    if (install_needs_reaction(SCENERY, present)) return false;
    scenery = present;
    return bump();
  }
  // A pose was stored.  none -> posed selects other kernels; an update keeps everything.
  bool pose_set() {
    if (!lattice || posed) return false;
    posed = true;
    return bump();
  }
  // back to the static kernels.  Refused (nothing changes) while a body owns the pose.
  bool pose_cleared() {
    if (!posed || body) return false;
    posed = false;
    return bump();
  }
  // The record buffers exist.  Starts without records: the next sort brings them.  Keeps everything else.
  bool reaction_enabled() {
    if (reaction) return false;
    reaction = true;
    pushAt = 0, pushRows = -1;
    return bump();
  }
  // Drops the records.  Refused (nothing changes) while why_reaction_must_stay() names a reader.
  bool reaction_disabled() {
    if (!reaction || why_reaction_must_stay() != HELD_BY_NONE) return false;
    reaction = false;
    pushAt = 0, pushRows = -1;
    return bump();
  }
  // A body record was stored.  Needs a lattice and the reaction (else nothing changes).  off -> on adds stage_body to the
  // step and takes the pose over; a re-placed body keeps everything.
  bool body_set() {
    if (!lattice || !reaction || body) return false;
    body = posed = true;
    return bump();
  }
  // The solid stays where it is: the pose stays set, the reaction stays on.
  bool body_cleared() {
    if (!body) return false;
    body = false;
    return bump();
  }
  // A friction record was stored.  Needs a lattice and the reaction (else nothing changes).  off -> on adds stage_friction to
  // the step and forgets any earlier pass; a rewritten record keeps everything, the pass that ran included.
  bool friction_set() {
    if (!lattice || !reaction || friction) return false;
    friction = true, frictionRan = false;
    return bump();
  }
  // Drops the pass; the reaction stays on.
  bool friction_cleared() {
    if (!friction) return false;
    friction = frictionRan = false;
    return bump();
  }

  // ---- events: the step (none of them changes the launch sequence) ----------------------------------
  // the sort has cleared the records for the order it established
  void records_cleared(uint64_t orderEpoch) {
    if (reaction) pushAt = orderEpoch, pushRows = -1;
  }
  // A delta-p launch is about to index the records by row slot (`rows`) or Morton index.  false, and nothing changes, when an
  // earlier launch of this step used the other index: a step's records have one kind of index.
  bool delta_indexed(bool rows) {
    if (pushRows >= 0 && pushRows != int(rows)) return false;
    pushRows = int(rows);
    return true;
  }
  void friction_passed() { frictionRan = friction; }
  // A captured step was replayed (or a failed capture rolled back, to be re-run): its sort cleared the records, its delta-p
  // launches indexed them by Morton index — row_mode() is off while graphs are on, so a captured step has no row-major
  // launch — and its friction pass ran.
  void step_replayed(uint64_t orderEpoch) {
    if (reaction) pushAt = orderEpoch, pushRows = 0;
    friction_passed();
  }

 private:
  bool bump() { return ++gen, true; }
};

}  // namespace pbf
