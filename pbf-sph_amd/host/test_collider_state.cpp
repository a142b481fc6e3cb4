// test_collider_state.cpp — walks pbf::ColliderState (csrc/pbf_collider_state.hpp) through the call sequences the collider's
// entry points and the step perform in pbf_hip.hip and checks, after every event, the rules the header states.  No device, no
// library: the header alone.  Exit status 1 if a check failed; each failure prints the sequence, the trail and the last event.
#include "pbf_collider_state.hpp"

#include <cstdio>
#include <set>
#include <string>

using pbf::ColliderState;

namespace {

int g_failures = 0;
std::set<int> g_seen;  // the flag combinations the walks have stood in

int flags_of(const ColliderState &c) { return c.lattice | c.posed << 1 | c.reaction << 2 | c.body << 3 | c.friction << 4 | c.scenery << 5; }
bool allowed(int f) {  // the header's rules on the six flags
  const bool lattice = f & 1, posed = f & 2, reaction = f & 4, body = f & 8, friction = f & 16, scenery = f & 32;
  return (!body || (reaction && posed && lattice)) && (!friction || (reaction && lattice)) && (!posed || lattice) &&
         (!(lattice && scenery) || reaction);
}
// the table delta_impl (pbf_hip.hip) instantiates from, written out.  Without scenery: no lattice -> OFF; else the reaction
// wins over a pose.  With it: alone it is STATIC, beside a lattice REACT_SCENERY whatever else is on.
ColliderState::DeltaMode mode_of(int f) {
  static const ColliderState::DeltaMode table[16] = {
      ColliderState::DELTA_OFF,           ColliderState::DELTA_OFF,           ColliderState::DELTA_OFF,           ColliderState::DELTA_OFF,
      ColliderState::DELTA_STATIC,        ColliderState::DELTA_POSED,         ColliderState::DELTA_REACT,         ColliderState::DELTA_REACT,
      ColliderState::DELTA_STATIC,        ColliderState::DELTA_STATIC,        ColliderState::DELTA_STATIC,        ColliderState::DELTA_STATIC,
      ColliderState::DELTA_REACT_SCENERY, ColliderState::DELTA_REACT_SCENERY, ColliderState::DELTA_REACT_SCENERY, ColliderState::DELTA_REACT_SCENERY};
  return table[((f >> 5) & 1) << 3 | (f & 1) << 2 | ((f >> 2) & 1) << 1 | ((f >> 1) & 1)];  // (scenery, lattice, reaction, posed)
}

struct Walk {
  ColliderState col;
  uint64_t orderEpoch = 1;  // pbf_ctx::orderEpoch
  bool sorted = false;      // DerivedState::sorted
  std::string name, trail;

  void expect(bool ok, const char *event, const char *what) {
    if (ok) return;
    std::printf("FAIL [%s] after %s: %s\n  events: %s\n", name.c_str(), event, what, trail.c_str());
    ++g_failures;
  }
  // after EVERY event.  `before`: the state it found; `said`: what it returned (an event of the step says nothing: false);
  // `install`: it was installed() or scenery_installed(), which move gen whatever the flags do
  void check(const char *event, const ColliderState &before, bool said, bool install = false) {
    trail += trail.empty() ? event : std::string(" > ") + event;
    const int f = flags_of(col);
    g_seen.insert(f);
    expect(!col.body || (col.reaction && col.posed && col.lattice), event, "body without reaction, pose and lattice");
    expect(!col.friction || (col.reaction && col.lattice), event, "friction without reaction and lattice");
    expect(!col.posed || col.lattice, event, "posed without a lattice");
    expect(!(col.lattice && col.scenery) || col.reaction, event, "a collider beside scenery without the reaction");
    expect(col.static_reads_scenery() == (col.scenery && !col.lattice), event, "static_reads_scenery");
    expect(!col.frictionRan || col.friction, event, "frictionRan without friction");
    expect(col.reaction || (col.pushAt == 0 && col.pushRows == -1), event, "records described with the reaction off");
    expect(col.pushRows >= -1 && col.pushRows <= 1, event, "pushRows out of range");
    expect(col.delta_mode() == mode_of(f), event, "delta_mode() is not delta_impl's table");
    expect(col.friction_sums_ready() == col.frictionRan && col.records_by_row() == (col.pushRows > 0), event, "a question and its field disagree");
    expect(col.needs_identity_pose() == (col.reaction && !col.posed), event, "needs_identity_pose");
    const bool moved = install || flags_of(before) != f;  // install, none <-> posed, reaction / body / friction on <-> off
    expect(col.gen == before.gen + (moved ? 1 : 0), event, moved ? "gen did not move by one with the launch sequence" : "gen moved although the launch sequence did not");
    expect(said == moved, event, "the event's answer is not whether gen moved");
  }
  bool same_records(const ColliderState &b) const { return col.pushAt == b.pushAt && col.pushRows == b.pushRows; }
  bool records_current() const { return col.records_current(orderEpoch, sorted); }

  // ---- the entry points, as pbf_hip.hip calls the events; false = the call is refused ---------------------------------------
  // solid_install's first act: the call that completes the pair turns the reaction on (the event alone refuses, and drops nothing)
  void pair_first(ColliderState::Solid which, bool present) {
    const bool completes = present && !col.reaction && (which == ColliderState::COLLIDER ? col.scenery : col.lattice);
    expect(col.install_needs_reaction(which, present) == completes, "install_needs_reaction", "not the pair rule");
    if (!completes) return;
    const ColliderState b = col;
    const bool said = which == ColliderState::COLLIDER ? col.installed(true) : col.scenery_installed(true);
    check("install(refused)", b, said);
    expect(same_records(b) && col.frictionRan == b.frictionRan, "install(refused)", "a refused install changed something");
    set_reaction(true);
  }
  void set_collider(bool present) {  // solid_install(.., COLLIDER, ..)
    pair_first(ColliderState::COLLIDER, present);
    const ColliderState b = col;
    const bool said = col.installed(present);
    check(present ? "installed(true)" : "installed(false)", b, said, true);
    expect(col.lattice == present && !col.posed && !col.body && !col.friction && !col.frictionRan, "installed", "a feature of the old solid survived");
    expect(col.reaction == b.reaction && same_records(b) && col.scenery == b.scenery, "installed", "the reaction, its records or the scenery changed");
  }
  void set_scenery(bool present) {  // solid_install(.., SCENERY, ..)
    pair_first(ColliderState::SCENERY, present);
    const ColliderState b = col;
    const bool said = col.scenery_installed(present);
    check(present ? "scenery_installed(true)" : "scenery_installed(false)", b, said, true);
    expect(col.scenery == present && (flags_of(col) & 31) == (flags_of(b) & 31) && col.frictionRan == b.frictionRan && same_records(b),
           "scenery_installed", "the scenery's install touched the collider");
  }
  bool set_pose(bool pose) {  // pbf_set_collider_pose
    if (!col.lattice || col.body) return false;
    const ColliderState b = col;
    const bool said = pose ? col.pose_set() : col.pose_cleared();
    check(pose ? "pose_set" : "pose_cleared", b, said);
    expect(col.posed == pose && same_records(b) && col.frictionRan == b.frictionRan, pose ? "pose_set" : "pose_cleared", "wrong flags");
    return true;
  }
  bool set_reaction(bool on) {  // pbf_set_collider_reaction
    if (on == col.reaction) return true;
    const ColliderState b = col;
    if (!on && col.why_reaction_must_stay() != ColliderState::HELD_BY_NONE) {
      expect(col.why_reaction_must_stay() == (col.body ? ColliderState::HELD_BY_BODY : col.friction ? ColliderState::HELD_BY_FRICTION : ColliderState::HELD_BY_SCENERY),
             "why_reaction_must_stay", "the body is named first, then friction, then the pair");
      const bool said = col.reaction_disabled();  // (pbf_hip.hip refuses before; the event refuses as well)
      check("reaction_disabled(refused)", b, said);
      expect(col.reaction && same_records(b), "reaction_disabled(refused)", "the records were dropped under their reader");
      return false;
    }
    const bool said = on ? col.reaction_enabled() : col.reaction_disabled();
    check(on ? "reaction_enabled" : "reaction_disabled", b, said);
    expect(col.reaction == on && col.pushAt == 0 && col.pushRows == -1 && !records_current(), on ? "reaction_enabled" : "reaction_disabled", "records believed without a sort");
    return true;
  }
  bool set_body(bool body) {  // pbf_set_collider_body
    if (!col.lattice) return false;
    const ColliderState b = col;
    if (!body) {
      const bool said = col.body_cleared();
      check("body_cleared", b, said);
      expect(!col.body && col.posed == b.posed && col.reaction == b.reaction && same_records(b), "body_cleared", "the pose or the reaction went with the body");
      return true;
    }
    set_reaction(true);
    const ColliderState b2 = col;
    const bool said = col.body_set();
    check("body_set", b2, said);
    expect(col.body && col.posed && same_records(b2) && col.frictionRan == b2.frictionRan, "body_set", "wrong flags");
    return true;
  }
  bool set_friction(bool friction) {  // pbf_set_collider_friction
    if (!col.lattice) return false;
    const ColliderState b = col;
    if (!friction) {
      const bool said = col.friction_cleared();
      check("friction_cleared", b, said);
      expect(!col.friction && !col.frictionRan && col.reaction == b.reaction && same_records(b), "friction_cleared", "wrong flags");
      return true;
    }
    if (!col.friction) set_reaction(true);
    const ColliderState b2 = col;
    const bool said = col.friction_set();
    check("friction_set", b2, said);
    // (turned on: no pass yet; rewritten: the pass that ran still counts)
    expect(col.friction && col.frictionRan == (b2.friction && b2.frictionRan) && same_records(b2), "friction_set", "wrong flags");
    return true;
  }

  // ---- the step --------------------------------------------------------------------------------------------------------------
  void upload() { sorted = false; }  // DerivedState::arrays_replaced: nothing an observer left is believed
  void sort() {                      // stage_sort
    ++orderEpoch, sorted = true;
    if (!col.reaction) return;
    const ColliderState b = col;
    col.records_cleared(orderEpoch);
    check("records_cleared", b, false);
    expect(records_current() && col.pushRows == -1, "records_cleared", "the fresh records are not believed");
  }
  bool delta(bool rows) {  // delta_run<.., COLLIDE_REACT / COLLIDE_REACT_SCENERY>; false = "the gather path changed"
    if (col.delta_mode() != ColliderState::DELTA_REACT && col.delta_mode() != ColliderState::DELTA_REACT_SCENERY) return true;
    expect(col.reaction, "delta", "kernels that write the records run without them");
    if (!records_current()) return false;  // "needs a sort since it was enabled"
    const ColliderState b = col;
    const bool ok = col.delta_indexed(rows);
    check(rows ? "delta_indexed(rows)" : "delta_indexed(morton)", b, false);
    expect(ok == (b.pushRows < 0 || b.pushRows == int(rows)), "delta_indexed", "two indexings in a step, or one refused");
    expect(ok ? col.records_by_row() == rows : same_records(b), "delta_indexed", "wrong index kept");
    return ok;
  }
  void finalise() {  // stage_body's and stage_finalise's demands, then stage_friction
    if (col.body) expect(records_current(), "stage_body", "the body would sum records of another order");
    if (!col.friction) return;
    expect(records_current(), "stage_friction", "the pass would read records of another order");
    const ColliderState b = col;
    col.friction_passed();
    check("friction_passed", b, false);
    expect(col.frictionRan && same_records(b), "friction_passed", "wrong flags");
  }
  void step(bool rows, int iterations = 2) {
    sort();
    for (int k = 0; k < iterations; ++k) expect(delta(rows), "step", "a delta-p launch of a whole step was refused");
    finalise();
  }
  void replay() {  // restore() after a hipGraphLaunch
    ++orderEpoch, sorted = true;
    const ColliderState b = col;
    col.step_replayed(orderEpoch);
    check("step_replayed", b, false);
    expect(!col.reaction || (records_current() && col.pushRows == 0), "step_replayed", "a graphed step's records are Morton-indexed and current");
    expect(col.frictionRan == col.friction, "step_replayed", "the captured friction pass ran");
  }
};

Walk fresh(const std::string &name) {
  Walk w;
  w.name = name;
  return w;
}

// every sequence of `depth` calls out of the entry points and the step, from a fresh context
const char *kActions[] = {"install", "clear", "pose", "unpose", "react", "unreact", "body", "unbody", "friction", "unfriction",
                          "step(rows)", "step(morton)", "replay", "upload", "scenery", "unscenery"};
void act(Walk &w, int a) {
  switch (a) {
    case 0: w.set_collider(true); break;
    case 1: w.set_collider(false); break;
    case 2: w.set_pose(true); break;
    case 3: w.set_pose(false); break;
    case 4: w.set_reaction(true); break;
    case 5: w.set_reaction(false); break;
    case 6: w.set_body(true); break;
    case 7: w.set_body(false); break;
    case 8: w.set_friction(true); break;
    case 9: w.set_friction(false); break;
    case 10: w.step(true); break;
    case 11: w.step(false); break;
    case 12: w.replay(); break;
    case 13: w.upload(); break;
    case 14: w.set_scenery(true); break;
    default: w.set_scenery(false); break;
  }
}
long every_sequence(const Walk &from, int depth) {
  if (depth == 0) return 1;
  long n = 0;
  for (int a = 0; a < 16; ++a) {
    Walk w = from;
    w.name += std::string(" ") + kActions[a];
    act(w, a);
    n += every_sequence(w, depth - 1);
  }
  return n;
}

}  // namespace

int main() {
  long sequences = 0;
  {  // install, then pose, then clear pose; an update in between
    Walk w = fresh("pose");
    w.expect(!w.set_pose(true), "pose", "posed without a lattice");
    w.set_collider(true);
    const uint64_t g = w.col.gen;
    w.set_pose(true), w.set_pose(true), w.set_pose(true);
    w.expect(w.col.gen == g + 1, "pose", "an update moved gen");
    w.set_pose(false), w.set_pose(false);
    w.expect(w.col.gen == g + 2 && w.col.delta_mode() == ColliderState::DELTA_STATIC, "pose", "not back at the static kernels");
    ++sequences;
  }
  {  // reaction on, then off, with and without a lattice; the observers between enabling and the first sort
    for (bool lattice : {false, true}) {
      Walk w = fresh(lattice ? "reaction" : "reaction, no lattice");
      if (lattice) w.set_collider(true);
      w.step(true);
      w.set_reaction(true);
      w.expect(!w.records_current() && w.col.needs_identity_pose(), "reaction", "records of a step that wrote none");
      w.expect(lattice ? !w.delta(true) : w.delta(true), "reaction", "delta-p before the sort");
      w.step(true), w.step(false);
      w.expect(w.records_current() && !w.col.records_by_row(), "reaction", "the last step was Morton-indexed");
      w.upload();
      w.expect(!w.records_current(), "reaction", "records believed across an upload");
      w.set_reaction(false);
      ++sequences;
    }
  }
  {  // body on with and without a prior pose, re-placed, off; the pose stays behind
    for (bool posed : {false, true}) {
      Walk w = fresh(posed ? "body over a pose" : "body");
      w.expect(!w.set_body(true), "body", "a body without a lattice");
      w.set_collider(true);
      if (posed) w.set_pose(true);
      w.set_body(true);
      const uint64_t g = w.col.gen;
      w.expect(!w.set_pose(true) && !w.set_pose(false) && !w.col.pose_cleared() && w.col.posed, "body", "the body's pose was taken away");
      w.step(true);
      w.set_body(true), w.set_body(true);
      w.expect(w.col.gen == g && w.records_current(), "body", "a re-placed body moved gen or dropped the records");
      w.expect(!w.set_reaction(false), "body", "the reaction went off under a body");
      w.set_body(false), w.set_body(false);
      w.expect(w.col.gen == g + 1 && w.col.posed && w.col.reaction && w.col.delta_mode() == ColliderState::DELTA_REACT, "body", "off: the pose and the reaction stay");
      w.expect(w.set_pose(false) && w.set_reaction(false), "body", "the pose and the reaction are free again");
      ++sequences;
    }
  }
  {  // friction on, rewritten, off
    Walk w = fresh("friction");
    w.expect(!w.set_friction(true), "friction", "friction without a lattice");
    w.set_collider(true);
    w.step(true);
    w.set_friction(true);
    const uint64_t g = w.col.gen;
    w.expect(!w.col.friction_sums_ready(), "friction", "sums before a pass");
    w.step(true);
    w.set_friction(true);
    w.expect(w.col.gen == g && w.col.friction_sums_ready(), "friction", "a rewritten record moved gen or forgot the pass");
    w.expect(!w.set_reaction(false), "friction", "the reaction went off under friction");
    w.set_friction(false), w.set_friction(false);
    w.expect(w.col.gen == g + 1 && w.col.reaction, "friction", "off: the reaction stays");
    w.set_friction(true);
    w.expect(!w.col.friction_sums_ready(), "friction", "on again: the pass count starts over");
    w.set_friction(false);
    w.expect(w.set_reaction(false), "friction", "the reaction is free again");
    ++sequences;
  }
  {  // the reaction is refused to go while both read it: the body is named; then the lattice is replaced with everything on
    Walk w = fresh("replace");
    w.set_collider(true);
    w.set_body(true), w.set_friction(true);
    w.step(true), w.step(true);
    w.expect(!w.set_reaction(false) && w.col.why_reaction_must_stay() == ColliderState::HELD_BY_BODY, "replace", "who holds the records");
    const ColliderState b = w.col;
    w.set_collider(true);
    w.expect(w.col.reaction && w.same_records(b) && w.records_current() && w.col.needs_identity_pose(), "replace", "the reaction and its records outlive the lattice");
    w.expect(w.col.delta_mode() == ColliderState::DELTA_REACT, "replace", "mode");
    w.step(true);
    ++sequences;
  }
  {  // clearing the collider while the reaction is on
    Walk w = fresh("clear");
    w.set_collider(true);
    w.set_pose(true), w.set_reaction(true);
    w.step(true);
    w.set_collider(false);
    w.expect(w.col.reaction && !w.col.lattice && w.col.delta_mode() == ColliderState::DELTA_OFF, "clear", "the reaction stays on, the kernels are the stock ones");
    w.expect(!w.set_pose(true) && !w.set_body(true) && !w.set_friction(true), "clear", "a feature without a lattice");
    w.step(true);
    w.expect(w.set_reaction(false), "clear", "the reaction is free");
    ++sequences;
  }
  {  // sort -> delta (rows or Morton) -> delta -> friction pass over several steps; a step that changes its gather path
    Walk w = fresh("steps");
    w.set_collider(true);
    w.set_body(true), w.set_friction(true);
    for (int k = 0; k < 6; ++k) w.step(k % 3 != 0, 1 + k % 4);
    w.sort();
    w.expect(w.delta(true) && !w.delta(false) && w.delta(true) && w.col.records_by_row(), "steps", "the gather path may not change inside a step");
    w.finalise();
    w.sort();
    w.expect(w.delta(false) && !w.delta(true) && !w.col.records_by_row(), "steps", "the gather path may not change inside a step");
    ++sequences;
  }
  {  // replayed steps between eager ones
    Walk w = fresh("replay");
    w.set_collider(true);
    w.set_friction(true);
    w.replay();
    w.expect(w.col.friction_sums_ready(), "replay", "the captured pass ran");
    w.step(true), w.replay(), w.replay(), w.step(false);
    w.set_friction(false), w.set_reaction(false);
    w.replay();
    w.expect(w.col.pushAt == 0 && !w.col.friction_sums_ready(), "replay", "a replay invented records");
    ++sequences;
  }
  {  // the pair completed in both orders: the completing call turns the reaction on, and it is held while both stand
    for (bool sceneryFirst : {false, true}) {
      Walk w = fresh(sceneryFirst ? "pair, scenery first" : "pair, collider first");
      sceneryFirst ? w.set_scenery(true) : w.set_collider(true);
      w.expect(!w.col.reaction && w.col.delta_mode() == ColliderState::DELTA_STATIC && w.col.static_reads_scenery() == sceneryFirst, "pair", "one solid alone is static");
      sceneryFirst ? w.set_collider(true) : w.set_scenery(true);
      w.expect(w.col.reaction && w.col.needs_identity_pose() && w.col.delta_mode() == ColliderState::DELTA_REACT_SCENERY, "pair", "the pair runs the fifth mode with the reaction on");
      w.expect(!w.delta(true), "pair", "delta-p before the sort");
      w.step(true), w.step(false);
      w.expect(!w.set_reaction(false) && w.col.why_reaction_must_stay() == ColliderState::HELD_BY_SCENERY, "pair", "the reaction went off under the pair");
      w.set_pose(true);
      w.expect(w.col.delta_mode() == ColliderState::DELTA_REACT_SCENERY, "pair", "a pose changes the record, not the mode");
      ++sequences;
    }
  }
  {  // each solid cleared: the reaction stays on, and is then free to go
    for (bool clearScenery : {false, true}) {
      Walk w = fresh(clearScenery ? "pair, scenery cleared" : "pair, collider cleared");
      w.set_collider(true), w.set_scenery(true);
      w.step(true);
      const ColliderState b = w.col;
      clearScenery ? w.set_scenery(false) : w.set_collider(false);
      w.expect(w.col.reaction && w.same_records(b) && w.records_current(), "clear one", "the reaction and its records stay");
      w.expect(w.col.delta_mode() == (clearScenery ? ColliderState::DELTA_REACT : ColliderState::DELTA_STATIC), "clear one", "mode");
      w.expect(w.col.static_reads_scenery() == !clearScenery, "clear one", "whose lattice the static kernels read");
      w.step(true);
      w.expect(w.set_reaction(false), "clear one", "the reaction is free");
      w.expect(w.col.delta_mode() == ColliderState::DELTA_STATIC, "clear one", "the solid left is static");
      ++sequences;
    }
  }
  {  // the lattice replaced beside scenery with everything on; the scenery replaced under a body
    Walk w = fresh("replace beside scenery");
    w.set_scenery(true), w.set_collider(true);
    w.set_body(true), w.set_friction(true);
    w.step(true), w.step(true);
    w.expect(!w.set_reaction(false) && w.col.why_reaction_must_stay() == ColliderState::HELD_BY_BODY, "replace", "the body is named before the pair");
    ColliderState b = w.col;
    w.set_scenery(true);
    w.expect(w.col.body && w.col.friction && w.col.posed && w.col.frictionRan && w.records_current(), "replace", "a new scenery left the collider alone");
    b = w.col;
    w.set_collider(true);
    w.expect(w.col.scenery && w.col.reaction && w.same_records(b) && w.records_current() && w.col.needs_identity_pose(), "replace", "the reaction and its records outlive the lattice");
    w.expect(w.col.delta_mode() == ColliderState::DELTA_REACT_SCENERY, "replace", "mode");
    w.step(true);
    ++sequences;
  }
  {  // scenery alone is static on its own lattice, whatever the reaction; every install moves gen by one, clears included
    Walk w = fresh("scenery alone");
    uint64_t g = w.col.gen;
    for (bool present : {true, true, false, false, true}) {
      w.set_scenery(present);
      w.expect(w.col.gen == ++g, "scenery alone", "an install did not move gen by one");
      w.expect(w.col.delta_mode() == (present ? ColliderState::DELTA_STATIC : ColliderState::DELTA_OFF) && w.col.static_reads_scenery() == present, "scenery alone", "mode");
    }
    w.step(true);
    w.set_reaction(true);
    w.expect(w.col.delta_mode() == ColliderState::DELTA_STATIC && w.delta(true), "scenery alone", "the reaction without a lattice changes no kernel");
    w.expect(!w.set_pose(true) && !w.set_body(true) && !w.set_friction(true), "scenery alone", "a feature without a lattice");
    w.step(false);
    w.expect(w.set_reaction(false), "scenery alone", "the reaction is free");
    ++sequences;
  }
  sequences += every_sequence(fresh("all:"), 5);

  int reachable = 0;
  for (int f = 0; f < 64; ++f) {
    if (!allowed(f)) {
      if (g_seen.count(f)) std::printf("FAIL: the walks stood in the forbidden combination %d\n", f), ++g_failures;
      continue;
    }
    ++reachable;
    if (!g_seen.count(f)) std::printf("FAIL: no walk reached the combination %d\n", f), ++g_failures;
  }
  if (g_failures) std::printf("%d check(s) failed\n", g_failures);
  else std::printf("collider state ok: %ld sequences walked, %d flag combinations reached\n", sequences, reachable);
  return g_failures ? 1 : 0;
}
