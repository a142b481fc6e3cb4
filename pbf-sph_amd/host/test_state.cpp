// test_state.cpp — walks pbf::DerivedState (csrc/pbf_state.hpp) through the event sequences pbf_hip.hip performs and checks,
// after every event, the invariants the stages rely on.  No device, no library: the header alone.
// Exit status 1 if a check failed; each failure prints the sequence, the trail of events and the last event.
#include "pbf_state.hpp"

#include <cstdio>
#include <functional>
#include <string>
#include <vector>

using pbf::DerivedState;

namespace {

constexpr uint32_t kTableN = 4096;
int g_failures = 0;

// what a context is configured to do (pbf_set_option), as far as the state machine sees it
struct Opts {
  bool rows = true;        // row_mode(): the iterations run on the row-major copy
  bool rowDiffuse = true;  // option "row_diffuse"
  bool lists = true;       // neighbour lists handed from lambda to delta-p
  bool overlap = false;    // the diffusion runs beside the iterations, in scratch of its own
  bool extras = false;     // vorticity + surface tension
};

struct Walk {
  DerivedState st;
  std::string name, trail;

  void fail(const char *event, const char *what) {
    std::printf("FAIL [%s] after %s: %s\n  events: %s\n", name.c_str(), event, what, trail.c_str());
    ++g_failures;
  }
  void expect(bool ok, const char *event, const char *what) {
    if (!ok) fail(event, what);
  }
  // after EVERY event
  void check(const char *event) {
    trail += trail.empty() ? event : std::string(" > ") + event;
    expect(!st.pstarInRows || (st.rowsValid && st.rowsCurrent), event, "pstarInRows without rowsValid && rowsCurrent");
    expect(!st.rowColValid || st.rowsValid, event, "rowColValid without rowsValid");
    expect(!st.nbrRows || st.nbrValid, event, "nbrRows without nbrValid");
    expect(!(st.sorted && st.counted), event, "sorted and counted both true");
    expect(!st.delta_on_rows() || !st.delta_from_lists(), event, "delta-p both on rows and from Morton lists");
    expect((st.cur == 0 || st.cur == 1) && st.pcur >= 0 && st.pcur <= 2 && (st.rcur == 0 || st.rcur == 1), event, "role index out of range");
  }

  // ---- the stages, as pbf_hip.hip calls the events ------------------------------------------
  void drop_histogram() {
    st.histogram_dropped();
    check("histogram_dropped");
  }
  void upload(int set = 0) {  // upload_impl / pbf_upload_aos / stage_scene
    drop_histogram();
    st.arrays_replaced(set);
    check("arrays_replaced");
    expect(!st.sorted && !st.counted && !st.bricksValid && !st.rowColValid && !st.rowsValid && !st.rowsCurrent && !st.pstarInRows &&
               !st.nbrValid && !st.nbrRows && !st.qposValid && !st.omegaValid && !st.surfaceValid && !st.prePredicted,
           "arrays_replaced", "a flag survived");
    expect(st.cur == set && st.pcur == set, "arrays_replaced", "roles not reset");
  }
  void expect_predicted(const char *event) {  // predicted clears everything sorted_now sets
    expect(!st.sorted && !st.rowsValid && !st.rowsCurrent && !st.pstarInRows && !st.rowColValid && !st.qposValid &&
               !st.bricksValid && !st.nbrValid && !st.omegaValid && !st.surfaceValid,
           event, "predicted left something of the last sort standing");
    expect(st.counted && st.countedTableN == kTableN && st.pcur == st.cur, event, "no histogram / pStar not in pstar[cur]");
  }
  void predict() {
    drop_histogram();
    st.predicted(kTableN, false);
    check("predicted");
    expect_predicted("predicted");
  }
  void sort(const Opts &o) {
    expect(st.counted, "sort", "stage_sort without a histogram");
    const int from = st.cur;
    const bool rowDiffuse = o.rows && o.rowDiffuse;
    st.sorted_now(o.rows, rowDiffuse);
    check("sorted_now");
    expect(st.cur == 1 - from && st.pcur == st.cur && st.sorted && st.qposValid == !o.rows && st.pstarInRows == o.rows, "sorted_now", "roles");
    if (!rowDiffuse) brick_list();
  }
  void brick_list() {
    if (st.bricksValid) return;
    st.bricks_listed();
    check("bricks_listed");
  }
  void diffuse(const Opts &o) {
    if (o.rowDiffuse && st.diffuse_on_rows()) {
      st.diffused(false);
    } else {
      brick_list();
      st.diffused(!o.overlap);
    }
    check("diffused");
    expect(!st.rowColValid && !st.omegaValid, "diffused", "stale colour copy / vorticity kept");
  }
  void materialise() {  // materialise_pstar
    if (!st.pstarInRows) return;
    expect(st.rows_usable(), "materialise", "k_rows_to_morton would read a row copy that is not current");
    st.materialised();
    check("materialised");
  }
  void lambda(const Opts &o) {
    if (o.lists && st.rows_usable() && o.rows) {
      st.lambda_done(true, true);
      check("lambda_done(rows)");
      expect(st.pstarInRows && st.delta_on_rows(), "lambda_done(rows)", "delta-p cannot follow on the rows");
      return;
    }
    materialise();
    st.lambda_done(o.lists, false);
    check("lambda_done(morton)");
    if (o.lists && !st.qposValid) {
      st.quantised();
      check("quantised");
    }
    expect(!st.delta_on_rows() && st.delta_from_lists() == o.lists, "lambda_done(morton)", "wrong delta-p path");
  }
  void delta() {
    if (st.delta_on_rows()) {
      const int out = 1 - st.rcur;
      st.pstar_moved(true, out);
      check("pstar_moved(rows)");
      expect(st.rcur == out && st.pstarInRows && !st.qposValid && !st.nbrValid, "pstar_moved(rows)", "roles");
      return;
    }
    materialise();
    const int out = st.pcur == 2 ? st.cur : 2;  // other_pstar
    st.pstar_moved(false, out);
    check("pstar_moved(morton)");
    expect(st.pcur == out && !st.pstarInRows && !st.rowsCurrent && !st.nbrValid, "pstar_moved(morton)", "roles");
  }
  void finalise(const Opts &o, bool fuseNext) {
    if (fuseNext && !o.extras) {
      drop_histogram();
      st.predicted(kTableN, true);
      check("predicted(ahead)");
      expect_predicted("predicted(ahead)");
      expect(st.prePredicted, "predicted(ahead)", "the next step would predict again");
      return;
    }
    if (o.extras) materialise();
    st.finalised();
    check("finalised");
    expect(st.pcur == st.cur && !st.nbrValid, "finalised", "roles");
    if (o.extras) {
      expect(!st.pstarInRows, "extras", "the extras would read a stale pstar[pcur]");
      st.extras_done(true, true);
      check("extras_done");
      expect(st.omegaValid && st.surfaceValid, "extras_done", "results not readable");
    }
  }
};

using Op = std::function<void(Walk &)>;

// one step as step_impl runs it; `switchAt`: from that iteration on the options say "Morton" (changed mid-step; delta-p
// follows the lambda it got)
std::vector<Op> step_ops(Opts o, int K, bool fuseNext = false, int switchAt = -1) {
  std::vector<Op> ops;
  ops.push_back([](Walk &w) {
    if (!w.st.take_prediction()) w.predict();
    else w.check("take_prediction");
  });
  ops.push_back([o](Walk &w) { w.sort(o); });
  ops.push_back([o](Walk &w) { w.diffuse(o); });
  for (int k = 0; k < K; ++k) {
    Opts ok = o;
    if (switchAt >= 0 && k >= switchAt) ok.rows = false;
    ops.push_back([ok](Walk &w) { w.lambda(ok); });
    ops.push_back([](Walk &w) { w.delta(); });
  }
  ops.push_back([o, fuseNext](Walk &w) { w.finalise(o, fuseNext); });
  return ops;
}
void run(Walk &w, const std::vector<Op> &ops, size_t from = 0, size_t to = ~size_t(0)) {
  for (size_t i = from; i < ops.size() && i < to; ++i) ops[i](w);
}
Walk fresh(const std::string &name) {
  Walk w;
  w.name = name;
  w.upload();
  return w;
}
std::string tag(const char *what, const Opts &o, int K) {
  return std::string(what) + " rows=" + std::to_string(o.rows) + " rowDiffuse=" + std::to_string(o.rowDiffuse) + " lists=" +
         std::to_string(o.lists) + " overlap=" + std::to_string(o.overlap) + " extras=" + std::to_string(o.extras) + " K=" + std::to_string(K);
}

void all_sequences(const Opts &o, int K) {
  {  // two plain steps (pbf_step twice)
    Walk w = fresh(tag("step", o, K));
    run(w, step_ops(o, K));
    w.expect(w.st.sorted && w.st.pcur == w.st.cur, "step", "not sorted / pStar not home after a step");
    w.expect(w.st.pstarInRows == (o.rows && !o.extras), "step", "pStar in the wrong place after a step");
    run(w, step_ops(o, K));
  }
  {  // pbf_steps(3): finalise + predict fused between the steps
    Walk w = fresh(tag("steps(3)", o, K));
    run(w, step_ops(o, K, true));
    run(w, step_ops(o, K, true));
    run(w, step_ops(o, K, false));
    w.expect(!w.st.prePredicted && w.st.sorted, "steps(3)", "a prediction was left over");
  }
  for (int at = 0; at < K; ++at) {  // the options change to the Morton path between two launches of a step
    Walk w = fresh(tag("switch", o, K) + " at=" + std::to_string(at));
    run(w, step_ops(o, K, false, at));
    run(w, step_ops(o, K));
  }
  const std::vector<Op> ops = step_ops(o, K);
  for (size_t at = 0; at <= ops.size(); ++at) {
    {  // pbf_read_buffer(PBF_BUF_PSTAR) at every point of a step
      Walk w = fresh(tag("materialise", o, K) + " at=" + std::to_string(at));
      run(w, ops, 0, at);
      w.materialise();
      w.expect(!w.st.pstarInRows, "materialise", "pstar[pcur] still stale");
      run(w, ops, at);
      run(w, ops);
    }
    {  // an upload at every point of a step, then a full step
      Walk w = fresh(tag("upload", o, K) + " at=" + std::to_string(at));
      run(w, ops, 0, at);
      w.upload();
      run(w, ops);
    }
    {  // sources / drains at every point (stage_scene: the live set stays where it is; a drain compacts into the other one)
      Walk w = fresh(tag("scene", o, K) + " at=" + std::to_string(at));
      run(w, ops, 0, at);
      w.upload(w.st.cur);
      w.st.compacted(true);
      w.check("compacted");
      w.expect(!w.st.sorted && w.st.pcur == w.st.cur, "compacted", "roles");
      run(w, ops);
    }
  }
}

}  // namespace

int main() {
  int sequences = 0;
  for (int mask = 0; mask < 32; ++mask) {
    Opts o;
    o.rows = mask & 1, o.rowDiffuse = mask & 2, o.lists = mask & 4, o.overlap = mask & 8, o.extras = mask & 16;
    if (o.rows && !o.lists) continue;  // row_mode() needs the lists
    for (int K : {0, 1, 4}) all_sequences(o, K), ++sequences;
  }
  // the hand-driven slab protocol: predict -> migrate (histogram dropped, compacted) -> ghosts appended and counted -> sort
  for (bool moved : {false, true}) {
    Walk w = fresh(std::string("slab moved=") + std::to_string(moved));
    Opts o;
    w.predict();
    w.drop_histogram();
    w.st.compacted(moved);
    w.check("compacted");
    w.st.histogram_current(kTableN);
    w.check("histogram_current");
    run(w, step_ops(o, 2), 1);
    w.st.compacted(true);  // slab_finish
    w.check("compacted");
    w.expect(!w.st.sorted, "compacted", "table still trusted");
    run(w, step_ops(o, 2));
    ++sequences;
  }
  if (g_failures) std::printf("%d check(s) failed\n", g_failures);
  else std::printf("state ok: %d configurations walked\n", sequences);
  return g_failures ? 1 : 0;
}
