// pbf_hip.hip — context, launch sequence and C ABI (include/pbf_hip.h) of the gfx950 PBF-SPH step.
//
// The product path: there is NO CPU fallback anywhere in this file.  If no HIP device is usable
// pbf_create fails with PBF_ERR_NO_DEVICE and every other entry point needs a ctx.
#include "pbf_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <initializer_list>
#include <limits>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "pbf_kernels.hpp"
#include "pbf_slab.hpp"
#include "pbf_tiles.hpp"
#include "pbf_mc.hpp"
#include "pbf_whitewater.hpp"
#include "pbf_whitewater_solids.hpp"
#include "pbf_anisotropy.hpp"
#include "pbf_aniso_field.hpp"
#include "pbf_mesh_sdf.hpp"
#include "pbf_mesh_winding.hpp"
#include "pbf_comm.hpp"
#include "pbf_state.hpp"
#include "pbf_collider_state.hpp"
#include "pbf_solid_lattice.hpp"
#include "pbf_collider_pose.hpp"
#include "pbf_collider_friction.hpp"
#include "pbf_body_contact.hpp"
#include "pbf_body_contact_kernels.hpp"

using namespace pbf;

namespace {

thread_local std::string g_create_error;

// Device memory with one owner.  Every DevBuf and Pinned of this file is a member of pbf_ctx (or a local of ensure()), so the
// destructors run inside pbf_destroy's `delete ctx` — after it has made the context's device current and synchronised the
// stream — or on a grow, after ensure() has synchronised: no free ever races work that still uses the memory, and no member
// can be forgotten.  snapshot() / restore() permute p / cap among the fifteen role buffers directly; each allocation still has
// exactly one owner afterwards.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      (void)reset();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { (void)reset(); }
  hipError_t reset() {  // frees now
    const hipError_t e = p ? hipFree(p) : hipSuccess;
    p = nullptr, cap = 0;
    return e;
  }
  template <typename T> T *as() const { return static_cast<T *>(p); }
};

// Pinned host memory with one owner: `count` elements of T, allocated by the first ensure(), zero-filled (`zero` = false: the
// caller overwrites all it reads), freed with the context like a DevBuf.  Nothing is carried across a grow.
template <typename T> struct Pinned {
  T *p = nullptr;
  size_t count = 0;
  Pinned() = default;
  Pinned(const Pinned &) = delete;
  Pinned &operator=(const Pinned &) = delete;
  ~Pinned() { reset(); }
  void reset() {
    if (p) (void)hipHostFree(p);
    p = nullptr, count = 0;
  }
  hipError_t ensure(size_t n, bool zero = true) {
    if (count >= n) return hipSuccess;
    reset();
    const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), n * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    if (zero) std::memset(static_cast<void *>(p), 0, n * sizeof(T));
    count = n;
    return hipSuccess;
  }
};

// A read-back mailbox: one pinned record T whose last member `seq` the host polls.  arm() makes the record and hands out the
// word for this round (never 0: the pinned word starts there); the last kernel of the round writes the record and then,
// behind a system-scope fence, that word; receive() (below wait_for_word) spins on it and copies the record out.
template <typename T> struct Mailbox {
  Pinned<T> rec;
  uint32_t seq = 0;
  hipError_t arm(uint32_t &word) {
    word = ++seq ? seq : ++seq;
    return rec.ensure(1);
  }
};
struct SceneRecord {  // k_drain_scan's host[0] and host[1]
  uint32_t kept, seq;
};

constexpr uint32_t kTickets = 252;  // (kTickets + 4 control words = 256: one pass of k_scan_sums' workgroup zeroes them all)
constexpr uint32_t kCtlWords = kTickets + 4;
constexpr int kBrickZ = 4;

enum Stage { ST_PREDICT = 0, ST_SORT, ST_DIFFUSE, ST_LAMBDA, ST_DELTA, ST_FINALISE, ST_BUILD, ST_COUNT };
// names follow the reference's Stopwatch entries (ompsph.hpp:130,157,161,188,209,252)
const char *kStageNames[ST_COUNT] = {"advect+zindex",      "sortz+gridtable", "sph-diffuse",
                                     "sph-lambda",         "sph-delta",       "sph-finalise",
                                     "sph-lambda/list-build"};  // (a sub-interval of sph-lambda: one kernel)

struct EventPair {
  hipEvent_t a, b;
  int stage;
};

}  // namespace

// hipGraph replay of the resident step (option "graph"): everything host-side that one step reads AND leaves behind —
// which physical buffer plays which role, the whole derived state — so that a replayed graph (or the rollback of a failed
// capture) can put the context into the state the captured step left (found) it in.  Inside a GraphKey it is also the key
// under which a captured step is found again; there `st` is reduced to DerivedState::step_key.
struct StepState {
  DerivedState st;
  bool hasObstacles;
  uint32_t tableN, gatherSeq;
  uint64_t extent[3];
  double minExtent[3];
  void *bufs[15];  // pos4[2] vel4[2] col4[2] id[2] type[2] key[2] pstar[3]: a step swaps them around
  size_t caps[15];
};
struct GraphEntry {
  hipGraphExec_t exec = nullptr;
  StepState after;
};
struct GraphKey {
  StepState before;
  unsigned char params[sizeof(double) * 11 + 32];  // dt, scale, force, bounds, iteration, xsph, vorticity, cohesion, adhesion
  uint64_t n;
  uint64_t collider;  // ColliderState::gen: a replay never runs on a lattice (the collider's or the scenery's) that has been
                      // replaced or freed, nor another launch sequence
  uint64_t contact;   // bodycontact::Mode::gen: the body's contact passes, their number and their point buffer
  int options[12];
  bool operator<(const GraphKey &o) const { return std::memcmp(this, &o, sizeof(GraphKey)) < 0; }
};

struct pbf_ctx {
  pbf_desc desc{};
  int device = 0;
  bool fp64 = false;
  bool fast = false;
  hipStream_t stream = nullptr;
  bool ownStream = false;
  std::string err;

  size_t n = 0;
  size_t cap = 0;        // particle capacity of the SoA buffers
  bool hasObstacles = false;
  DerivedState st;       // which buffer holds the truth: roles and validity flags, changed through its events only (pbf_state.hpp)
  // two sets (sort scatters from one into the other)
  DevBuf pos4[2], vel4[2], col4[2], id[2], type[2], key[2];
  DevBuf pstar[3];       // [0],[1]: sort ping-pong partner of set 0/1 ; [2]: Jacobi partner
  DevBuf count, table, blockSums, permTmp, wells, staging;
  DevBuf cellSlot;  // per particle: its slot among its bucket's members, handed out by the histogram's atomics (k_scatter_slots)
  // slab decomposition (pbf_slab_*): bookkeeping of what was sent / received this step
  DevBuf slotOf, selCounts, selTotals, ghostSrcL, ghostSrcR, colHist;
  bool slabActive = false, realObstacles = false;
  bool ghostsPending = false;  // pbf_slab_step leaves the copies in place (the next step's migration select drops them);
                               // anything that looks at the particle arrays from outside drops them first (drop_ghosts)
  bool slabConfigured = false;  // pbf_slab_configure: rank-local x frame for the keys (compact table per rank)
  pbf_slab_cut slabCut{0, 0, 0, 0};
  uint32_t xoff = 0;
  int32_t shiftL = 0, shiftR = 0;
  // pbf_slab_attach: the whole step incl. the exchanges runs inside the library (pbf_slab_step)
  pbf_comm *comm = nullptr;  // not owned
  std::vector<uint32_t> cuts;
  uint32_t capMig = 0, capGhost = 0;  // records in the FIRST message of an assembly round (the rest follows when needed)
  uint32_t wireCap = 0;               // records the wire buffers hold per neighbour
  DevBuf wireSend[2], wireRecv[2];
  DevBuf wireGhost[2];               // the ghost round's send buffers (packed by the same select pass as the migrants')
  bool slabStepMode = false;         // inside pbf_slab_step: predict classifies (StepConsts::slabOn)
  size_t sortLive = 0;               // pbf_slab_step: particles that take part in this step's sort (the others are dead slots)
  uint32_t ghostAt = 0;              // pre-sort index of the first copy received this step (k_unpack_field)
  uint32_t slabSeq = 0;              // sequence number of the next read-back (k_slab_counts -> pinned host word)
  uint64_t slabHostSyncs = 0;        // host read-backs inside pbf_slab_step so far (2 per step: the two assembly rounds)
  Pinned<uint32_t> hostCounts;     // read-back of the assembly rounds' counts (16 words)
  size_t reserve = 0;        // pbf_reserve: capacity kept for migrants and ghost copies
  uint32_t nOwned = 0, sentL = 0, sentR = 0, gotL = 0, gotR = 0;
  // marching cubes (pbf_surface)
  DevBuf latticePN, latticeC, mcCounts, mcOffsets, mcSums, meshV, meshN, meshC, mcNear;
  Pinned<char> meshHost;  // staging of the last mesh (pbf_map_mesh)
  bool meshStaged = false;
  uint64_t mcSample[3] = {0, 0, 0};
  uint64_t mcTriangles = 0;
  // pbf_surface_indexed: per node the count of crossed owned edges, then (first vertex << 3) | mask; its scan; the index triples
  DevBuf mcEdgeWord, mcEdgeOffsets, mcEdgeSums, meshT;
  enum MeshKind { MESH_NONE, MESH_SOUP, MESH_INDEXED };
  MeshKind meshKind = MESH_NONE;  // what the last surface call left in meshV / meshN / meshC (3 per triangle, or 1 per crossed edge)
  uint64_t mcVertices = 0;
  DevBuf qpos;               // 8-byte quantised pStar for the list build (k_build_lists_op)
  DevBuf nbrList, nbrCount;  // neighbour lists handed from the lambda launch to the delta launch: NBR_ROWS slots per particle
  // option "row_major": the iterations' working set also laid out cell-row-major (csrc/pbf_kernels.hpp RowArrays)
  int rowMajor = 1;           // default ON since round 3: -3 % per step at 1 M, -10 % at 4 M (profiles/r03_matrix.txt)
  DevBuf rowPstar[2], rowMass, rowQpos, rowXYZ, rowType, rowSlotOf, linTable, linSums;
  DevBuf rowCol, rowMortonOf, rowSegs;  // k_diffuse_rows: the colours in row order, slot -> Morton index, non-empty segments
  uint32_t rowSegShift = 0;
  uint32_t diffuseCap = 0;   // option "diffuse_cap" (diagnostic): records in k_diffuse_rows' tile, 0 = default
  int rowDiffuse = 1;        // option "row_diffuse": the diffusion runs on the row-major copy (k_diffuse_rows)
  uint32_t rowShift = 0;      // the row grid is the cube [0, 1 << rowShift)^3
  uint64_t nbrExtraAt = 0;   // ... + behind them a pool of NBR_EXTRA-slot chunks for the particles that need more (NbrLists)
  uint32_t nbrChunks = 0, nbrChunksOpt = 0;
  // pbf_set_surface_tension (opt-in, Akinci 2013): coefficients, the two Jacobi fields of its passes (allocated on first use)
  double cohesion = 0, adhesion = 0;
  DevBuf surfA, surfB;         // A = {0, rho}; B = {n, rho} (PBF_BUF_SURFACE, while st.surfaceValid)
  // The solids (opt-in): which of lattice / scenery / pose / reaction / body / friction is on and what the step's reaction
  // records describe, changed through its events only (pbf_collider_state.hpp: the rules are there); below it, the memory.
  ColliderState col;
  // pbf_set_collider (csrc/pbf_collider.hpp) and pbf_set_scenery (one static lattice in the world frame beside it): each
  // lattice in N on the device and the setting as given (pbf_solid_lattice.hpp), changed by solid_install only
  SolidLattice<DevBuf> solid[2];  // [ColliderState::COLLIDER], [ColliderState::SCENERY]
  // pbf_set_collider_pose: the one ColliderPose<N> record the posed kernels read through a pointer (allocated by the first call)
  DevBuf colliderPose;
  // pbf_set_collider_reaction: the records {A, hits}, {B, 0} of DeltaOp<.., COLLIDE_REACT> (2 vec4<N> per particle, sized to
  // the capacity), the step counter its clear bumps, the partial sums of pbf_collider_reaction and its pinned record
  DevBuf pushRec, pushCtl, pushPartials, pushOut;
  Mailbox<WrenchRecord> hostWrench;
  // pbf_set_collider_body: the one colliderbody::Record on the device (parameters and state; allocated by the first call)
  DevBuf bodyRec;
  Mailbox<BodyStateRecord> hostBody;
  // pbf_set_collider_body_contact (csrc/pbf_body_contact.hpp): on / off, the point count, the passes per step and the
  // generation, changed through its events only; the configuration as given; the body's surface points in N (body frame), one
  // partial record per DIAG_TILE points, the one bodycontact::Record on the device, and the observer's pinned mailbox
  bodycontact::Mode contact;
  pbf_body_contact contactCfg{};
  DevBuf contactPoints, contactPartials, contactRec;
  Mailbox<ContactStateRecord> hostContact;
  // pbf_set_collider_friction: the record {mu, V, W} the pass reads through a pointer, the device's counters, the pass's own
  // partial records (they outlive the step: the observer and the next step's body stage fold them)
  DevBuf frictionRec, frictionCtl, frictionPartials;
  Mailbox<WrenchRecord> hostFriction;
  // "sdf_cull": pbf_sdf_from_mesh / pbf_set_collider_mesh skip the triangles out of a brick's reach (same bytes, 5 - 7 x faster)
  bool sdfCull = true;
  // "sdf_launch_pairs": the cap on lane-triangle pairs per launch of the distance fold and the winding fold (0 = each fold's own)
  uint64_t sdfLaunchPairs = 0;
  // pbf_set_sources / pbf_set_drains (ompsph.hpp:93-118 on resident state): the settings as given, their device images in N,
  // the compaction's per-tile counts and total, the pinned words of the drained count's read-back {total, sequence number}
  std::vector<pbf_source> sources;
  std::vector<pbf_drain> drains;
  uint32_t emitTotal = 0;  // particles the sources emit per step
  size_t uploaded = 0;     // particles of the last upload: with pbf_reserve the sources' bound is max(reserve, uploaded)
  DevBuf sceneSources, sceneDrains, drainCounts;
  Mailbox<SceneRecord> hostScene;
  uint64_t sceneHostSyncs = 0;
  DevBuf queryPoints, queryCounts, queryIds;  // pbf_query_cells
  // pbf_sample_points / pbf_sample_lattice: the uploaded points in N, and one allocation holding the call's SoA outputs
  // {rho, weight, mv, mc, count, outside}.  Scratch of an observer: no step reads either.
  DevBuf samplePoints, sampleOut;
  // pbf_diagnostics: the density pass's own outputs (N[cap] rho, uint32[cap] neighbour counts; allocated with the first
  // density request), one partial record per DIAG_TILE particles, the pinned record the last kernel writes and the host
  // polls.  diagRhoAt: the order epoch (below) diagRho's pass was made at (PBF_BUF_DENSITY).
  DevBuf diagRho, diagNbr, diagPartials;
  Mailbox<DiagRecord> hostDiag;
  uint64_t diagRhoAt = 0;
  // What an observer leaves behind for a later read describes the sorted set it ran on: it goes stale with every sort
  // (stage_sort, or a replayed one: restore), which bumps orderEpoch, and is only ever believed while st.sorted holds, which
  // every event that changes the arrays clears; record_current() asks both.  0 = never made.  An observer-side fact, not
  // derived state of the step: it is no part of DerivedState.
  uint64_t orderEpoch = 1;
  // pbf_whitewater_* (csrc/pbf_whitewater.hpp): the configuration, the pool in two sets (the compaction moves from one into
  // the other), the scratch of its passes — k_sample's outputs at the pool's particles, the two scans' inputs and results,
  // the normal pass's two fields (its own: surfA / surfB belong to the surface-tension pass), the potentials (PBF_BUF_WHITEWATER,
  // while current like diagRho: wwPotAt) — and the pinned record the host polls.
  // An observer's state like the diagnostics': no step reads any of it.
  bool wwOn = false;
  pbf_whitewater ww{};
  uint64_t wwFrame = 0;
  size_t wwCount = 0;
  int wwCur = 0;
  DevBuf wwPos[2], wwVel[2], wwKind[2], wwParent[2];
  DevBuf wwSample, wwAlive, wwAliveOff, wwSums, wwFieldA, wwFieldB, wwPot, wwEmit, wwOffset, wwChildKind;
  Mailbox<WwRecord> hostWw;
  uint64_t wwPotAt = 0;
  // pbf_set_whitewater_solids (csrc/pbf_whitewater_solids.hpp): a wish that outlives every solid — the setting as given, the
  // whitewater steps run since it was turned on, the per-workgroup partial counts of its two kernels (sized to the pool's
  // capacity: ww_solids_buffers) and the device's WwSolidsRecord.  No ColliderState mode, no graph key: the step never reads it.
  bool wwSolidsOn = false;
  pbf_whitewater_solids wwSolids{};
  uint64_t wwSolidsSteps = 0;
  bool wwSolidsFolded = false;  // the last whitewater step ran the kernels and wrote wwSolidsRec (else its counts are zero)
  DevBuf wwSolidsPartials, wwSolidsRec;
  // pbf_anisotropy_compute (csrc/pbf_anisotropy.hpp): AnisotropyOp's outputs in one allocation sized to the capacity —
  // {centre 3, G 6, axes 9, radii 3} values of N and one uint32 per particle — made by the first call.  Scratch of an
  // observer: no step reads or writes it.
  DevBuf anisoOut;
  // pbf_surface_anisotropic (csrc/pbf_aniso_field.hpp): three vec4 per particle, made from anisoOut by k_aniso_pack
  DevBuf anisoRec;
  // advance() path: the caller's std::vector<Particle> buffer, page-locked in place (hipHostRegister) so the per-frame
  // 56-byte-per-particle upload and download are plain DMA instead of the runtime's pageable staging
  void *regPtr = nullptr;
  size_t regBytes = 0;
  size_t stagedBytes = 0;  // bytes of `staging` that hold a defined AoS image (padding bytes of a download come from it)
  // option "graph" (default OFF): pbf_steps replays each distinct step as a captured hipGraph (one graph launch instead
  // of ~25 kernel launches); stage timing, wells, growing buffers or a box that moves every frame fall back to eager.
  // Measured on MI355X / ROCm 7 (tools/graph_ab.sh): replay is SLOWER than the eager launches — 0.294 vs 0.269 ms/step
  // at 16 K particles, 0.512 vs 0.479 at 256 K, 1.724 vs 1.709 at 1 M: the step is never host-launch bound (the host
  // enqueues a step in ~90 us) and a graph does not shorten the dependent-kernel boundary.
  int graphMode = 0;
  std::map<GraphKey, GraphEntry> graphs;
  uint64_t allocEpoch = 0;     // bumped by every hipMalloc of ensure(): a step that allocated is not captured
  uint32_t graphMisses = 0;    // captures without a replay in between: a scene that never repeats turns graphs off
  uint64_t graphReplays = 0, graphCaptures = 0;
  pbf_params lastParams{};   // the params of the last stage call (entry points without a params argument derive their consts from it)
  bool haveParams = false;
  bool reuseLists = true;    // option "reuse_lists"
  // option "split_build": 0 = lambda builds the neighbour lists while it gathers on fp32 candidates (k_gather_lists<SAVE>);
  // 4 / 5 = the build is a launch of its own (k_build_lists_op<ListOnlyOp> on quantised pairs, 2 / 4 pair loads per trip)
  // followed by a list-driven lambda; 8 (default) = the same kernel with lambda riding on its flushes
  // (k_build_lists_op<LambdaOp>: one launch, no list read for lambda).  (Round 1's intermediate build kernels, values 1-3,
  // are gone.)
  int splitBuild = 8;
  int pipeline = -1;         // option "pipeline": software-pipelined list readers (bit-identical either way); -1 = auto = off
                             // (measured at 1 M, round 3: fp32 +3 %, fp64 +2.4 % per step with it)
  int coop = 0;              // option "coop": 0 = one lane per particle (bit-exact), 2 / 4 / 8 = lanes sharing a particle's
                             // list with a wave-shuffle reduction (k_gather_from_lists_coop; rounding-level differences)
  // options "build_wg" / "reader_wg" ("iter_wg" sets both): the workgroup width of the row build (k_build_rows_op) and of the
  // plain row reader (k_gather_from_lists<.., false, true>), 64 / 128 / 256; 0 = the default, kIterWgBuild / kIterWgReader.  The
  // lists are the same at every width, so either may change between any two launches; no derived state depends on them.
  int buildWg = 0, readerWg = 0;
  bool fusePredict = true;   // option "fuse_predict": pbf_steps runs finalise(t) + predict(t + 1) as one kernel
  bool cellDiffuse = true;   // option "cell_diffuse": one walk per occupied cell instead of one per particle
  // option "overlap_diffuse" (default on): inside pbf_step the colour diffusion — memory-latency bound, 85 % of its wave
  // time parked — runs on a side stream beside the VALU-bound solver iterations (nothing else touches colours)
  bool overlapDiffuse = true;
  bool overlapDiffuseForced = false;  // option / env set explicitly: no size heuristic
  hipStream_t sideStream = nullptr;
  hipStream_t copyStream = nullptr;  // pbf_download_aos_begin's DMA
  hipEvent_t evPacked = nullptr;
  bool downloadPending = false;
  hipEvent_t evFork = nullptr, evJoin = nullptr;
  bool diffusePending = false;
  DevBuf diffSum, diffCnt;   // the overlapped diffusion's own per-cell scratch
  bool fuseDiffuse = false;  // option "fuse_diffuse": pbf_step folds the diffuse walk into the first lambda launch
                             // (bit-identical; measured 2 % SLOWER at 1 M — the colour loads stall the filter loop — so off)
  // pbf_steps' request to the step it starts: the NEXT step's predict rides on this step's finalise (k_finalise_predict)
  bool fuseNextPredict = false;
  // non-empty brick list; brickCtl = {nActive, ticket[kTickets], nBigCells, row tail allocator, number of row segments}
  DevBuf bricks, brickCtl;
  DevBuf bigCells;          // cells with more than BIG_CELL members this step (k_sort_big_cells)
  uint32_t gatherSeq = 0;   // which ticket word the next persistent gather launch uses
  int numCUs = 256;
  uint32_t timingMask = 0xFFFFFFFFu;  // option "timing_mask": which stages PBF_FLAG_STAGE_TIMING brackets with events
  uint32_t padLds = 0;      // option "pad_lds": occupancy limiter for k_gather_global
  std::map<const void *, size_t> ldsLimit;  // kernel -> the dynamic-LDS limit this context has raised it to (raise_lds_limit)
  int gatherKind = 1;       // 0 = global walk (k_gather_global), 1 = neighbour lists (default), 3 = LDS tiles per brick (pbf_tiles.hpp)
  uint32_t tileCap = 0, listMax = 0;  // 0 = defaults (env PBF_TILE_CAP / PBF_LIST_MAX override)
  size_t tableCap = 0;   // entries allocated in count/table
  uint32_t tableN = 0;
  uint64_t extent[3] = {0, 0, 0};
  double minExtent[3] = {0, 0, 0};

  // stage timing
  std::vector<EventPair> pending;
  std::vector<hipEvent_t> freeEvents;
  double stageMs[ST_COUNT] = {0};
  uint64_t stageCalls[ST_COUNT] = {0};
};

namespace {

#define HIPCHK(ctx, expr)                                                                          \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                              \
      return PBF_ERR_HIP;                                                                          \
    }                                                                                              \
  } while (0)

int fail(pbf_ctx *ctx, int code, const std::string &msg) {
  ctx->err = msg;
  return code;
}

int ensure(pbf_ctx *ctx, DevBuf &b, size_t bytes, bool zero = false) {
  if (b.cap >= bytes) return PBF_OK;
  DevBuf fresh;
  fresh.cap = bytes + bytes / 4 + 256;
  HIPCHK(ctx, hipMalloc(&fresh.p, fresh.cap));
  ctx->allocEpoch++;
  if (zero) HIPCHK(ctx, hipMemsetAsync(fresh.p, 0, fresh.cap, ctx->stream));
  if (b.p) {
    // contents are never carried across a grow: callers refill
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, b.reset());
  }
  b = std::move(fresh);
  return PBF_OK;
}

// what an observer left at order epoch `madeAt` (pbf_ctx::orderEpoch) still describes the arrays: pbf_read_buffer may hand it out
bool record_current(const pbf_ctx *ctx, uint64_t madeAt) { return madeAt == ctx->orderEpoch && ctx->st.sorted; }

template <typename N> size_t vsz() { return sizeof(vec4<N>); }

int ensure_particles(pbf_ctx *ctx, size_t n) {
  n = std::max(n, ctx->reserve);
  if (ctx->cap >= n) return PBF_OK;
  // slab mode (a reserve was asked for): pbf_slab_step leaves the slots of the particles that left — migrants, last step's
  // copies — in place until the step's sort drops them, so a step transiently needs more slots than live particles
  if (ctx->reserve) n += n / 4 + 65536;
  const size_t v = ctx->fp64 ? sizeof(double4) : sizeof(float4);
  for (int s = 0; s < 2; ++s) {
    if (int rc = ensure(ctx, ctx->pos4[s], n * v)) return rc;
    if (int rc = ensure(ctx, ctx->vel4[s], n * v)) return rc;
    if (int rc = ensure(ctx, ctx->col4[s], n * v)) return rc;
    if (int rc = ensure(ctx, ctx->id[s], n * 8)) return rc;
    if (int rc = ensure(ctx, ctx->type[s], n)) return rc;
    if (int rc = ensure(ctx, ctx->key[s], n * 4)) return rc;
  }
  for (int s = 0; s < 3; ++s)
    if (int rc = ensure(ctx, ctx->pstar[s], n * v)) return rc;
  if (int rc = ensure(ctx, ctx->permTmp, n * 4)) return rc;
  if (int rc = ensure(ctx, ctx->cellSlot, n * 4)) return rc;
  if (int rc = ensure(ctx, ctx->slotOf, n * 4)) return rc;
  if (int rc = ensure(ctx, ctx->qpos, (n + QPOS_PAD) * 8)) return rc;
  if (int rc = ensure(ctx, ctx->nbrCount, n * 4)) return rc;
  // two-tier lists: NBR_ROWS slots per particle in rows + a pool of NBR_EXTRA-slot chunks for the few longer lists
  // (one allocation: a lane addresses both tiers from its row pointer with a 32-bit word offset — which caps the whole at
  // 2^31 words, i.e. ~45 M particles per GPU; beyond that the pool is left out and longer lists walk)
  const size_t rowWords = ((n + BLOCK - 1) / BLOCK) * size_t(NBR_ROWS) * BLOCK;
  ctx->nbrChunks = ctx->nbrChunksOpt ? ctx->nbrChunksOpt : uint32_t(n / 8 + 1024);  // (option "nbr_chunks": tests shrink the pool)
  if (rowWords + size_t(ctx->nbrChunks) * NBR_EXTRA >= (size_t(1) << 31)) ctx->nbrChunks = 0;
  ctx->nbrExtraAt = rowWords;
  if (int rc = ensure(ctx, ctx->nbrList, (rowWords + size_t(ctx->nbrChunks) * NBR_EXTRA + 64) * 4)) return rc;
  ctx->cap = n;
  return PBF_OK;
}

template <typename N> ParticleArrays<N> arrays(pbf_ctx *ctx, int set, int pstarIdx) {
  ParticleArrays<N> a;
  a.pos4 = ctx->pos4[set].as<vec4<N>>();
  a.vel4 = ctx->vel4[set].as<vec4<N>>();
  a.col4 = ctx->col4[set].as<vec4<N>>();
  a.pstar = ctx->pstar[pstarIdx].as<vec4<N>>();
  a.id = ctx->id[set].as<uint64_t>();
  a.type = ctx->type[set].as<uint8_t>();
  a.key = ctx->key[set].as<uint32_t>();
  return a;
}

// ---- per-step constants, in N, as the reference computes them ---------------------------------
template <typename N> N piN() { return std::acos(-N(1)); }
// sph.hpp:251-253 — std::pow(N, int) promotes to double for N = float; the result is rounded to N
template <typename N> N poly6_factor(N h) { return N(N(315.0) / (N(64.0) * piN<N>() * std::pow(h, 9))); }
template <typename N> N spiky_factor(N h) { return N(-(N(45.0) / (piN<N>() * std::pow(h, 6)))); }

template <typename N> int make_consts(pbf_ctx *ctx, const pbf_params *p, StepConsts<N> &c) {
  const N h = N(ctx->desc.h), scale = N(p->scale);
  c.h = h, c.dt = N(p->dt), c.scale = scale;
  // ompsph.hpp:132-135
  const N padding = h * 2;
  uint64_t ext[3];
  for (int i = 0; i < 3; ++i) {
    c.force[i] = N(p->constant_force[i]);
    c.minB[i] = N(p->min_bound[i]);
    c.maxB[i] = N(p->max_bound[i]);
    const N lo = c.minB[i] / scale - padding;
    const N hi = c.maxB[i] / scale + padding;
    c.minExtent[i] = lo;
    ext[i] = static_cast<uint64_t>((hi - lo) / h);
    ctx->minExtent[i] = double(lo);
  }
  for (int i = 0; i < 3; ++i) {
    if (ext[i] > 1023)
      return fail(ctx, PBF_ERR_INVALID, "grid extent exceeds the 10-bit-per-axis Morton range (curves.h:72-88)");
    ctx->extent[i] = ext[i];
  }
  c.xoff = 0;
  c.slabOn = 0, c.sxlo = 0, c.sxhi = 0xFFFFFFFFu, c.sHasL = c.sHasR = 0;
  if (ctx->slabStepMode && ctx->comm) {  // pbf_slab_step: predict sorts the particles into stayers / leavers / old copies
    const uint32_t xo = ctx->slabConfigured ? ctx->xoff : 0u;
    const int r = ctx->comm->rank, nr = ctx->comm->nranks;
    c.slabOn = 1;
    c.sxlo = ctx->cuts[r] - std::min(ctx->cuts[r], xo), c.sxhi = ctx->cuts[r + 1] - std::min(ctx->cuts[r + 1], xo);
    c.sHasL = r > 0 ? 1u : 0u, c.sHasR = r + 1 < nr ? 1u : 0u;
  }
  if (ctx->slabConfigured) {  // keys live in this rank's x frame: columns [xoff, right ghost column]
    c.xoff = ctx->xoff;
    const uint64_t hi = ctx->slabCut.has_right ? std::min<uint64_t>(ext[0], uint64_t(ctx->slabCut.xhi) + 1) : ext[0];
    ext[0] = hi > ctx->xoff ? hi - ctx->xoff : 1;
  }
  c.tableN = morton_encode(uint32_t(ext[0]), uint32_t(ext[1]), uint32_t(ext[2]));  // sph.hpp:240
  if (c.tableN == 0) return fail(ctx, PBF_ERR_INVALID, "empty grid (max_bound <= min_bound?)");
  c.poly6Factor = poly6_factor<N>(h);
  c.spikyFactor = spiky_factor<N>(h);
  {  // ompsph.hpp:213 with poly6Kernel of ompsph.hpp:67-69
    const N r = N(CorrDeltaQ * h);
    const N d = (h * h) - r * r;
    c.p6DeltaQ = r <= h ? c.poly6Factor * (d * d * d) : N(0);
  }
  c.diffuseT = c.dt / N(750.0);
  c.h2filter = (h * h) * N(1.00001);
  c.n = uint32_t(ctx->n);
  c.nWells = uint32_t(p->n_wells > 0 ? p->n_wells : 0);
  c.hasObstacles = ctx->hasObstacles ? 1u : 0u;
  ctx->tableN = c.tableN;
  return PBF_OK;
}

// A histogram that was built but never consumed (predict without sort) must not leak into the next one.
int drop_histogram(pbf_ctx *ctx) {
  if (ctx->st.counted && ctx->count.p) HIPCHK(ctx, hipMemsetAsync(ctx->count.p, 0, ctx->count.cap, ctx->stream));
  ctx->st.histogram_dropped();
  return PBF_OK;
}

int ensure_table(pbf_ctx *ctx, uint32_t tableN) {
  const size_t entries = size_t(tableN) + 2;  // buckets 0..tableN (+1 overflow) and the closing total
  if (ctx->tableCap >= entries) return PBF_OK;
  // count must start (and always returns to) all-zero: k_scatter_slots stores 0 over every bucket the producers raised (the
  // member that holds slot 0 does), and a histogram that never reaches a scatter is cleared by drop_histogram
  if (ctx->count.p) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, ctx->count.reset());
  }
  if (int rc = ensure(ctx, ctx->count, (entries + SCAN_TILE) * 4, true)) return rc;
  if (int rc = ensure(ctx, ctx->table, (entries + SCAN_TILE) * 4)) return rc;
  const size_t nb = (entries + SCAN_TILE - 1) / SCAN_TILE + 1;
  if (int rc = ensure(ctx, ctx->blockSums, nb * 4)) return rc;
  if (int rc = ensure(ctx, ctx->bricks, (entries / Brick<kBrickZ>::HOME + 2) * 4)) return rc;
  if (int rc = ensure(ctx, ctx->brickCtl, kCtlWords * 4)) return rc;
  ctx->tableCap = ctx->count.cap / 4 - SCAN_TILE;
  return PBF_OK;
}

// ---- stage timing (Stopwatch analogue, utils.hpp:15-57) ----------------------------------------
hipEvent_t get_event(pbf_ctx *ctx) {
  if (!ctx->freeEvents.empty()) {
    hipEvent_t e = ctx->freeEvents.back();
    ctx->freeEvents.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
int resolve_events(pbf_ctx *ctx) {
  if (ctx->pending.empty()) return PBF_OK;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (auto &ep : ctx->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ep.a, ep.b) == hipSuccess) {
      ctx->stageMs[ep.stage] += ms;
      ctx->stageCalls[ep.stage] += 1;
    }
    ctx->freeEvents.push_back(ep.a);
    ctx->freeEvents.push_back(ep.b);
  }
  ctx->pending.clear();
  return PBF_OK;
}
struct StageTimer {
  pbf_ctx *ctx;
  EventPair ep{};
  bool on;
  StageTimer(pbf_ctx *c, int stage)
      : ctx(c), on((c->desc.flags & PBF_FLAG_STAGE_TIMING) != 0 && ((c->timingMask >> stage) & 1u) != 0) {
    if (!on) return;
    ep.a = get_event(ctx), ep.b = get_event(ctx), ep.stage = stage;
    (void)hipEventRecord(ep.a, ctx->stream);
  }
  ~StageTimer() {
    if (!on) return;
    (void)hipEventRecord(ep.b, ctx->stream);
    ctx->pending.push_back(ep);
    if (ctx->pending.size() > 8192) (void)resolve_events(ctx);
  }
};

// (at least one workgroup: a slab may own no particle at all, and every kernel bounds-checks its index)
inline dim3 grid_for(size_t n) { return dim3(unsigned(std::max<size_t>(1, (n + BLOCK - 1) / BLOCK))); }
// the row iteration kernels at workgroup width wg: BLOCK / wg units per chunk, the grid counts units (iter_unit)
inline dim3 iter_grid(size_t n, unsigned wg) { return dim3(grid_for(n).x * (unsigned(BLOCK) / wg)); }
// The default widths (A/B builds override them), measured at 1 M (profiles/wave_workgroups_1m.md).  The build is capped at four
// waves per SIMD by its staging LDS, which a CU gets back only when a workgroup's last wave ends: one wave per workgroup, every
// launch of the build 3 to 4.5 us shorter (128: half of that).  The reader is not LDS-capped and measured the same at every width.
#ifndef PBF_BUILD_WG
#define PBF_BUILD_WG 64
#endif
#ifndef PBF_READER_WG
#define PBF_READER_WG 256
#endif
constexpr int kIterWgBuild = PBF_BUILD_WG, kIterWgReader = PBF_READER_WG;
inline int iter_wg(int option, int dflt) { return option ? option : dflt; }

#define LAUNCH_CHECK(ctx)                                                  \
  do {                                                                     \
    hipError_t e_ = hipGetLastError();                                     \
    if (e_ != hipSuccess) {                                                \
      (ctx)->err = std::string("kernel launch: ") + hipGetErrorString(e_); \
      return PBF_ERR_HIP;                                                  \
    }                                                                      \
  } while (0)

// the precision the context was created with, and (DISPATCH_FAST, inside a function templated on N) PBF_FLAG_FAST_MATH
#define DISPATCH(ctx, fn, ...) ((ctx)->fp64 ? fn<double>(__VA_ARGS__) : fn<float>(__VA_ARGS__))
#define DISPATCH_FAST(ctx, fn, ...) ((ctx)->fast ? fn<N, true>(__VA_ARGS__) : fn<N, false>(__VA_ARGS__))

int upload_wells(pbf_ctx *ctx, const pbf_params *p) {
  if (p->n_wells <= 0) return PBF_OK;
  if (!p->wells) return fail(ctx, PBF_ERR_INVALID, "n_wells > 0 but wells == NULL");
  const size_t cnt = size_t(p->n_wells) * 4;
  const size_t esz = ctx->fp64 ? 8 : 4;
  if (int rc = ensure(ctx, ctx->wells, cnt * esz)) return rc;
  if (ctx->fp64) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->wells.p, p->wells, cnt * 8, hipMemcpyHostToDevice, ctx->stream));
  } else {
    std::vector<float> w(cnt);
    for (size_t i = 0; i < cnt; ++i) w[i] = float(p->wells[i]);
    HIPCHK(ctx, hipMemcpyAsync(ctx->wells.p, w.data(), cnt * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // w is a temporary
  }
  return PBF_OK;
}

// Spin on a pinned word a kernel writes last (behind a system-scope fence).  A kernel fault or a lost device would leave it
// unwritten for ever: every ~2 ms of spinning the stream is queried, and an error (or an idle stream without the word) ends
// the wait.
int wait_for_word(pbf_ctx *ctx, const volatile uint32_t *word, uint32_t seq, const char *what) {
  for (uint64_t spin = 1;; ++spin) {
    if (*word == seq) return PBF_OK;
    if ((spin & 0xFFFFu) == 0) {
      const hipError_t e = hipStreamQuery(ctx->stream);
      if (e == hipSuccess) {
        if (*word == seq) return PBF_OK;
        return fail(ctx, PBF_ERR_HIP, std::string(what) + ": the stream went idle without delivering the counts");
      }
      if (e != hipErrorNotReady) {
        ctx->err = std::string(what) + ": " + hipGetErrorString(e);
        return PBF_ERR_HIP;
      }
    }
  }
}
// the mailbox's round is in: `out` is the front of its record (read through a plain pointer, hence the fence after the polled word)
template <typename T, typename Out> int receive(pbf_ctx *ctx, const Mailbox<T> &box, const char *what, Out &out) {
  static_assert(sizeof(Out) <= offsetof(T, seq), "the record ends with the polled word");
  if (int rc = wait_for_word(ctx, &box.rec.p->seq, box.seq, what)) return rc;
  std::atomic_thread_fence(std::memory_order_acquire);
  std::memcpy(&out, box.rec.p, sizeof(Out));
  return PBF_OK;
}

// ---- stages ------------------------------------------------------------------------------------
template <typename N> int stage_predict(pbf_ctx *ctx, const pbf_params *p) {
  StepConsts<N> c;
  if (int rc = make_consts<N>(ctx, p, c)) return rc;
  if (int rc = ensure_table(ctx, c.tableN)) return rc;
  if (int rc = drop_histogram(ctx)) return rc;
  if (int rc = upload_wells(ctx, p)) return rc;
  StageTimer t(ctx, ST_PREDICT);
  const int s = ctx->st.cur;
  hipLaunchKernelGGL((k_predict<N>), grid_for(ctx->n), dim3(BLOCK), 0, ctx->stream, c,
                     ctx->pos4[s].as<const vec4<N>>(), ctx->vel4[s].as<vec4<N>>(), ctx->type[s].as<const uint8_t>(),
                     ctx->wells.as<const N>(), ctx->pstar[s].as<vec4<N>>(), ctx->key[s].as<uint32_t>(),
                     ctx->count.as<uint32_t>(), ctx->cellSlot.as<uint32_t>());
  LAUNCH_CHECK(ctx);
  ctx->st.predicted(c.tableN, /*ahead=*/false);
  return PBF_OK;
}

bool row_mode(const pbf_ctx *ctx);

// list of the non-empty 4 x 4 x 4 bricks for the persistent brick kernels (k_diffuse_bricks, pbf_tiles.hpp): built by the sort
// stage when one of them is going to run (its counter word is zero then), otherwise by whoever turns out to need it
void brick_list(pbf_ctx *ctx, uint32_t tableN, bool counterIsZero = false) {
  if (ctx->st.bricksValid) return;
  if (!counterIsZero) (void)hipMemsetAsync(ctx->brickCtl.p, 0, 4, ctx->stream);
  const uint32_t home = Brick<kBrickZ>::HOME, nBricks = (tableN + home - 1) / home;
  hipLaunchKernelGGL(k_brick_list, grid_for(nBricks), dim3(BLOCK), 0, ctx->stream, ctx->table.as<const uint32_t>(), tableN, home,
                     nBricks, ctx->bricks.as<uint32_t>(), ctx->brickCtl.as<uint32_t>());
  ctx->st.bricks_listed();
}

// one to two exclusive scans in three launches (k_scan_sums zeroes `nZero` control words on its way)
void launch_scans(pbf_ctx *ctx, const ScanJobs &jobs, int njobs, uint32_t *zero = nullptr, uint32_t nZero = 0) {
  const uint32_t blocks = jobs.nb[0] + (njobs > 1 ? jobs.nb[1] : 0u);
  hipLaunchKernelGGL(k_scan_block_sums, dim3(blocks), dim3(BLOCK), 0, ctx->stream, jobs);
  hipLaunchKernelGGL(k_scan_sums, dim3(uint32_t(njobs)), dim3(BLOCK), 0, ctx->stream, jobs, zero, nZero);
  hipLaunchKernelGGL(k_scan_apply, dim3(blocks), dim3(BLOCK), 0, ctx->stream, jobs);
}
ScanJobs scan_job(const uint32_t *count, uint32_t len, uint32_t *sums, uint32_t *table) {
  ScanJobs j{};
  j.count[0] = count, j.sums[0] = sums, j.table[0] = table, j.len[0] = len, j.nb[0] = (len + SCAN_TILE - 1) / SCAN_TILE;
  return j;
}

int ensure_reaction(pbf_ctx *ctx);
template <typename N> int stage_sort(pbf_ctx *ctx, const pbf_params *p) {
  // the scatter consumes the histogram k_predict built (it stores the buckets back to zero, and the slots in cellSlot belong
  // to that histogram): never run it twice
  if (!ctx->st.counted) return fail(ctx, PBF_ERR_STATE, "pbf_stage_sort needs pbf_stage_predict first");
  StepConsts<N> c;
  if (int rc = make_consts<N>(ctx, p, c)) return rc;
  if (c.tableN != ctx->st.countedTableN) return fail(ctx, PBF_ERR_STATE, "bounds changed between predict and sort");
  StageTimer t(ctx, ST_SORT);
  const uint32_t len = c.tableN + 2;
  uint32_t *count = ctx->count.as<uint32_t>(), *table = ctx->table.as<uint32_t>(),
           *sums = ctx->blockSums.as<uint32_t>();
  ScanJobs jobs = scan_job(count, len, sums, table);
  int njobs = 1;
  const int s = ctx->st.cur, d = 1 - s;
  uint32_t *ctl = ctx->brickCtl.as<uint32_t>();
  // option "row_major": the box cells' populations in cell-row-major order and their scan (the row table), read off the
  // Morton table; k_rank_move below then writes the iterations' row-major copy on its way
  RowArrays<N> row{};
  const bool rows = row_mode(ctx), rowDiffuse = rows && ctx->cellDiffuse && ctx->rowDiffuse > 0;
  if (rows) {
    // the cube that holds every cell the Morton table knows: P = 2^(bits of tableN / 3, rounded up)
    uint32_t pshift = 1;
    while (pshift < 10 && (uint64_t(1) << (3 * pshift)) < uint64_t(c.tableN)) ++pshift;
    const size_t ncells = size_t(1) << (3 * pshift), llen = ncells + 1;
    const uint32_t lnb = uint32_t((llen + SCAN_TILE - 1) / SCAN_TILE);
    const size_t v = sizeof(vec4<N>);
    if (int rc = ensure(ctx, ctx->linTable, (ncells + 2 + SCAN_TILE) * 4)) return rc;
    if (int rc = ensure(ctx, ctx->linSums, (size_t(lnb) + 2) * 4)) return rc;
    for (int k = 0; k < 2; ++k)
      if (int rc = ensure(ctx, ctx->rowPstar[k], ctx->cap * v)) return rc;
    if (int rc = ensure(ctx, ctx->rowMass, ctx->cap * sizeof(N))) return rc;
    if (int rc = ensure(ctx, ctx->rowQpos, (ctx->cap + QPOS_PAD) * 8)) return rc;
    if (int rc = ensure(ctx, ctx->rowXYZ, ctx->cap * 4)) return rc;
    if (int rc = ensure(ctx, ctx->rowType, ctx->cap)) return rc;
    if (int rc = ensure(ctx, ctx->rowSlotOf, ctx->cap * 4)) return rc;
    const uint32_t segShift = std::min<uint32_t>(pshift, 6u);  // segments of 64 x cells (the whole row in a smaller cube)
    const size_t nSegTotal = ncells >> segShift;
    if (rowDiffuse) {
      if (int rc = ensure(ctx, ctx->rowCol, ctx->cap * v)) return rc;
      if (int rc = ensure(ctx, ctx->rowMortonOf, ctx->cap * 4)) return rc;
      if (int rc = ensure(ctx, ctx->rowSegs, (std::min(nSegTotal, ctx->cap) + 1) * 4)) return rc;
    }
    // the row table's scan has no input array: it gathers the cells' populations from the histogram itself (row_populations),
    // in the launches of the Morton table's scan
    jobs.count[1] = nullptr, jobs.rowShift = pshift, jobs.tableN = c.tableN;
    jobs.sums[1] = ctx->linSums.as<uint32_t>(), jobs.table[1] = ctx->linTable.as<uint32_t>();
    jobs.len[1] = uint32_t(llen), jobs.nb[1] = lnb;
    njobs = 2;
    if (rowDiffuse)  // the apply pass lists the x-segments that hold a particle (at most one per particle), for k_diffuse_rows
      jobs.segs = ctx->rowSegs.as<uint32_t>(), jobs.nSegs = ctl + kTickets + 3, jobs.segShift = segShift;
    // (brickCtl: zeroed once per step, by k_scan_sums on its way — before the apply pass counts segments in it)
    launch_scans(ctx, jobs, njobs, ctl, kCtlWords);
    row = RowArrays<N>{ctx->rowPstar[0].as<vec4<N>>(), ctx->rowMass.as<N>(), ctx->rowQpos.as<uint2>(), ctx->rowXYZ.as<uint32_t>(),
                       ctx->rowType.as<uint8_t>(), ctx->rowSlotOf.as<uint32_t>(),
                       rowDiffuse ? ctx->rowCol.as<vec4<N>>() : nullptr, rowDiffuse ? ctx->rowMortonOf.as<uint32_t>() : nullptr,
                       ctx->linTable.as<const uint32_t>(), ctl + kTickets + 2, pshift};
    ctx->rowShift = pshift, ctx->rowSegShift = segShift;
  }
  if (njobs == 1) launch_scans(ctx, jobs, 1, ctl, kCtlWords);  // (Morton order only)
  uint32_t *nBig = ctl + kTickets + 1;
  if (int rc = ensure(ctx, ctx->bigCells, (ctx->cap / BIG_CELL + 2) * 4)) return rc;
  hipLaunchKernelGGL(k_scatter_slots, grid_for(ctx->n), dim3(BLOCK), 0, ctx->stream, c.n, c.tableN,
                     ctx->key[s].as<const uint32_t>(), table, ctx->cellSlot.as<const uint32_t>(), count,
                     ctx->permTmp.as<uint32_t>(),
                     ctx->bigCells.as<uint32_t>(), nBig);
  // pile-ups only: cells with more than BIG_CELL members get their segment sorted (exits at once when there are none)
  hipLaunchKernelGGL(k_sort_big_cells, dim3(64), dim3(BLOCK), 0, ctx->stream, table, c.tableN,
                     ctx->bigCells.as<const uint32_t>(), nBig, ctx->permTmp.as<uint32_t>(),
                     ctx->key[s].as<const uint32_t>());
  // pbf_slab_step: the arrays still hold the slots of the particles that left (DEAD_KEY: skipped by the scatter); only
  // the live ones arrive in the sorted set
  const size_t nLive = ctx->slabStepMode ? ctx->sortLive : ctx->n;
  hipLaunchKernelGGL((k_rank_move<N>), grid_for(nLive), dim3(BLOCK), 0, ctx->stream, c, uint32_t(nLive), c.tableN,
                     ctx->permTmp.as<const uint32_t>(), table, arrays<N>(ctx, s, s), arrays<N>(ctx, d, d),
                     ctx->slabActive ? ctx->slotOf.as<uint32_t>() : nullptr, ctx->qpos.as<uint2>(), row);
  LAUNCH_CHECK(ctx);
  ctx->n = nLive;
  ctx->gatherSeq = 0;  // (fresh tickets)
  ctx->st.sorted_now(rows, rowDiffuse);
  ctx->orderEpoch++;  // (a new order: what the observers left describes the old one)
  if (ctx->col.reaction) {  // the reaction records are indexed by the order just established: cleared once per step, here
    if (int rc = ensure_reaction(ctx)) return rc;  // (allocates only if the capacity grew without an upload)
    const uint32_t n2 = 2u * uint32_t(ctx->n);
    hipLaunchKernelGGL((k_push_clear<N>), grid_for(std::max<size_t>(n2, 1)), dim3(BLOCK), 0, ctx->stream, n2, ctx->pushRec.as<vec4<N>>(),
                       ctx->pushCtl.as<unsigned long long>());
    LAUNCH_CHECK(ctx);
    ctx->col.records_cleared(ctx->orderEpoch);
  }
  if (!rowDiffuse) brick_list(ctx, c.tableN, /*counterIsZero=*/true);  // (the row-major diffusion has its own segments)
  return PBF_OK;
}

// the Jacobi partner of pstar[pcur]: any of the three buffers that is neither live nor needed
inline int other_pstar(const pbf_ctx *ctx) { return ctx->st.pcur == 2 ? ctx->st.cur : 2; }

// Launch one gather stage.  gatherKind picks the kernel (option "gather" / env PBF_GATHER);
// PBF_FLAG_NO_LDS always forces the plain per-particle global walk.
enum GatherMode { GATHER_PLAIN = 0, GATHER_SAVE_LISTS = 1, GATHER_FROM_LISTS = 2 };

// Row-major iterations apply to the default configuration only (neighbour lists, lambda riding on the build, one lane per
// particle, eager launches); everything else keeps the Morton walk.
// The last condition is the PRECONDITION of the row kernels' 32-bit candidate offsets (load_at(), pbf_kernels.hpp): every row
// slot a list can name, times the bytes of a candidate, fits 32 bits.  A list names slots below the count its build ran
// with.  That is ctx->n as stage_lambda sees it — which evaluates this function itself, after the sort has set the live
// count, in a slab step the one after assembly — and the sort stage's own evaluation, with the pre-sort count (dead slots
// included, never less than the live one), only decides whether the copy is written.  The delta-p launches do not come
// through here: row_offsets_fit() holds them to the same bound.
bool row_offsets_fit(const pbf_ctx *ctx) { return uint64_t(ctx->n) * (ctx->fp64 ? sizeof(vec4<double>) : sizeof(vec4<float>)) <= ROW_BYTES_MAX; }
bool row_mode(const pbf_ctx *ctx) {
  return ctx->rowMajor > 0 && ctx->gatherKind == 1 && ctx->splitBuild == 8 && ctx->coop == 0 && ctx->reuseLists &&
         !ctx->fuseDiffuse && ctx->graphMode <= 0 &&
         !(ctx->desc.flags & PBF_FLAG_NO_LDS) && row_offsets_fit(ctx);
}
template <typename N> RowWalk row_walk(pbf_ctx *ctx) {
  return RowWalk{ctx->linTable.as<const uint32_t>(), ctx->rowXYZ.as<const uint32_t>(), ctx->rowSlotOf.as<const uint32_t>(),
                 ctx->table.as<const uint32_t>(), ctx->tableN, ctx->rowShift};
}
// whoever wants {pStar, lambda} in the Morton-sorted array (stage-level read-backs, the extras, the surface) gets it here
template <typename N> int materialise_pstar(pbf_ctx *ctx) {
  if (!ctx->st.pstarInRows) return PBF_OK;
  hipLaunchKernelGGL((k_rows_to_morton<N>), grid_for(ctx->n), dim3(BLOCK), 0, ctx->stream, uint32_t(ctx->n),
                     ctx->rowPstar[ctx->st.rcur].as<const vec4<N>>(), ctx->rowSlotOf.as<const uint32_t>(),
                     ctx->pstar[ctx->st.pcur].as<vec4<N>>());
  LAUNCH_CHECK(ctx);
  ctx->st.materialised();
  return PBF_OK;
}

// A zeroed word of brickCtl (the sort stage zeroes them all once per step) for ONE launch: the work ticket of a persistent
// tile kernel, or the chunk allocator of a list build.  More launches than words since the last sort: re-arm.
uint32_t *next_ticket(pbf_ctx *ctx) {
  uint32_t *ctl = ctx->brickCtl.as<uint32_t>();
  if (ctx->gatherSeq >= kTickets) {
    (void)hipMemsetAsync(ctl + 1, 0, kTickets * 4, ctx->stream);
    ctx->gatherSeq = 0;
  }
  return ctl + 1 + ctx->gatherSeq++;
}
// build = this launch WRITES the lists (takes a fresh chunk allocator)
NbrLists nbr_lists(pbf_ctx *ctx, bool build) {
  return NbrLists{ctx->nbrList.as<uint32_t>(), ctx->nbrCount.as<uint32_t>(), build ? next_ticket(ctx) : nullptr,
                  ctx->nbrExtraAt, ctx->nbrChunks};
}

// A launch with more than the default dynamic LDS needs the kernel's limit raised first.  The high-water mark is this
// context's own: the attribute belongs to the device the context runs on, and contexts of other devices or threads raise it
// themselves.
int raise_lds_limit(pbf_ctx *ctx, const void *kernel, size_t lds) {
  size_t &mark = ctx->ldsLimit[kernel];
  if (lds <= mark) return PBF_OK;
  HIPCHK(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
  mark = lds;
  return PBF_OK;
}

// the quantised copy of pStar, made here only after a stage that moved pStar without refreshing it
template <typename N> uint2 *ensure_qpos(pbf_ctx *ctx, const StepConsts<N> &c, const vec4<N> *pstar) {
  uint2 *qp = ctx->qpos.as<uint2>();
  if (!ctx->st.qposValid) {
    hipLaunchKernelGGL((k_quantise<N>), grid_for(ctx->n), dim3(BLOCK), 0, ctx->stream, c, pstar, qp);
    ctx->st.quantised();
  }
  return qp;
}

// the list-driven reader, one lane per particle (ROWS: on the row-major copy)
// (option "pipeline", auto = off: with round 3's trimmed fp64 sqrt / divides the plain reader wins in fp64 too — 2.05 vs
// 2.10 ms per step at 1 M; in round 2, on the compiler's IEEE forms, the pipelined one had been 1.3 % ahead there)
template <typename N, typename Op, bool ROWS>
void launch_from_lists(pbf_ctx *ctx, const StepConsts<N> &c, const typename Op::Args &args, const uint32_t *key,
                       const uint32_t *table, const RowWalk &rw = {}) {
  const dim3 g = grid_for(ctx->n), b(BLOCK);
  const NbrLists ls = nbr_lists(ctx, false);
  if (ctx->pipeline > 0) {
    hipLaunchKernelGGL((k_gather_from_lists<N, Op, true, ROWS>), g, b, 0, ctx->stream, c, args, key, table, ls, rw);
    return;
  }
  if constexpr (ROWS) {  // the plain reader on the row-major copy: at the width option "reader_wg" asks for
    switch (iter_wg(ctx->readerWg, kIterWgReader)) {
      case 64: hipLaunchKernelGGL((k_gather_from_lists<N, Op, false, true, 64>), iter_grid(ctx->n, 64), dim3(64), 0, ctx->stream, c, args, key, table, ls, rw); return;
      case 128: hipLaunchKernelGGL((k_gather_from_lists<N, Op, false, true, 128>), iter_grid(ctx->n, 128), dim3(128), 0, ctx->stream, c, args, key, table, ls, rw); return;
      default: break;
    }
  }
  hipLaunchKernelGGL((k_gather_from_lists<N, Op, false, ROWS>), g, b, 0, ctx->stream, c, args, key, table, ls, rw);
}

// the list build on the Morton-sorted arrays with `Ride` riding on it: W pair loads per trip, staging depth LMAX, FW survivors
// per drain trip
template <typename N, typename Ride, int W, int LMAX, int FW>
void launch_build_lists(pbf_ctx *ctx, const StepConsts<N> &c, const typename Ride::Args &ride, const vec4<N> *pstar,
                        const uint2 *qp, const uint8_t *type, const uint32_t *key, const uint32_t *table) {
  hipLaunchKernelGGL((k_build_lists_op<N, Ride, W, LMAX, FW>), grid_for(ctx->n), dim3(BLOCK), 0, ctx->stream, c, ride, pstar, qp,
                     type, key, table, nbr_lists(ctx, true));
}

template <typename N, typename Op>
int launch_gather(pbf_ctx *ctx, const StepConsts<N> &c, typename Op::Args args, GatherMode mode = GATHER_PLAIN) {
  const uint32_t *key = ctx->key[ctx->st.cur].as<const uint32_t>();
  const uint32_t *table = ctx->table.as<const uint32_t>();
  if ((ctx->desc.flags & PBF_FLAG_NO_LDS) || ctx->gatherKind == 0) {
    // `padLds` bytes of unused dynamic LDS cap the workgroups per CU: fewer resident waves keep the
    // 32 KiB L1 from thrashing on the gather's working set (each wave touches ~9 cache lines per load)
    hipLaunchKernelGGL((k_gather_global<N, Op>), grid_for(ctx->n), dim3(BLOCK), ctx->padLds, ctx->stream, c, args, key,
                       table);
    LAUNCH_CHECK(ctx);
    return PBF_OK;
  }
  if constexpr (Op::kTileable && Op::kFilter) {
    // gather = 3: the solver iteration per brick out of LDS tiles (pbf_tiles.hpp); everything else it does not cover
    // (diffuse, the opt-in extras) takes the list path below
    if (ctx->gatherKind == 3 && mode != GATHER_PLAIN && uint64_t(ctx->n) * sizeof(typename Op::Src) <= 0xFFFFFFFFull) {
      using B = TileBrick;
      static_assert(kBrickZ == TILE_BZ, "the sort stage's brick list is the tile kernels' one");
      brick_list(ctx, c.tableN);
      constexpr int WAYS = 4, LMAX = 16;
      uint32_t cap = ctx->tileCap ? std::min(ctx->tileCap, 65535u) : 2048u;  // list entries of a tiled brick are tile slots
      uint32_t *nl = ctx->nbrList.as<uint32_t>(), *nc = ctx->nbrCount.as<uint32_t>();
      uint32_t *ctl = ctx->brickCtl.as<uint32_t>();
      auto ticket = [&]() -> uint32_t * { return next_ticket(ctx); };
      auto grid_of = [&](size_t lds) {
        const uint32_t perCU = uint32_t(std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / (lds + 512))));
        return dim3(uint32_t(ctx->numCUs) * perCU);
      };
      if (mode == GATHER_SAVE_LISTS) {
        const uint2 *qp = ensure_qpos<N>(ctx, c, Op::src(args));
        StageTimer tb(ctx, ST_BUILD);
        const size_t lds = B::HDR2 + size_t(cap + WAYS) * sizeof(uint2) + size_t(LMAX + WAYS) * TILE_THREADS * 2;
        if (lds > 160 * 1024 - 64) return fail(ctx, PBF_ERR_INVALID, "tile cap exceeds the CU's 160 KiB LDS");
        auto kernel = k_tile_build<N, WAYS, LMAX>;
        if (int rc = raise_lds_limit(ctx, reinterpret_cast<const void *>(kernel), lds)) return rc;
        hipLaunchKernelGGL(kernel, grid_of(lds), dim3(TILE_THREADS), lds, ctx->stream, c, Op::src(args), qp, args.type, key, table,
                           ctx->bricks.as<const uint32_t>(), ctl, ticket(), cap, nl, nc);
      }
      const size_t lds = B::HDR2 + size_t(cap) * sizeof(typename Op::Src);
      if (lds > 160 * 1024 - 64) return fail(ctx, PBF_ERR_INVALID, "tile cap exceeds the CU's 160 KiB LDS");
      auto kernel = k_tile_from_lists<N, Op>;
      if (int rc = raise_lds_limit(ctx, reinterpret_cast<const void *>(kernel), lds)) return rc;
      hipLaunchKernelGGL(kernel, grid_of(lds), dim3(TILE_THREADS), lds, ctx->stream, c, args, key, table,
                         ctx->bricks.as<const uint32_t>(), ctl, ticket(), cap, nl, nc);
      LAUNCH_CHECK(ctx);
      return PBF_OK;
    }
  }
  if (ctx->gatherKind == 1 || ctx->gatherKind == 3) {
    const dim3 g = grid_for(ctx->n), b(BLOCK);
    auto from_lists = [&]() {  // the list-driven reader: one lane per particle, or (option "coop") a lane group per particle
      if constexpr (Op::kTileable && Op::kFilter) {
        const NbrLists ls = nbr_lists(ctx, false);
        auto coop_grid = [&](int k) { return dim3(unsigned(std::max<size_t>(1, (ctx->n * k + BLOCK - 1) / BLOCK))); };
        switch (ctx->coop) {
          case 2: hipLaunchKernelGGL((k_gather_from_lists_coop<N, Op, 2>), coop_grid(2), b, 0, ctx->stream, c, args, key, table, ls); return;
          case 4: hipLaunchKernelGGL((k_gather_from_lists_coop<N, Op, 4>), coop_grid(4), b, 0, ctx->stream, c, args, key, table, ls); return;
          case 8: hipLaunchKernelGGL((k_gather_from_lists_coop<N, Op, 8>), coop_grid(8), b, 0, ctx->stream, c, args, key, table, ls); return;
          default: break;
        }
      }
      launch_from_lists<N, Op, false>(ctx, c, args, key, table);
    };
    if (mode == GATHER_FROM_LISTS) {
      from_lists();
    } else if (mode == GATHER_SAVE_LISTS && ctx->splitBuild &&
               uint64_t(ctx->n) * sizeof(typename Op::Src) <= 0xFFFFFFFFull) {  // (k_build_lists_op: 32-bit offsets)
      // One build kernel; split_build says what rides on it.  8: the op itself — nothing is left to run list-driven.
      // 4 / 5: nothing (ListOnlyOp), with 2 / 4 pair loads per trip — the op then runs list-driven.
      if constexpr (Op::kTileable && Op::kFilter) {  // (the ops that filter on pStar itself: lambda, delta-p)
        const vec4<N> *ps = Op::src(args);
        const uint2 *qp = ensure_qpos<N>(ctx, c, ps);
        if (ctx->splitBuild == 8) {
          // (staging depth 32 and four survivors per drain trip: measured best of 16 / 24 / 32 x 2 / 4 / 6 / 8)
#ifndef PBF_BUILD_LMAX
#define PBF_BUILD_LMAX 32
#endif
          launch_build_lists<N, Op, 4, PBF_BUILD_LMAX, 4>(ctx, c, args, ps, qp, args.type, key, table);
          LAUNCH_CHECK(ctx);
          return PBF_OK;
        }
        // survivors per drain trip of a build that only stores them
#ifndef PBF_LISTONLY_FW
#define PBF_LISTONLY_FW 1
#endif
        using Lists = ListOnlyOp<N>;
        constexpr int FW = PBF_LISTONLY_FW;
        const typename Lists::Args only{args.type};
        StageTimer tb(ctx, ST_BUILD);
        if (ctx->splitBuild == 4)
          launch_build_lists<N, Lists, 2, 16, FW>(ctx, c, only, ps, qp, args.type, key, table);
        else  // staging depth (option "list_max", default 32: one flush for most particles beats the two more workgroups per CU that 16 leaves room for: -2 % per step)
          switch (ctx->listMax ? ctx->listMax : 32u) {
            case 16: launch_build_lists<N, Lists, 4, 16, FW>(ctx, c, only, ps, qp, args.type, key, table); break;
            case 24: launch_build_lists<N, Lists, 4, 24, FW>(ctx, c, only, ps, qp, args.type, key, table); break;
            default: launch_build_lists<N, Lists, 4, 32, FW>(ctx, c, only, ps, qp, args.type, key, table); break;
          }
      }
      from_lists();
    } else if (mode == GATHER_SAVE_LISTS) {
      hipLaunchKernelGGL((k_gather_lists<N, Op, 16, true>), g, b, 0, ctx->stream, c, args, key, table, nbr_lists(ctx, true));
    } else {
      switch (ctx->listMax ? ctx->listMax : 16u) {
        case 12: hipLaunchKernelGGL((k_gather_lists<N, Op, 12>), g, b, 0, ctx->stream, c, args, key, table, nbr_lists(ctx, false)); break;
        case 24: hipLaunchKernelGGL((k_gather_lists<N, Op, 24>), g, b, 0, ctx->stream, c, args, key, table, nbr_lists(ctx, false)); break;
        case 32: hipLaunchKernelGGL((k_gather_lists<N, Op, 32>), g, b, 0, ctx->stream, c, args, key, table, nbr_lists(ctx, false)); break;
        default: hipLaunchKernelGGL((k_gather_lists<N, Op, 16>), g, b, 0, ctx->stream, c, args, key, table, nbr_lists(ctx, false)); break;
      }
    }
    LAUNCH_CHECK(ctx);
    return PBF_OK;
  }
  return fail(ctx, PBF_ERR_INVALID, "unknown gather kind");
}

// The overlapped diffusion must be done before anything rewrites what it reads (colours, types, keys, table, brick
// list: the next sort) or reads what it writes (colours: download, surface).  Stream-side wait, no host sync.
int join_diffuse(pbf_ctx *ctx) {
  if (!ctx->diffusePending) return PBF_OK;
  ctx->diffusePending = false;
  HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->evJoin, 0));
  return PBF_OK;
}

template <typename N> int stage_diffuse(pbf_ctx *ctx, const pbf_params *p, bool overlap = false) {
  StepConsts<N> c;
  if (int rc = make_consts<N>(ctx, p, c)) return rc;
  const int s = ctx->st.cur, d = 1 - s;  // col4[d] is free after the sort
  typename DiffuseOp<N>::Args args{ctx->col4[s].as<const vec4<N>>(), ctx->col4[d].as<vec4<N>>(),
                                   ctx->type[s].as<const uint8_t>()};
  const bool timed = (ctx->desc.flags & PBF_FLAG_STAGE_TIMING) != 0 && ((ctx->timingMask >> ST_DIFFUSE) & 1u) != 0;
  // beside the solver iterations only where that pays: at 1 M particles -2.2 % per step, at 256 K +1.4 % (the side stream's
  // one-workgroup-per-CU launch is then longer than the iteration it hides behind) — measured, profiles/r03_matrix.txt
  overlap = overlap && ctx->overlapDiffuse && ctx->cellDiffuse && !(ctx->desc.flags & PBF_FLAG_NO_LDS) && !timed &&
            (ctx->overlapDiffuseForced || ctx->n >= (size_t(1) << 19));
  bool parked = false;  // the per-cell sums went through pStar's idle Jacobi partner and the list lengths
  StageTimer t(ctx, ST_DIFFUSE);
  if (ctx->cellDiffuse && ctx->st.diffuse_on_rows() && ctx->rowDiffuse) {
    // the row-major copy: one wave per segment of 64 x cells, runs staged through LDS, sums applied in place (k_diffuse_rows).
    // On the solver's own stream: the launch is short, nothing is gained by hiding it
    // records of one row's run in the LDS tile (66 cells; the settled dam-break's are ~460): a longer run walks from memory.
    // A small tile matters more than a roomy one: 13 single-wave workgroups per CU at 640 records (fp32), and the launch time
    // is inversely proportional to that number (measured: 1 024 records 68 us, 768 61 us, 640 51 us, 576 51 us)
    const uint32_t cap = ctx->diffuseCap ? ctx->diffuseCap : 640u;
    const size_t lds = size_t(cap + 8) * sizeof(vec4<N>) + size_t(DIFFUSE_ROW_THREADS) * (4 * sizeof(N) + 4) + cap + 8;  // (+ 8 records / types: the fold reads ahead)
    if (int rc = raise_lds_limit(ctx, reinterpret_cast<const void *>(k_diffuse_rows<N>), lds)) return rc;
    const uint32_t perCU = uint32_t(std::max<size_t>(1, std::min<size_t>(16, (160 * 1024) / (lds + 256))));
    const uint32_t blocks = std::max(8u, (uint32_t(ctx->numCUs) * perCU) & ~7u);  // (the kernel deals segments per XCD: a multiple of 8)
    hipLaunchKernelGGL((k_diffuse_rows<N>), dim3(blocks), dim3(DIFFUSE_ROW_THREADS), lds, ctx->stream, c,
                       row_walk<N>(ctx), ctx->rowCol.as<const vec4<N>>(), ctx->rowType.as<const uint8_t>(),
                       ctx->rowMortonOf.as<const uint32_t>(), ctx->rowSegs.as<const uint32_t>(),
                       ctx->brickCtl.as<const uint32_t>() + kTickets + 3, ctx->rowSegShift, args.colOut, cap, uint32_t(ctx->n));
    LAUNCH_CHECK(ctx);
  } else if (ctx->cellDiffuse && !(ctx->desc.flags & PBF_FLAG_NO_LDS)) {
    brick_list(ctx, c.tableN);
    // sums per cell, parked in buffers that are idle here (the Jacobi partner of pStar and the list lengths) — or, when
    // the stage runs beside the solver iterations, in scratch of its own
    vec4<N> *cellSum = ctx->pstar[other_pstar(ctx)].as<vec4<N>>();
    uint32_t *cellCnt = ctx->nbrCount.as<uint32_t>();
    hipStream_t st = ctx->stream;
    // records in the LDS tile: 48 KiB (fp32) / 96 KiB (fp64) of colours.  (Round 2 gave fp64 the same BYTES, i.e. half the
    // records — below the p99 of the settled dam-break's halos, 1 800: a third of the bricks fell back to the per-cell
    // global walk and the fp64 diffusion took 0.43 ms against fp32's 0.13.)
    uint32_t cap = 3072u;
    // beside the solver iterations: a 32-KiB tile (fp32) leaves room for THREE of the list build's 40-KiB workgroups on
    // the CU instead of two (measured: step -2.6 %; p99 of the settled dam-break's halos is 1 800 records, a fuller
    // brick walks globally)
    if (overlap) cap = 2048u;  // (fp64: 64 KiB + two of the build's 40-KiB workgroups)
    const size_t lds = Brick<4>::HDR + size_t(cap) * sizeof(vec4<N>);
    uint32_t perCU = uint32_t((160 * 1024) / (lds + 1024));
    if (overlap) {
      if (int rc = ensure(ctx, ctx->diffSum, ctx->cap * sizeof(vec4<N>))) return rc;
      if (int rc = ensure(ctx, ctx->diffCnt, ctx->cap * 4)) return rc;
      if (!ctx->sideStream) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->sideStream, hipStreamNonBlocking));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->evFork, hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->evJoin, hipEventDisableTiming));
      }
      cellSum = ctx->diffSum.as<vec4<N>>(), cellCnt = ctx->diffCnt.as<uint32_t>();
      st = ctx->sideStream;
      perCU = 1;  // one 48-KiB workgroup per CU: the list build's staging lists (24 KiB per workgroup) keep their room
      HIPCHK(ctx, hipEventRecord(ctx->evFork, ctx->stream));
      HIPCHK(ctx, hipStreamWaitEvent(st, ctx->evFork, 0));
    }
    const uint32_t *key = ctx->key[s].as<const uint32_t>(), *table = ctx->table.as<const uint32_t>();
    static_assert(kBrickZ == 4, "the sort stage's brick list is the 4 x 4 x 4 one");
    hipLaunchKernelGGL((k_diffuse_bricks<N>), dim3(uint32_t(ctx->numCUs) * perCU), dim3(DIFFUSE_BRICK_THREADS), lds,
                       st, c, args.colIn, args.type, table, ctx->bricks.as<const uint32_t>(),
                       ctx->brickCtl.as<const uint32_t>(), cellSum, cellCnt, cap);
    hipLaunchKernelGGL((k_diffuse_apply<N>), grid_for(ctx->n), dim3(BLOCK), 0, st, c, args, key, table,
                       cellSum, cellCnt);
    LAUNCH_CHECK(ctx);
    if (overlap) {
      HIPCHK(ctx, hipEventRecord(ctx->evJoin, st));
      ctx->diffusePending = true;
    }
    parked = !overlap;
  } else if (int rc = launch_gather<N, DiffuseOp<N>>(ctx, c, args)) {
    return rc;
  }
  std::swap(ctx->col4[s], ctx->col4[d]);
  ctx->st.diffused(parked);
  return PBF_OK;
}

// the row build's shape: pair loads per trip, staging depth, survivors per drain trip (A/B builds override these)
#ifndef PBF_ROWS_W
#define PBF_ROWS_W 4
#endif
#ifndef PBF_ROWS_LMAX
#define PBF_ROWS_LMAX 32
#endif
#ifndef PBF_ROWS_FW
#define PBF_ROWS_FW 4
#endif
// fuseDiffuse (pbf_step, option "fuse_diffuse"): the colour diffusion rides on this launch's walk
template <typename N, bool FAST> int lambda_impl(pbf_ctx *ctx, const pbf_params *p, bool fuseDiffuse) {
  using Op = LambdaOp<N, FAST>;
  StepConsts<N> c;
  if (int rc = make_consts<N>(ctx, p, c)) return rc;
  StageTimer t(ctx, ST_LAMBDA);
  const int s = ctx->st.cur;
  // the survivors of lambda's filter are exactly delta's (same pStar): hand them over through HBM
  const bool lists = (ctx->gatherKind == 1 || ctx->gatherKind == 3) && ctx->reuseLists && !(ctx->desc.flags & PBF_FLAG_NO_LDS);
  if (lists && ctx->st.rows_usable() && row_mode(ctx) && !fuseDiffuse) {  // the build + lambda on the row-major copy
    typename Op::Args a{ctx->rowPstar[ctx->st.rcur].as<vec4<N>>(), nullptr, ctx->rowType.as<const uint8_t>(), ctx->rowMass.as<const N>()};
    const uint2 *qp = ctx->rowQpos.as<const uint2>();
    const RowWalk rw = row_walk<N>(ctx);
    const NbrLists ls = nbr_lists(ctx, true);
    switch (iter_wg(ctx->buildWg, kIterWgBuild)) {  // (option "build_wg": one workgroup per unit of that many lanes)
      case 64: hipLaunchKernelGGL((k_build_rows_op<N, Op, PBF_ROWS_W, PBF_ROWS_LMAX, PBF_ROWS_FW, 64>), iter_grid(ctx->n, 64), dim3(64), 0, ctx->stream, c, a, qp, rw, ls); break;
      case 128: hipLaunchKernelGGL((k_build_rows_op<N, Op, PBF_ROWS_W, PBF_ROWS_LMAX, PBF_ROWS_FW, 128>), iter_grid(ctx->n, 128), dim3(128), 0, ctx->stream, c, a, qp, rw, ls); break;
      default: hipLaunchKernelGGL((k_build_rows_op<N, Op, PBF_ROWS_W, PBF_ROWS_LMAX, PBF_ROWS_FW>), grid_for(ctx->n), dim3(BLOCK), 0, ctx->stream, c, a, qp, rw, ls); break;
    }
    LAUNCH_CHECK(ctx);
    ctx->st.lambda_done(lists, /*rows=*/true);
    return PBF_OK;
  }
  if (int rc = materialise_pstar<N>(ctx)) return rc;  // (a Morton-path launch after row-major ones: options changed mid-step)
  ctx->st.lambda_done(lists, /*rows=*/false);
  typename Op::Args a{ctx->pstar[ctx->st.pcur].as<vec4<N>>(), ctx->pos4[s].as<const vec4<N>>(), ctx->type[s].as<const uint8_t>()};
  if (!lists || !fuseDiffuse) return launch_gather<N, Op>(ctx, c, a, lists ? GATHER_SAVE_LISTS : GATHER_PLAIN);
  const int d = 1 - s;
  typename DiffuseOp<N>::Args xa{ctx->col4[s].as<const vec4<N>>(), ctx->col4[d].as<vec4<N>>(),
                                 ctx->type[s].as<const uint8_t>()};
  hipLaunchKernelGGL((k_gather_lists<N, Op, 16, true, DiffuseOp<N>>), grid_for(ctx->n), dim3(BLOCK), 0, ctx->stream, c, a,
                     ctx->key[s].as<const uint32_t>(), ctx->table.as<const uint32_t>(), nbr_lists(ctx, true), xa);
  LAUNCH_CHECK(ctx);
  std::swap(ctx->col4[s], ctx->col4[d]);
  ctx->st.diffused(/*parked=*/false);
  return PBF_OK;
}
template <typename N> int stage_lambda(pbf_ctx *ctx, const pbf_params *p, bool fuseDiffuse = false) {
  return DISPATCH_FAST(ctx, lambda_impl, ctx, p, fuseDiffuse);
}

// which solids are installed (ColliderState's flags: solid_install keeps each in step with its SolidLattice::present())
bool collider_on(const pbf_ctx *ctx) { return ctx->col.lattice; }
bool scenery_on(const pbf_ctx *ctx) { return ctx->col.scenery; }
static_assert(int(ColliderState::DELTA_OFF) == COLLIDE_OFF && int(ColliderState::DELTA_STATIC) == COLLIDE_STATIC &&
                  int(ColliderState::DELTA_POSED) == COLLIDE_POSED && int(ColliderState::DELTA_REACT) == COLLIDE_REACT &&
                  int(ColliderState::DELTA_REACT_SCENERY) == COLLIDE_REACT_SCENERY,
              "ColliderState::delta_mode() names pbf_kernels.hpp's ColliderMode");
// the reaction records of the step: whether they describe the arrays as they are, and the slots their readers index them by
bool push_current(const pbf_ctx *ctx) { return ctx->col.records_current(ctx->orderEpoch, ctx->st.sorted); }
const uint32_t *push_slots(const pbf_ctx *ctx) { return ctx->col.records_by_row() ? ctx->rowSlotOf.as<const uint32_t>() : nullptr; }
// a solid's lattice as DeltaOp<.., COLLIDE> and k_collider_sample take it: N(origin), N(1) / N(spacing), N(margin), each
// rounded once from the setting as given (all zero, phi == NULL, without one)
template <typename N> ColliderSdf<N> sdf_args(const SolidLattice<DevBuf> &l) {
  ColliderSdf<N> s{};
  if (!l.present()) return s;
  s.phi = l.phi.as<const N>();
  for (int a = 0; a < 3; ++a) s.dims[a] = l.dims[a], s.origin[a] = N(l.origin[a]);
  s.inv = N(1) / N(l.spacing), s.margin = N(l.margin);
  return s;
}
constexpr const char *kColliderSlabError = "a collider is not supported in slab mode (pbf_set_collider(ctx, NULL) clears it)";
bool slab_ctx(const pbf_ctx *ctx) { return ctx->comm || ctx->slabActive || ctx->slabConfigured; }
int collider_refuse_slab(pbf_ctx *ctx) { return slab_ctx(ctx) ? fail(ctx, PBF_ERR_STATE, kColliderSlabError) : PBF_OK; }
// what the entry points that need a lattice (`who`) refuse alike, after the refusals that are their own: none set, then slab mode
int collider_needed(pbf_ctx *ctx, const char *who) {
  if (!collider_on(ctx)) return fail(ctx, PBF_ERR_STATE, std::string(who) + ": no collider set (pbf_set_collider)");
  return collider_refuse_slab(ctx);
}

template <typename N, bool FAST, int COLLIDE> int delta_run(pbf_ctx *ctx, const pbf_params *p) {
  using Op = DeltaOp<N, FAST, COLLIDE>;
  // (with a collider the lattice follows the stock arguments, and with a pose the pointer to its record follows the lattice)
  auto args = [&](const typename Op::ArgsPlain &plain) {
    if constexpr (COLLIDE == COLLIDE_REACT_SCENERY)  // (the scenery's lattice follows the records)
      return typename Op::Args{{{{plain, sdf_args<N>(ctx->solid[ColliderState::COLLIDER])}, ctx->colliderPose.as<const ColliderPose<N>>()}, ctx->pushRec.as<vec4<N>>()}, sdf_args<N>(ctx->solid[ColliderState::SCENERY])};
    else if constexpr (COLLIDE == COLLIDE_REACT)
      return typename Op::Args{{{plain, sdf_args<N>(ctx->solid[ColliderState::COLLIDER])}, ctx->colliderPose.as<const ColliderPose<N>>()}, ctx->pushRec.as<vec4<N>>()};
    else if constexpr (COLLIDE == COLLIDE_POSED) return typename Op::Args{{plain, sdf_args<N>(ctx->solid[ColliderState::COLLIDER])}, ctx->colliderPose.as<const ColliderPose<N>>()};
    else if constexpr (COLLIDE == COLLIDE_STATIC)  // (a static collider, or scenery without a collider: the same kernels)
      return typename Op::Args{plain, sdf_args<N>(ctx->solid[ctx->col.static_reads_scenery() ? ColliderState::SCENERY : ColliderState::COLLIDER])};
    else return plain;
  };
  StepConsts<N> c;
  if (int rc = make_consts<N>(ctx, p, c)) return rc;
  if constexpr (COLLIDE == COLLIDE_REACT || COLLIDE == COLLIDE_REACT_SCENERY) {  // the records follow the index of the launch: one kind of index per step
    if (!push_current(ctx)) return fail(ctx, PBF_ERR_STATE, "the collider reaction needs a sort since it was enabled");
    if (!ctx->col.delta_indexed(ctx->st.delta_on_rows()))
      return fail(ctx, PBF_ERR_STATE, "the gather path changed between two delta-p launches of a step with the collider reaction on");
  }
  StageTimer t(ctx, ST_DELTA);
  const int s = ctx->st.cur;
  if (ctx->st.delta_on_rows()) {  // list-driven delta-p on the row-major copy
    // (the lists are those of a lambda launch that went through row_mode(); the count has not grown since, or the state would not be here)
    if (!row_offsets_fit(ctx)) return fail(ctx, PBF_ERR_STATE, "the row-major copy has outgrown its 32-bit candidate offsets");
    const int rin = ctx->st.rcur, rout = 1 - rin;
    const uint32_t *key = ctx->key[s].as<const uint32_t>(), *table = ctx->table.as<const uint32_t>();
    const typename Op::Args a = args({ctx->rowPstar[rin].as<const vec4<N>>(), ctx->rowPstar[rout].as<vec4<N>>(), ctx->rowType.as<const uint8_t>(), ctx->rowQpos.as<uint2>()});
    launch_from_lists<N, Op, true>(ctx, c, a, key, table, row_walk<N>(ctx));
    LAUNCH_CHECK(ctx);
    ctx->st.pstar_moved(/*rows=*/true, rout);
    return PBF_OK;
  }
  if (int rc = materialise_pstar<N>(ctx)) return rc;
  const int in = ctx->st.pcur, out = other_pstar(ctx);
  // delta-p's epilogue also writes the quantised copy of the new pStar: the next iteration's list build needs it
  const typename Op::Args a = args({ctx->pstar[in].as<const vec4<N>>(), ctx->pstar[out].as<vec4<N>>(), ctx->type[s].as<const uint8_t>(),
                                    ctx->st.qposValid ? ctx->qpos.as<uint2>() : nullptr});
  const int rc = launch_gather<N, Op>(ctx, c, a, ctx->st.delta_from_lists() ? GATHER_FROM_LISTS : GATHER_PLAIN);
  ctx->st.pstar_moved(/*rows=*/false, rc ? in : out);  // (launched or not: nothing derived from the old pStar is trusted any more)
  return rc;
}
template <typename N, bool FAST> int delta_impl(pbf_ctx *ctx, const pbf_params *p) {
  // the one place that turns the mode into an instantiation.  The cases stand in this order, not the enum's, on purpose: the
  // order of first use fixes the kernels' order in the code object.
  switch (ctx->col.delta_mode()) {
    case ColliderState::DELTA_OFF: return delta_run<N, FAST, COLLIDE_OFF>(ctx, p);
    case ColliderState::DELTA_REACT: return delta_run<N, FAST, COLLIDE_REACT>(ctx, p);
    case ColliderState::DELTA_POSED: return delta_run<N, FAST, COLLIDE_POSED>(ctx, p);
    case ColliderState::DELTA_STATIC: return delta_run<N, FAST, COLLIDE_STATIC>(ctx, p);
    case ColliderState::DELTA_REACT_SCENERY: break;
  }
  return delta_run<N, FAST, COLLIDE_REACT_SCENERY>(ctx, p);
}
template <typename N> int stage_delta(pbf_ctx *ctx, const pbf_params *p) {
  if (collider_on(ctx) || scenery_on(ctx))
    if (int rc = collider_refuse_slab(ctx)) return rc;
  return DISPATCH_FAST(ctx, delta_impl, ctx, p);
}

// Opt-in extras (pbf_params.vorticity / .xsph, pbf_set_surface_tension), absent from the reference: see VorticityOp /
// XsphOp / SurfaceTensionOp.  Off (the default), none of them changes a launch of the step.
bool surface_on(const pbf_ctx *ctx) { return ctx->cohesion > 0 || ctx->adhesion > 0; }
bool extras_on(const pbf_ctx *ctx, const pbf_params *p) { return p->vorticity || p->xsph || surface_on(ctx); }
// its two fields, sized to the particle capacity.  Allocated when the feature is enabled and when an upload grows the
// capacity, so that no step allocates (a step that allocates is never captured into a hipGraph, and one that does so while
// being captured turns graph replay off)
int ensure_surface(pbf_ctx *ctx) {
  const size_t bytes = ctx->cap * (ctx->fp64 ? sizeof(double4) : sizeof(float4));
  if (int rc = ensure(ctx, ctx->surfA, bytes)) return rc;
  return ensure(ctx, ctx->surfB, bytes);
}

// The friction pass's partial records outlive the step (the observer and the next step's body stage fold them), so unlike
// every other buffer they are carried across a grow: the old bytes are copied into the new allocation on the ctx's stream
// before the old one is freed.  (While the stream is being captured the synchronise fails and nothing is replaced: the step
// is then redone eagerly, as after any allocation.)
int ensure_friction_partials(pbf_ctx *ctx) {
  const size_t bytes = (ctx->cap / DIAG_TILE + 2) * sizeof(WrenchPartial);
  DevBuf &b = ctx->frictionPartials;
  if (b.cap >= bytes) return PBF_OK;
  DevBuf fresh;
  if (int rc = ensure(ctx, fresh, bytes)) return rc;
  if (b.p) {
    HIPCHK(ctx, hipMemcpyAsync(fresh.p, b.p, b.cap, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  b = std::move(fresh);  // (frees the old records)
  return PBF_OK;
}

// pbf_set_collider_reaction's buffers, sized to the particle capacity: made when the feature is enabled and regrown when an
// upload grows the capacity while it is on, so that no step allocates
int ensure_reaction(pbf_ctx *ctx) {
  const size_t v = ctx->fp64 ? sizeof(double4) : sizeof(float4);
  if (int rc = ensure(ctx, ctx->pushRec, std::max<size_t>(ctx->cap, 1) * 2 * v)) return rc;
  if (ctx->col.friction)
    if (int rc = ensure_friction_partials(ctx)) return rc;
  return ensure(ctx, ctx->pushPartials, (ctx->cap / DIAG_TILE + 2) * sizeof(WrenchPartial));
}

// pbf_diagnostics' buffers, sized to the particle capacity: allocated by the first call that needs them (`first`) and, once
// they exist, regrown when an upload grows the capacity
int ensure_diag(pbf_ctx *ctx, bool first, bool density) {
  if (first || ctx->diagPartials.p)
    if (int rc = ensure(ctx, ctx->diagPartials, (ctx->cap / DIAG_TILE + 2) * sizeof(DiagPartial))) return rc;
  if ((first && density) || ctx->diagRho.p) {
    if (int rc = ensure(ctx, ctx->diagRho, ctx->cap * (ctx->fp64 ? sizeof(double) : sizeof(float)))) return rc;
    if (int rc = ensure(ctx, ctx->diagNbr, ctx->cap * 4)) return rc;
  }
  return PBF_OK;
}

// pbf_whitewater_step's per-fluid-particle buffers, sized to the particle capacity: allocated when the pool is configured and
// when an upload grows the capacity (the step itself only allocates when neither has seen the capacity yet)
int ensure_whitewater_fields(pbf_ctx *ctx) {
  const size_t v = ctx->fp64 ? sizeof(double4) : sizeof(float4), n = ctx->cap;
  if (!n) return PBF_OK;
  if (int rc = ensure(ctx, ctx->wwFieldA, n * v)) return rc;
  if (int rc = ensure(ctx, ctx->wwFieldB, n * v)) return rc;
  if (int rc = ensure(ctx, ctx->wwPot, n * v)) return rc;
  if (int rc = ensure(ctx, ctx->wwEmit, (n + SCAN_TILE) * 4)) return rc;  // (k_scan_block_sums reads whole uint4 pairs)
  if (int rc = ensure(ctx, ctx->wwOffset, (n + SCAN_TILE) * 4)) return rc;
  return ensure(ctx, ctx->wwChildKind, n);
}

// Surface tension and adhesion (Akinci et al. 2013), last among the extras: density -> A, normals -> B, velocity update.
template <typename N, bool FAST> int surface_tension_impl(pbf_ctx *ctx, const StepConsts<N> &c) {
  if (int rc = ensure_surface(ctx)) return rc;
  const int s = ctx->st.cur, o = 1 - s;
  const double h = ctx->desc.h;
  SurfArgs<N> a{};
  a.pstar = ctx->pstar[s].as<const vec4<N>>(), a.pos4 = ctx->pos4[s].as<const vec4<N>>();
  a.type = ctx->type[s].as<const uint8_t>();
  a.cohesion = N(ctx->cohesion), a.adhesion = N(ctx->adhesion);
  a.cohFactor = N(32.0 / (M_PI * std::pow(h, 9))), a.h6over64 = N(std::pow(h, 6) / 64.0);
  a.adhFactor = N(0.007 / std::pow(h, 3.25)), a.adhQuad = N(-4.0 / h);
  a.fieldOut = ctx->surfA.as<vec4<N>>();
  if (int rc = launch_gather<N, SurfaceDensityOp<N, FAST>>(ctx, c, a)) return rc;
  a.fieldIn = ctx->surfA.as<const vec4<N>>(), a.fieldOut = ctx->surfB.as<vec4<N>>();  // Jacobi: A is read while B is written
  if (int rc = launch_gather<N, SurfaceNormalOp<N, FAST>>(ctx, c, a)) return rc;
  a.fieldIn = ctx->surfB.as<const vec4<N>>(), a.fieldOut = nullptr;
  a.velIn = ctx->vel4[s].as<const vec4<N>>(), a.velOut = ctx->vel4[o].as<vec4<N>>();
  if (int rc = launch_gather<N, SurfaceTensionOp<N, FAST>>(ctx, c, a)) return rc;
  std::swap(ctx->vel4[s], ctx->vel4[o]);
  return PBF_OK;
}

template <typename N, bool FAST> int extras_impl(pbf_ctx *ctx, const pbf_params *p, const StepConsts<N> &c) {
  const int s = ctx->st.cur, o = 1 - s;
  const uint8_t *type = ctx->type[s].as<const uint8_t>();
  const vec4<N> *ps = ctx->pstar[s].as<const vec4<N>>();
  if (p->vorticity) {
    vec4<N> *omega = ctx->pstar[2].as<vec4<N>>();
    typename VorticityOp<N, FAST>::Args a1{ps, ctx->vel4[s].as<const vec4<N>>(), omega, type};
    if (int rc = launch_gather<N, VorticityOp<N, FAST>>(ctx, c, a1)) return rc;
    typename VorticityForceOp<N, FAST>::Args a2{ps, omega, ctx->vel4[s].as<const vec4<N>>(), ctx->vel4[o].as<vec4<N>>(), type};
    if (int rc = launch_gather<N, VorticityForceOp<N, FAST>>(ctx, c, a2)) return rc;
    std::swap(ctx->vel4[s], ctx->vel4[o]);
  }
  if (p->xsph) {
    typename XsphOp<N, FAST>::Args a3{ps, ctx->vel4[s].as<const vec4<N>>(), ctx->vel4[o].as<vec4<N>>(), type};
    if (int rc = launch_gather<N, XsphOp<N, FAST>>(ctx, c, a3)) return rc;
    std::swap(ctx->vel4[s], ctx->vel4[o]);
  }
  if (surface_on(ctx))
    if (int rc = surface_tension_impl<N, FAST>(ctx, c)) return rc;
  ctx->st.extras_done(p->vorticity != 0, surface_on(ctx));
  return PBF_OK;
}
template <typename N> int extras(pbf_ctx *ctx, const pbf_params *p, const StepConsts<N> &c) {
  if (ctx->slabActive && surface_on(ctx))
    return fail(ctx, PBF_ERR_STATE, "surface tension is not supported in slab mode (pbf_set_surface_tension(ctx, 0, 0) turns it off)");
  if (ctx->slabActive) return PBF_OK;  // slab mode: pbf_slab_step runs them itself, with the ghost refreshes in between
  return DISPATCH_FAST(ctx, extras_impl, ctx, p, c);
}

// pbf_set_collider_friction's pass, right after k_finalise and before the extras: one streaming launch over the step's
// reaction records (indexed as collider_reaction_impl chooses) on the finalised velocity.  No read-back, nothing allocated;
// captured with the step.
template <typename N> int stage_friction(pbf_ctx *ctx, const pbf_params *p) {
  const uint32_t n = uint32_t(ctx->n), nb = (n + DIAG_TILE - 1) / DIAG_TILE;
  const int s = ctx->st.cur;
  const pbf_collider_friction *rec = ctx->frictionRec.as<const pbf_collider_friction>();
  const double *vw = ctx->col.body ? ctx->bodyRec.as<const colliderbody::Record>()->st.velocity : rec->velocity;  // (addresses only)
  hipLaunchKernelGGL((k_collider_friction<N>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n, N(p->scale), N(p->dt), rec, vw,
                     ctx->colliderPose.as<const ColliderPose<N>>(), ctx->pushRec.as<const vec4<N>>(), push_slots(ctx),
                     ctx->pos4[s].as<const vec4<N>>(), ctx->vel4[s].as<vec4<N>>(), ctx->frictionPartials.as<WrenchPartial>(),
                     ctx->frictionCtl.as<colliderfriction::Ctl>());
  LAUNCH_CHECK(ctx);
  ctx->col.friction_passed();
  return PBF_OK;
}

template <typename N> int stage_finalise(pbf_ctx *ctx, const pbf_params *p) {
  StepConsts<N> c;
  if (int rc = make_consts<N>(ctx, p, c)) return rc;
  const int s = ctx->st.cur;
  if (ctx->col.friction) {  // (the pass follows the finalise below: refuse before anything is launched)
    if (int rc = collider_refuse_slab(ctx)) return rc;
    if (!push_current(ctx)) return fail(ctx, PBF_ERR_STATE, "the collider friction needs a sort since the reaction records were enabled");
  }
  if (ctx->fuseNextPredict && !extras_on(ctx, p) && !ctx->col.friction) {
    // finalise(t) + predict(t + 1) in one pass: everything stage_predict does, around one launch
    ctx->fuseNextPredict = false;
    if (int rc = ensure_table(ctx, c.tableN)) return rc;
    if (int rc = drop_histogram(ctx)) return rc;
    if (int rc = upload_wells(ctx, p)) return rc;
    if (int rc = join_diffuse(ctx)) return rc;  // (the side stream reads keys and types of this step)
    StageTimer t(ctx, ST_FINALISE);
    std::swap(ctx->pstar[ctx->st.pcur], ctx->pstar[s]);  // pStar is overwritten in place: make the live buffer pstar[cur] first
    hipLaunchKernelGGL((k_finalise_predict<N>), grid_for(ctx->n), dim3(BLOCK), 0, ctx->stream, c,
                       ctx->type[s].as<const uint8_t>(), ctx->pstar[s].as<vec4<N>>(), ctx->pos4[s].as<vec4<N>>(),
                       ctx->vel4[s].as<vec4<N>>(), ctx->wells.as<const N>(), ctx->key[s].as<uint32_t>(),
                       ctx->count.as<uint32_t>(), ctx->cellSlot.as<uint32_t>(), ctx->rowPstar[ctx->st.rcur].as<const vec4<N>>(),
                       ctx->st.pstarInRows ? ctx->rowSlotOf.as<const uint32_t>() : nullptr);
    ctx->st.predicted(c.tableN, /*ahead=*/true);
    LAUNCH_CHECK(ctx);
    return PBF_OK;
  }
  ctx->fuseNextPredict = false;
  if (ctx->st.pstarInRows && extras_on(ctx, p))  // the extras read the Morton-sorted pStar
    if (int rc = materialise_pstar<N>(ctx)) return rc;
  StageTimer t(ctx, ST_FINALISE);
  if (ctx->st.pstarInRows)
    hipLaunchKernelGGL((k_finalise<N>), grid_for(ctx->n), dim3(BLOCK), 0, ctx->stream, c, ctx->type[s].as<const uint8_t>(),
                       ctx->rowPstar[ctx->st.rcur].as<const vec4<N>>(), ctx->pos4[s].as<vec4<N>>(), ctx->vel4[s].as<vec4<N>>(),
                       ctx->rowSlotOf.as<const uint32_t>());
  else
    hipLaunchKernelGGL((k_finalise<N>), grid_for(ctx->n), dim3(BLOCK), 0, ctx->stream, c, ctx->type[s].as<const uint8_t>(),
                       ctx->pstar[ctx->st.pcur].as<const vec4<N>>(), ctx->pos4[s].as<vec4<N>>(), ctx->vel4[s].as<vec4<N>>(),
                       static_cast<const uint32_t *>(nullptr));
  LAUNCH_CHECK(ctx);
  // keep pstar[cur] as the live buffer so that a later sort scatters pstar[cur] -> pstar[1-cur]
  std::swap(ctx->pstar[ctx->st.pcur], ctx->pstar[s]);
  ctx->st.finalised();
  if (ctx->col.friction)  // (before the extras: they see the boundary-corrected velocity)
    if (int rc = stage_friction<N>(ctx, p)) return rc;
  if (extras_on(ctx, p)) return extras<N>(ctx, p, c);
  return PBF_OK;
}

// Sources and drains of the scene (ompsph.hpp:93-118) on the resident arrays: append the sources' sheets behind the
// particles present, then compact the fluid particles no drain reaches into the other array set (the sets swap roles,
// as in the sort).  The emitted count is host arithmetic; the drained one is data: ONE read-back per call while a drain
// is set (k_drain_scan -> pinned word, polled).  It is awaited before the move: when every particle survives — the
// common frame of an outlet nothing has reached yet — the arrays stay where they are and the move is not launched.
bool scene_on(const pbf_ctx *ctx) { return !ctx->sources.empty() || !ctx->drains.empty(); }
const char *kSceneSlabError = "sources and drains are not supported in slab mode (pbf_set_sources / pbf_set_drains with n = 0 clear them)";

template <typename N> int stage_scene(pbf_ctx *ctx, const pbf_params *p) {
  if (!scene_on(ctx)) return PBF_OK;
  if (ctx->comm || ctx->slabActive || ctx->ghostsPending) return fail(ctx, PBF_ERR_STATE, kSceneSlabError);
  const size_t e = ctx->emitTotal;
  // (the arrays carry slab-mode slack beyond a reserve, ensure_particles: not part of what the caller asked for)
  const size_t limit = ctx->reserve ? std::min(ctx->cap, std::max(ctx->reserve, ctx->uploaded)) : ctx->cap;
  if (ctx->n + e > limit)
    return fail(ctx, PBF_ERR_INVALID, "particle capacity exceeded by the sources' emission: call pbf_reserve before pbf_upload");
  if (e == 0 && (ctx->drains.empty() || ctx->n == 0)) return PBF_OK;
  if (ctx->downloadPending) (void)pbf_download_aos_end(ctx);
  if (int rc = join_diffuse(ctx)) return rc;
  if (int rc = drop_histogram(ctx)) return rc;  // (a predict without its sort: it describes the set before this stage)
  const int s = ctx->st.cur;
  ctx->st.arrays_replaced(s);
  if (e) {
    const N spacing = N(ctx->desc.h) * N(p->scale) / 2;  // ompsph.hpp:93
    hipLaunchKernelGGL((k_scene_emit<N>), grid_for(e), dim3(BLOCK), 0, ctx->stream, uint32_t(ctx->n), uint32_t(e),
                       uint32_t(ctx->sources.size()), ctx->sceneSources.as<const SceneSource<N>>(), spacing, arrays<N>(ctx, s, s));
    LAUNCH_CHECK(ctx);
    ctx->n += e;
  }
  if (ctx->drains.empty()) return PBF_OK;
  const uint32_t n = uint32_t(ctx->n), nb = (n + DRAIN_TILE - 1) / DRAIN_TILE, nd = uint32_t(ctx->drains.size());
  if (int rc = ensure(ctx, ctx->drainCounts, (ctx->cap / DRAIN_TILE + 2) * 4)) return rc;
  uint32_t seq, kept;
  HIPCHK(ctx, ctx->hostScene.arm(seq));
  const SceneDrain<N> *drains = ctx->sceneDrains.as<const SceneDrain<N>>();
  uint32_t *counts = ctx->drainCounts.as<uint32_t>();
  hipLaunchKernelGGL((k_drain_count<N>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n, ctx->pos4[s].as<const vec4<N>>(),
                     ctx->type[s].as<const uint8_t>(), drains, nd, counts);
  hipLaunchKernelGGL(k_drain_scan, dim3(1), dim3(BLOCK), 0, ctx->stream, nb, counts, &ctx->hostScene.rec.p->kept, seq);
  LAUNCH_CHECK(ctx);
  if (int rc = receive(ctx, ctx->hostScene, "drain read-back", kept)) return rc;
  ctx->sceneHostSyncs++;
  if (kept > n) return fail(ctx, PBF_ERR_HIP, "drain read-back: more survivors than particles");
  if (kept == n) return PBF_OK;
  if (kept) {
    hipLaunchKernelGGL((k_drain_move<N>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n, arrays<N>(ctx, s, s), arrays<N>(ctx, 1 - s, 1 - s),
                       drains, nd, counts);
    LAUNCH_CHECK(ctx);
    ctx->st.compacted(/*flipped=*/true);
  }
  ctx->n = kept;
  return PBF_OK;
}

// pbf_set_collider_body's stage, after the delta-p iterations and before finalise: the reaction records summed by the
// observer's partial kernel (indexed as collider_reaction_impl chooses) and ONE workgroup that folds the partial records,
// advances the body and writes the pose of the next step.  No read-back, nothing allocated; captured with the step.
template <typename N> int stage_body(pbf_ctx *ctx, const pbf_params *p) {
  if (int rc = collider_refuse_slab(ctx)) return rc;
  if (!push_current(ctx)) return fail(ctx, PBF_ERR_STATE, "the collider body needs a sort since the reaction records were enabled");
  const uint32_t n = uint32_t(ctx->n), nb = (n + DIAG_TILE - 1) / DIAG_TILE;
  hipLaunchKernelGGL((k_wrench_partial<N>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n, ctx->pushRec.as<const vec4<N>>(), push_slots(ctx),
                     ctx->pos4[ctx->st.cur].as<const vec4<N>>(), ctx->pushPartials.as<WrenchPartial>());
  if (ctx->col.friction)  // (the previous step's friction sums kick the body first, consumed once: the device's pending word)
    hipLaunchKernelGGL((k_body_kick_advance<N>), dim3(1), dim3(BLOCK), 0, ctx->stream, ctx->frictionPartials.as<const WrenchPartial>(),
                       ctx->frictionCtl.as<colliderfriction::Ctl>(), nb, ctx->pushPartials.as<const WrenchPartial>(), double(p->dt),
                       ctx->bodyRec.as<colliderbody::Record>(), ctx->colliderPose.as<ColliderPose<N>>());
  else
    hipLaunchKernelGGL((k_body_advance<N>), dim3(1), dim3(BLOCK), 0, ctx->stream, nb, ctx->pushPartials.as<const WrenchPartial>(),
                       double(p->dt), ctx->bodyRec.as<colliderbody::Record>(), ctx->colliderPose.as<ColliderPose<N>>());
  if (ctx->contact.on) {  // (pbf_set_collider_body_contact: the advanced body against the scenery, `iterations` passes of two launches)
    const uint32_t np = uint32_t(ctx->contact.points), cnb = (np + DIAG_TILE - 1) / DIAG_TILE;
    const ColliderSdf<N> scenery = sdf_args<N>(ctx->solid[ColliderState::SCENERY]);  // (its margin is replaced by the record's skin)
    for (uint32_t it = 0; it < ctx->contact.iterations; ++it) {
      hipLaunchKernelGGL((k_contact_partial<N>), dim3(cnb), dim3(BLOCK), 0, ctx->stream, scenery, np, ctx->contactPoints.as<const N>(),
                         ctx->bodyRec.as<const colliderbody::Record>(), ctx->contactRec.as<const bodycontact::Record>(),
                         ctx->contactPartials.as<ContactPartial>());
      hipLaunchKernelGGL((k_contact_resolve<N>), dim3(1), dim3(BLOCK), 0, ctx->stream, cnb, ctx->contactPartials.as<const ContactPartial>(),
                         ctx->bodyRec.as<colliderbody::Record>(), ctx->contactRec.as<bodycontact::Record>(),
                         ctx->colliderPose.as<ColliderPose<N>>());
    }
  }
  LAUNCH_CHECK(ctx);
  return PBF_OK;
}

template <typename N> int step_impl(pbf_ctx *ctx, const pbf_params *p) {
  if (scene_on(ctx))  // ompsph.hpp:93-118, before the "depleted" test as there: a source refills an empty state
    if (int rc = stage_scene<N>(ctx, p)) return rc;
  if (ctx->n == 0) return PBF_OK;  // "Particles depleted" (ompsph.hpp:122-126)
  if (!ctx->st.take_prediction())  // (else the previous step of this pbf_steps call has predicted already: k_finalise_predict)
    if (int rc = stage_predict<N>(ctx, p)) return rc;
  if (int rc = stage_sort<N>(ctx, p)) return rc;
  // diffuse (ompsph.hpp:188-207) visits exactly the candidates of the first lambda launch: fuse the two walks
  const bool fuse = ctx->fuseDiffuse && p->iteration > 0 && ctx->gatherKind == 1 && ctx->reuseLists &&
                    !(ctx->desc.flags & PBF_FLAG_NO_LDS);
  if (!fuse) {
    if (int rc = stage_diffuse<N>(ctx, p, /*overlap=*/p->iteration > 0)) return rc;
  }
  for (uint64_t it = 0; it < p->iteration; ++it) {
    if (int rc = stage_lambda<N>(ctx, p, fuse && it == 0)) return rc;
    if (int rc = stage_delta<N>(ctx, p)) return rc;
  }
  if (ctx->col.body)  // (pbf_set_collider_body: the step's reaction moves the solid before the next step reads its pose)
    if (int rc = stage_body<N>(ctx, p)) return rc;
  if (int rc = stage_finalise<N>(ctx, p)) return rc;
  return join_diffuse(ctx);  // the step is complete on ctx->stream only once the colours are
}

int check(pbf_ctx *ctx, const pbf_params *p, bool needSorted) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!p) return fail(ctx, PBF_ERR_INVALID, "params == NULL");
  if (!(p->scale > 0) || !(p->dt > 0)) return fail(ctx, PBF_ERR_INVALID, "dt and scale must be > 0");
  if (needSorted && !ctx->st.sorted) return fail(ctx, PBF_ERR_STATE, "stage needs pbf_stage_sort first");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ctx->lastParams = *p;
  ctx->haveParams = true;
  return PBF_OK;
}

// What the observers of the last step (entry point `who`) refuse alike.  Each entry point asks for the parts in its own,
// documented order, between the refusals that are its alone.
struct Refuse {
  pbf_ctx *ctx;
  const char *who;
  int params(const pbf_params *p) const {
    if (!(p->scale > 0) || !(p->dt > 0)) return fail(ctx, PBF_ERR_INVALID, "dt and scale must be > 0");
    return PBF_OK;
  }
  int slab_mode() const {
    if (ctx->comm || ctx->slabActive || ctx->ghostsPending || ctx->slabConfigured)
      return fail(ctx, PBF_ERR_STATE, std::string(who) + " is not supported in slab mode");
    return PBF_OK;
  }
  int no_step(const char *part = "") const {  // the keys and the table it reads are the last sort's
    if (!ctx->st.sorted) return fail(ctx, PBF_ERR_STATE, std::string(who) + part + " needs a step first (no valid cell table)");
    return PBF_OK;
  }
};

int drop_ghosts(pbf_ctx *ctx);  // (defined with the slab code)

template <typename N>
int upload_impl(pbf_ctx *ctx, size_t n, const uint64_t *id, const uint8_t *type, const N *mass, const N *pos,
                const N *vel, const N *colour) {
  if (ctx->downloadPending) (void)pbf_download_aos_end(ctx);  // (a download left open: finish it before the state changes)
  if (int rc = ensure_particles(ctx, n)) return rc;
  if (surface_on(ctx))
    if (int rc = ensure_surface(ctx)) return rc;
  if (int rc = ensure_diag(ctx, /*first=*/false, /*density=*/false)) return rc;
  if (ctx->col.reaction)
    if (int rc = ensure_reaction(ctx)) return rc;
  if (ctx->wwOn)
    if (int rc = ensure_whitewater_fields(ctx)) return rc;
  if (int rc = drop_histogram(ctx)) return rc;
  ctx->st.arrays_replaced(0);
  ctx->ghostsPending = false, ctx->slabActive = false;
  ctx->n = n, ctx->uploaded = n;
  ctx->hasObstacles = false;
  if (n == 0) return PBF_OK;
  std::vector<vec4<N>> P(n), V(n), C(n);
  for (size_t i = 0; i < n; ++i) {
    P[i] = make_vec4<N>(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], mass[i]);
    V[i] = make_vec4<N>(vel[3 * i], vel[3 * i + 1], vel[3 * i + 2], N(0));
    C[i] = make_vec4<N>(colour[4 * i], colour[4 * i + 1], colour[4 * i + 2], colour[4 * i + 3]);
    if (type[i] & PBF_TYPE_OBSTACLE) ctx->hasObstacles = true;
  }
  ctx->realObstacles = ctx->hasObstacles;
  HIPCHK(ctx, hipMemcpyAsync(ctx->pos4[0].p, P.data(), n * sizeof(vec4<N>), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->vel4[0].p, V.data(), n * sizeof(vec4<N>), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->col4[0].p, C.data(), n * sizeof(vec4<N>), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->id[0].p, id, n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->type[0].p, type, n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // P, V, C are temporaries
  return PBF_OK;
}

template <typename N>
int download_impl(pbf_ctx *ctx, uint64_t *id, uint8_t *type, N *mass, N *pos, N *vel, N *colour) {
  if (int rc = drop_ghosts(ctx)) return rc;
  const size_t n = ctx->n;
  if (n == 0) return PBF_OK;
  const int s = ctx->st.cur;
  std::vector<vec4<N>> tmp(n);
  if (mass || pos) {
    HIPCHK(ctx, hipMemcpyAsync(tmp.data(), ctx->pos4[s].p, n * sizeof(vec4<N>), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; ++i) {
      if (pos) pos[3 * i] = tmp[i].x, pos[3 * i + 1] = tmp[i].y, pos[3 * i + 2] = tmp[i].z;
      if (mass) mass[i] = tmp[i].w;
    }
  }
  if (vel) {
    HIPCHK(ctx, hipMemcpyAsync(tmp.data(), ctx->vel4[s].p, n * sizeof(vec4<N>), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; ++i) vel[3 * i] = tmp[i].x, vel[3 * i + 1] = tmp[i].y, vel[3 * i + 2] = tmp[i].z;
  }
  if (colour) {
    HIPCHK(ctx, hipMemcpyAsync(colour, ctx->col4[s].p, n * sizeof(vec4<N>), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (id) HIPCHK(ctx, hipMemcpyAsync(id, ctx->id[s].p, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (type) HIPCHK(ctx, hipMemcpyAsync(type, ctx->type[s].p, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PBF_OK;
}

}  // namespace

extern "C" {

int pbf_abi_version(void) { return PBF_ABI_VERSION; }

int pbf_set_surface_tension(pbf_ctx *ctx, double cohesion, double adhesion) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!std::isfinite(cohesion) || !std::isfinite(adhesion) || cohesion < 0 || adhesion < 0)
    return fail(ctx, PBF_ERR_INVALID, "pbf_set_surface_tension: cohesion and adhesion must be finite and >= 0");
  if (ctx->comm && (cohesion > 0 || adhesion > 0))
    return fail(ctx, PBF_ERR_STATE, "surface tension is not supported in slab mode (pbf_slab_attach)");
  ctx->cohesion = cohesion, ctx->adhesion = adhesion;
  if (surface_on(ctx) && ctx->cap) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return ensure_surface(ctx);
  }
  return PBF_OK;
}

int pbf_set_option(pbf_ctx *ctx, const char *name, int64_t value) {
  if (!ctx || !name) return PBF_ERR_INVALID;
  const std::string n(name);
  if (n == "list_max") ctx->listMax = uint32_t(value);
  else if (n == "gather") {
    if (value != 0 && value != 1 && value != 3) return fail(ctx, PBF_ERR_INVALID, "gather: 0, 1 or 3 (2, round 1's brick kernel, was removed)");
    ctx->gatherKind = int(value);
  }
  else if (n == "tile_cap") ctx->tileCap = uint32_t(value);
  else if (n == "reuse_lists") ctx->reuseLists = value != 0;
  else if (n == "fuse_diffuse") ctx->fuseDiffuse = value != 0;
  else if (n == "cell_diffuse") ctx->cellDiffuse = value != 0;
  else if (n == "pipeline") ctx->pipeline = int(value);
  else if (n == "graph") ctx->graphMode = int(value);
  else if (n == "overlap_diffuse") ctx->overlapDiffuse = value != 0, ctx->overlapDiffuseForced = true;
  else if (n == "coop") {
    if (value != 0 && value != 2 && value != 4 && value != 8) return fail(ctx, PBF_ERR_INVALID, "coop must be 0, 2, 4 or 8");
    ctx->coop = int(value);
  }
  else if (n == "iter_wg" || n == "build_wg" || n == "reader_wg") {
    if (value != 64 && value != 128 && value != 256) return fail(ctx, PBF_ERR_INVALID, n + " must be 64, 128 or 256");
    if (n != "reader_wg") ctx->buildWg = int(value);
    if (n != "build_wg") ctx->readerWg = int(value);
  }
  else if (n == "split_build") ctx->splitBuild = int(value);
  else if (n == "fuse_predict") ctx->fusePredict = value != 0;
  else if (n == "timing_mask") ctx->timingMask = uint32_t(value);
  else if (n == "pad_lds") ctx->padLds = uint32_t(value);
  else if (n == "row_major") ctx->rowMajor = int(value);
  else if (n == "row_diffuse") ctx->rowDiffuse = int(value);
  else if (n == "diffuse_cap") {
    if (value < 0 || value > 4096) return fail(ctx, PBF_ERR_INVALID, "diffuse_cap: 0 (default) .. 4096 records");
    ctx->diffuseCap = uint32_t(value);
  }
  else if (n == "sdf_cull") ctx->sdfCull = value != 0;
  else if (n == "sdf_launch_pairs") {
    if (value < 0) return fail(ctx, PBF_ERR_INVALID, "sdf_launch_pairs: 0 (default) or the cap on pairs per launch");
    ctx->sdfLaunchPairs = uint64_t(value);
  }
  else if (n == "nbr_chunks") {  // diagnostic: size of the lists' second tier (before the first upload; 0 = capacity / 8 + 1024)
    if (ctx->cap) return fail(ctx, PBF_ERR_STATE, "nbr_chunks must be set before the first upload");
    ctx->nbrChunksOpt = uint32_t(value);
  }
  else return fail(ctx, PBF_ERR_INVALID, "unknown option " + n);
  return PBF_OK;
}

int pbf_create(const pbf_desc *desc, pbf_ctx **out) {
  if (!desc || !out) {
    g_create_error = "pbf_create: NULL argument";
    return PBF_ERR_INVALID;
  }
  *out = nullptr;
  if (desc->abi_version != PBF_ABI_VERSION) {
    g_create_error = "pbf_create: abi_version mismatch";
    return PBF_ERR_INVALID;
  }
  if (!(desc->h > 0)) {
    g_create_error = "pbf_create: h must be > 0";
    return PBF_ERR_INVALID;
  }
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    g_create_error = std::string("pbf_create: no usable HIP device (") + hipGetErrorString(e) +
                     "); this library has no CPU fallback";
    return PBF_ERR_NO_DEVICE;
  }
  if (desc->device < 0 || desc->device >= count) {
    g_create_error = "pbf_create: device ordinal out of range";
    return PBF_ERR_INVALID;
  }
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, desc->device)) != hipSuccess) {
    g_create_error = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
    return PBF_ERR_HIP;
  }
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    g_create_error = std::string("pbf_create: device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
    return PBF_ERR_NO_DEVICE;
  }
  auto *ctx = new pbf_ctx();
  ctx->desc = *desc;
  ctx->device = desc->device;
  ctx->fp64 = desc->fp64 != 0;
  ctx->fast = (desc->flags & PBF_FLAG_FAST_MATH) != 0;
  ctx->numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (const char *e = std::getenv("PBF_TILE_CAP")) ctx->tileCap = uint32_t(std::atoi(e));
  if (const char *e = std::getenv("PBF_GATHER")) {
    const int g = std::atoi(e);
    if (g == 0 || g == 1 || g == 3) ctx->gatherKind = g;  // (2, round 1's brick kernel, was removed)
  }
  if (const char *e = std::getenv("PBF_REUSE_LISTS")) ctx->reuseLists = std::atoi(e) != 0;
  if (const char *e = std::getenv("PBF_SPLIT_BUILD")) ctx->splitBuild = std::atoi(e);
  if (const char *e = std::getenv("PBF_LIST_MAX")) ctx->listMax = uint32_t(std::atoi(e));
  if (const char *e = std::getenv("PBF_OVERLAP_DIFFUSE")) ctx->overlapDiffuse = std::atoi(e) != 0, ctx->overlapDiffuseForced = true;
  if (const char *e = std::getenv("PBF_PIPELINE")) ctx->pipeline = std::atoi(e);
  if (const char *e = std::getenv("PBF_ROW_MAJOR")) ctx->rowMajor = std::atoi(e);
  if (const char *e = std::getenv("PBF_GRAPH")) ctx->graphMode = std::atoi(e);
  auto width_env = [](const char *name, int dflt) {
    const char *e = std::getenv(name);
    const int v = e ? std::atoi(e) : 0;
    return v == 64 || v == 128 || v == 256 ? v : dflt;
  };
  ctx->buildWg = width_env("PBF_BUILD_WG", width_env("PBF_ITER_WG", 0));
  ctx->readerWg = width_env("PBF_READER_WG", width_env("PBF_ITER_WG", 0));
  if (const char *e = std::getenv("PBF_COOP")) {
    const int v = std::atoi(e);
    if (v == 0 || v == 2 || v == 4 || v == 8) ctx->coop = v;
  }
  if ((e = hipSetDevice(ctx->device)) != hipSuccess) {
    g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e);
    delete ctx;
    return PBF_ERR_HIP;
  }
  if (desc->stream) {
    ctx->stream = static_cast<hipStream_t>(desc->stream);
  } else {
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) {
      g_create_error = std::string("hipStreamCreate: ") + hipGetErrorString(e);
      delete ctx;
      return PBF_ERR_HIP;
    }
    ctx->ownStream = true;
  }
  *out = ctx;
  return PBF_OK;
}

void pbf_destroy(pbf_ctx *ctx) {
  if (ctx && ctx->downloadPending) (void)pbf_download_aos_end(ctx);
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto &ep : ctx->pending) {
    (void)hipEventDestroy(ep.a);
    (void)hipEventDestroy(ep.b);
  }
  for (auto ev : ctx->freeEvents) (void)hipEventDestroy(ev);
  for (auto &g : ctx->graphs)
    if (g.second.exec) (void)hipGraphExecDestroy(g.second.exec);
  if (ctx->evFork) (void)hipEventDestroy(ctx->evFork);
  if (ctx->evJoin) (void)hipEventDestroy(ctx->evJoin);
  if (ctx->sideStream) (void)hipStreamDestroy(ctx->sideStream);
  if (ctx->copyStream) (void)hipStreamDestroy(ctx->copyStream);
  if (ctx->evPacked) (void)hipEventDestroy(ctx->evPacked);
  if (ctx->regPtr) (void)hipHostUnregister(ctx->regPtr);
  if (ctx->ownStream) (void)hipStreamDestroy(ctx->stream);
  // every DevBuf and Pinned frees itself here: this device is current and the stream has drained (the side stream's work was
  // joined into it by the step that started it, the copy stream's by the download ended above)
  delete ctx;
}

const char *pbf_last_error(const pbf_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int pbf_upload(pbf_ctx *ctx, size_t n, const uint64_t *id, const uint8_t *type, const void *mass, const void *pos,
               const void *vel, const void *colour) {
  if (!ctx) return PBF_ERR_INVALID;
  if (n && (!id || !type || !mass || !pos || !vel || !colour)) return fail(ctx, PBF_ERR_INVALID, "NULL array");
  if (n >= (size_t(1) << 31)) return fail(ctx, PBF_ERR_INVALID, "n must be < 2^31 (ompsph.hpp:41 iterates with int)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->fp64)
    return upload_impl<double>(ctx, n, id, type, (const double *)mass, (const double *)pos, (const double *)vel,
                               (const double *)colour);
  return upload_impl<float>(ctx, n, id, type, (const float *)mass, (const float *)pos, (const float *)vel,
                            (const float *)colour);
}

int pbf_download(pbf_ctx *ctx, uint64_t *id, uint8_t *type, void *mass, void *pos, void *vel, void *colour) {
  if (!ctx) return PBF_ERR_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->fp64)
    return download_impl<double>(ctx, id, type, (double *)mass, (double *)pos, (double *)vel, (double *)colour);
  return download_impl<float>(ctx, id, type, (float *)mass, (float *)pos, (float *)vel, (float *)colour);
}

size_t pbf_count(const pbf_ctx *ctx) { return ctx ? (ctx->ghostsPending ? ctx->nOwned : ctx->n) : 0; }

namespace {
// Page-lock the caller's AoS buffer once and keep the registration while the same buffer comes back every frame
// (benchmark.cpp:33,47 calls advance() on one vector).  Failure is not an error: the copy then takes the pageable path.
void pin_user_buffer(pbf_ctx *ctx, const void *ptr, size_t bytes) {
  if (ctx->regPtr == ptr && ctx->regBytes >= bytes) return;
  if (ctx->regPtr) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipHostUnregister(ctx->regPtr);
    ctx->regPtr = nullptr, ctx->regBytes = 0;
  }
  if (bytes < (1u << 20)) return;  // small scenes: registration costs more than it saves
  if (hipHostRegister(const_cast<void *>(ptr), bytes, hipHostRegisterDefault) == hipSuccess)
    ctx->regPtr = const_cast<void *>(ptr), ctx->regBytes = bytes;
  else
    (void)hipGetLastError();
}
}  // namespace

int pbf_upload_aos(pbf_ctx *ctx, size_t n, const void *particles, const pbf_aos_layout *l) {
  if (ctx && ctx->downloadPending) (void)pbf_download_aos_end(ctx);  // (an open download owns the staging buffer)
  if (!ctx) return PBF_ERR_INVALID;
  if (!l || (n && !particles)) return fail(ctx, PBF_ERR_INVALID, "NULL argument");
  if (n >= (size_t(1) << 31)) return fail(ctx, PBF_ERR_INVALID, "n must be < 2^31");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = ensure_particles(ctx, n)) return rc;
  if (surface_on(ctx))
    if (int rc = ensure_surface(ctx)) return rc;
  if (int rc = ensure_diag(ctx, /*first=*/false, /*density=*/false)) return rc;
  if (ctx->col.reaction)
    if (int rc = ensure_reaction(ctx)) return rc;
  if (int rc = drop_histogram(ctx)) return rc;
  ctx->st.arrays_replaced(0);
  ctx->n = n, ctx->uploaded = n;
  ctx->ghostsPending = false, ctx->slabActive = false;
  ctx->hasObstacles = false;
  if (n == 0) return PBF_OK;
  if (int rc = ensure(ctx, ctx->staging, n * l->stride)) return rc;
  if (int rc = ensure(ctx, ctx->selTotals, 16)) return rc;
  pin_user_buffer(ctx, particles, n * l->stride);
  HIPCHK(ctx, hipMemcpyAsync(ctx->staging.p, particles, n * l->stride, hipMemcpyHostToDevice, ctx->stream));
  ctx->stagedBytes = n * l->stride;
  // "are there obstacle particles" is answered by the unpack kernel (a strided host scan over the 56-byte structs cost
  // more than the copy itself: 2 of 3 ms at 1 M particles)
  uint32_t *flag = ctx->selTotals.as<uint32_t>() + 3;
  HIPCHK(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
  AosLayout L{l->stride, l->off_id, l->off_type, l->off_mass, l->off_pos, l->off_vel, l->off_colour};
  if (ctx->fp64)
    hipLaunchKernelGGL((k_unpack_aos<double>), grid_for(n), dim3(BLOCK), 0, ctx->stream, uint32_t(n),
                       ctx->staging.as<const uint8_t>(), L, arrays<double>(ctx, 0, 0), flag);
  else
    hipLaunchKernelGGL((k_unpack_aos<float>), grid_for(n), dim3(BLOCK), 0, ctx->stream, uint32_t(n),
                       ctx->staging.as<const uint8_t>(), L, arrays<float>(ctx, 0, 0), flag);
  LAUNCH_CHECK(ctx);
  uint32_t any = 0;
  HIPCHK(ctx, hipMemcpyAsync(&any, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
  // the caller owns `particles` and may change or free it as soon as we return: from page-locked memory the copy
  // above is a genuinely asynchronous DMA, so wait for it (the pageable path used to block inside the runtime)
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->hasObstacles = any != 0;
  ctx->realObstacles = ctx->hasObstacles;
  return PBF_OK;
}

// The download in two halves: _begin packs the AoS image on the solver's stream and starts its DMA on a copy stream of
// its own, _end waits for it — so that whatever the caller enqueues in between (the surface kernels) runs WHILE the
// particles travel.  The image is packed before _begin returns control to the stream, so later launches cannot change
// what travels; the uploads (which reuse the staging buffer) and pbf_destroy end an open download themselves.
int pbf_download_aos_begin(pbf_ctx *ctx, void *particles, const pbf_aos_layout *l) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!l || (ctx->n && !particles)) return fail(ctx, PBF_ERR_INVALID, "NULL argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->downloadPending) return fail(ctx, PBF_ERR_STATE, "pbf_download_aos_begin: the previous one has not been ended");
  if (int rc = drop_ghosts(ctx)) return rc;
  const size_t n = ctx->n;
  if (n == 0) return PBF_OK;
  const size_t before = ctx->staging.cap;
  if (int rc = ensure(ctx, ctx->staging, n * l->stride)) return rc;
  if (ctx->staging.cap != before) ctx->stagedBytes = 0;  // (a grown buffer starts undefined)
  // Only the fields are written below.  The struct's padding bytes are no part of the reference's contract (its
  // write-back copies whole structs whose padding is unspecified, ompsph.hpp:479-481): they keep the bytes of the
  // last uploaded image at that slot — all zero / all equal in practice — instead of costing a second full
  // host-to-device copy per frame as in round 1; slots never uploaded are zeroed.
  if (ctx->stagedBytes < n * l->stride) {
    HIPCHK(ctx, hipMemsetAsync(ctx->staging.as<uint8_t>() + ctx->stagedBytes, 0, n * l->stride - ctx->stagedBytes, ctx->stream));
    ctx->stagedBytes = n * l->stride;
  }
  pin_user_buffer(ctx, particles, n * l->stride);
  AosLayout L{l->stride, l->off_id, l->off_type, l->off_mass, l->off_pos, l->off_vel, l->off_colour};
  if (ctx->fp64)
    hipLaunchKernelGGL((k_pack_aos<double>), grid_for(n), dim3(BLOCK), 0, ctx->stream, uint32_t(n),
                       ctx->staging.as<uint8_t>(), L, arrays<double>(ctx, ctx->st.cur, ctx->st.pcur));
  else
    hipLaunchKernelGGL((k_pack_aos<float>), grid_for(n), dim3(BLOCK), 0, ctx->stream, uint32_t(n),
                       ctx->staging.as<uint8_t>(), L, arrays<float>(ctx, ctx->st.cur, ctx->st.pcur));
  LAUNCH_CHECK(ctx);
  if (!ctx->copyStream) {
    HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copyStream, hipStreamNonBlocking));
    HIPCHK(ctx, hipEventCreateWithFlags(&ctx->evPacked, hipEventDisableTiming));
  }
  HIPCHK(ctx, hipEventRecord(ctx->evPacked, ctx->stream));
  HIPCHK(ctx, hipStreamWaitEvent(ctx->copyStream, ctx->evPacked, 0));
  HIPCHK(ctx, hipMemcpyAsync(particles, ctx->staging.p, n * l->stride, hipMemcpyDeviceToHost, ctx->copyStream));
  ctx->downloadPending = true;
  return PBF_OK;
}
int pbf_download_aos_end(pbf_ctx *ctx) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!ctx->downloadPending) return PBF_OK;
  ctx->downloadPending = false;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->copyStream));
  return PBF_OK;
}
int pbf_download_aos(pbf_ctx *ctx, void *particles, const pbf_aos_layout *l) {
  if (int rc = pbf_download_aos_begin(ctx, particles, l)) return rc;
  return pbf_download_aos_end(ctx);
}

int pbf_step(pbf_ctx *ctx, const pbf_params *p) {
  if (int rc = check(ctx, p, false)) return rc;
  if (int rc = drop_ghosts(ctx)) return rc;
  return DISPATCH(ctx, step_impl, ctx, p);
}

}  // extern "C"

namespace {

void role_buffers(pbf_ctx *ctx, DevBuf *out[15]) {
  DevBuf *all[15] = {&ctx->pos4[0], &ctx->pos4[1], &ctx->vel4[0], &ctx->vel4[1], &ctx->col4[0], &ctx->col4[1],
                     &ctx->id[0],   &ctx->id[1],   &ctx->type[0], &ctx->type[1], &ctx->key[0],  &ctx->key[1],
                     &ctx->pstar[0], &ctx->pstar[1], &ctx->pstar[2]};
  for (int k = 0; k < 15; ++k) out[k] = all[k];
}
StepState snapshot(pbf_ctx *ctx) {
  StepState s;
  std::memset(&s, 0, sizeof(s));  // (padding bytes take part in the comparison)
  s.st = ctx->st, s.hasObstacles = ctx->hasObstacles;
  s.tableN = ctx->tableN, s.gatherSeq = ctx->gatherSeq;
  DevBuf *b[15];
  role_buffers(ctx, b);
  for (int k = 0; k < 3; ++k) s.extent[k] = ctx->extent[k], s.minExtent[k] = ctx->minExtent[k];
  for (int k = 0; k < 15; ++k) s.bufs[k] = b[k]->p, s.caps[k] = b[k]->cap;
  return s;
}
void restore(pbf_ctx *ctx, const StepState &s) {
  ctx->st = s.st, ctx->hasObstacles = s.hasObstacles;  // (all of the derived state, not only what the key compares)
  ctx->tableN = s.tableN, ctx->gatherSeq = s.gatherSeq;
  ctx->orderEpoch++;  // (a replayed step has sorted; a rolled-back capture re-runs its sort)
  ctx->col.step_replayed(ctx->orderEpoch);  // (the records' clear ran with it, and the friction pass)
  DevBuf *b[15];
  role_buffers(ctx, b);
  for (int k = 0; k < 3; ++k) ctx->extent[k] = s.extent[k], ctx->minExtent[k] = s.minExtent[k];
  for (int k = 0; k < 15; ++k) b[k]->p = s.bufs[k], b[k]->cap = s.caps[k];
}
GraphKey graph_key(pbf_ctx *ctx, const pbf_params *p, const StepState &before) {
  GraphKey k;
  std::memset(&k, 0, sizeof(k));
  k.before = before;
  // of the derived state only what a step's launch sequence depends on takes part (a key that also compared, say,
  // omegaValid would capture the same step twice)
  std::memset(static_cast<void *>(&k.before.st), 0, sizeof(k.before.st));
  before.st.step_key(k.before.st);
  double v[11] = {p->dt, p->scale, p->constant_force[0], p->constant_force[1], p->constant_force[2], p->min_bound[0],
                  p->min_bound[1], p->min_bound[2], p->max_bound[0], p->max_bound[1], p->max_bound[2]};
  std::memcpy(k.params, v, sizeof(v));
  const uint64_t it = p->iteration;
  const int32_t xv[2] = {p->xsph, p->vorticity};
  const double st[2] = {ctx->cohesion, ctx->adhesion};  // (pbf_set_surface_tension: a ctx setting, not a pbf_params field)
  std::memcpy(k.params + sizeof(v), &it, 8);
  std::memcpy(k.params + sizeof(v) + 8, xv, 8);
  std::memcpy(k.params + sizeof(v) + 16, st, 16);
  k.n = ctx->n;
  k.collider = ctx->col.gen;
  k.contact = ctx->contact.gen;
  const int opt[12] = {ctx->gatherKind, ctx->splitBuild, ctx->coop, ctx->pipeline, int(ctx->cellDiffuse), int(ctx->overlapDiffuse),
                       int(ctx->fuseDiffuse), int(ctx->reuseLists), int(ctx->listMax), int(ctx->tileCap), ctx->buildWg, ctx->readerWg};
  std::memcpy(k.options, opt, sizeof(opt));
  return k;
}

// One step of pbf_steps: replayed from a captured graph when this exact step (same buffer roles, same parameters) has been
// seen before, captured the first time it comes by, eager whenever capturing is not possible.
int step_maybe_graphed(pbf_ctx *ctx, const pbf_params *p) {
  const bool timing = (ctx->desc.flags & PBF_FLAG_STAGE_TIMING) != 0 && ctx->timingMask != 0;
  if (ctx->graphMode <= 0 || timing || p->n_wells > 0 || ctx->n == 0 || ctx->slabConfigured || scene_on(ctx))
    return DISPATCH(ctx, step_impl, ctx, p);
  const StepState before = snapshot(ctx);
  const GraphKey key = graph_key(ctx, p, before);
  auto it = ctx->graphs.find(key);
  if (it != ctx->graphs.end()) {
    HIPCHK(ctx, hipGraphLaunch(it->second.exec, ctx->stream));
    // (omegaValid / surfaceValid included: the extras' switches and coefficients are part of the key, so the replayed step
    // ran those passes iff the captured one did)
    restore(ctx, it->second.after);
    ctx->graphMisses = 0;
    ctx->graphReplays++;
    return PBF_OK;
  }
  if (ctx->graphs.size() >= 32 || ctx->graphMisses >= 8) {  // the steps never repeat (a box that moves every frame)
    ctx->graphMode = 0;
    return DISPATCH(ctx, step_impl, ctx, p);
  }
  // capture only a step that allocates nothing: run it eagerly once more if the last one still grew a buffer
  const uint64_t epoch = ctx->allocEpoch;
  if (ctx->graphCaptures == 0 && ctx->graphReplays == 0 && ctx->graphMisses == 0) {
    ctx->graphMisses = 1;  // the very first step after an upload allocates (scratch, side stream): eager
    return DISPATCH(ctx, step_impl, ctx, p);
  }
  hipGraph_t graph = nullptr;
  if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed) != hipSuccess) {
    (void)hipGetLastError();
    ctx->graphMode = 0;
    return DISPATCH(ctx, step_impl, ctx, p);
  }
  const int rc = DISPATCH(ctx, step_impl, ctx, p);
  const hipError_t e = hipStreamEndCapture(ctx->stream, &graph);
  if (rc != PBF_OK || e != hipSuccess || !graph || ctx->allocEpoch != epoch) {
    // could not be captured (an allocation, a call that is illegal while capturing): nothing ran — redo it eagerly
    if (graph) (void)hipGraphDestroy(graph);
    (void)hipGetLastError();
    ctx->graphMode = 0;
    restore(ctx, before);
    ctx->diffusePending = false;
    return DISPATCH(ctx, step_impl, ctx, p);
  }
  GraphEntry entry;
  const hipError_t ei = hipGraphInstantiate(&entry.exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ei != hipSuccess) {
    (void)hipGetLastError();
    ctx->graphMode = 0;
    restore(ctx, before);
    ctx->diffusePending = false;
    return DISPATCH(ctx, step_impl, ctx, p);
  }
  entry.after = snapshot(ctx);
  ctx->graphs.emplace(key, entry);
  ctx->graphCaptures++, ctx->graphMisses++;
  HIPCHK(ctx, hipGraphLaunch(entry.exec, ctx->stream));  // the capture recorded the step; this runs it
  return PBF_OK;
}

}  // namespace

extern "C" {

int pbf_steps(pbf_ctx *ctx, const pbf_params *p, uint32_t count) {
  if (int rc = check(ctx, p, false)) return rc;
  if (int rc = drop_ghosts(ctx)) return rc;
  // finalise(t) + predict(t + 1) as one kernel between two steps of THIS call (same parameters, nothing observes the
  // state in between).  Not with stage timing on either entry, hipGraph replay, slabs or a step that may stop early.
  const bool timed = (ctx->desc.flags & PBF_FLAG_STAGE_TIMING) != 0 &&
                     (((ctx->timingMask >> ST_PREDICT) & 1u) != 0 || ((ctx->timingMask >> ST_FINALISE) & 1u) != 0);
  // (nor across the scene stage: sources and drains change the set between finalise(t) and predict(t + 1))
  const bool fusable = ctx->fusePredict && !timed && ctx->graphMode <= 0 && !ctx->slabActive && ctx->n != 0 && !scene_on(ctx);
  for (uint32_t i = 0; i < count; ++i) {
    ctx->fuseNextPredict = fusable && i + 1 < count;
    if (int rc = step_maybe_graphed(ctx, p)) {
      ctx->fuseNextPredict = false;
      (void)ctx->st.take_prediction();
      return rc;
    }
  }
  ctx->fuseNextPredict = false;
  return PBF_OK;
}
int pbf_graph_stats(const pbf_ctx *ctx, uint64_t out[3]) {
  if (!ctx || !out) return PBF_ERR_INVALID;
  out[0] = ctx->graphCaptures, out[1] = ctx->graphReplays, out[2] = uint64_t(ctx->graphMode > 0);
  return PBF_OK;
}
int pbf_sync(pbf_ctx *ctx) {
  if (!ctx) return PBF_ERR_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PBF_OK;
}

int pbf_stage_predict(pbf_ctx *ctx, const pbf_params *p) {
  if (int rc = check(ctx, p, false)) return rc;
  if (ctx->n == 0) return PBF_OK;
  return DISPATCH(ctx, stage_predict, ctx, p);
}
int pbf_stage_sort(pbf_ctx *ctx, const pbf_params *p) {
  if (int rc = check(ctx, p, false)) return rc;
  if (ctx->n == 0) return PBF_OK;
  return DISPATCH(ctx, stage_sort, ctx, p);
}
int pbf_stage_diffuse(pbf_ctx *ctx, const pbf_params *p) {
  if (int rc = check(ctx, p, true)) return rc;
  return DISPATCH(ctx, stage_diffuse, ctx, p);
}
int pbf_stage_lambda(pbf_ctx *ctx, const pbf_params *p) {
  if (int rc = check(ctx, p, true)) return rc;
  return DISPATCH(ctx, stage_lambda, ctx, p);
}
int pbf_stage_delta(pbf_ctx *ctx, const pbf_params *p) {
  if (ctx && (collider_on(ctx) || scenery_on(ctx)))
    if (int rc = collider_refuse_slab(ctx)) return rc;
  if (int rc = check(ctx, p, true)) return rc;
  return DISPATCH(ctx, stage_delta, ctx, p);
}
int pbf_stage_finalise(pbf_ctx *ctx, const pbf_params *p) {
  if (int rc = check(ctx, p, true)) return rc;
  return DISPATCH(ctx, stage_finalise, ctx, p);
}
int pbf_stage_body(pbf_ctx *ctx, const pbf_params *p) {
  if (int rc = check(ctx, p, false)) return rc;
  if (!ctx->col.body) return fail(ctx, PBF_ERR_STATE, "pbf_stage_body: no body set (pbf_set_collider_body)");
  if (ctx->n == 0) return PBF_OK;  // (a depleted step does not advance the body)
  return DISPATCH(ctx, stage_body, ctx, p);
}
int pbf_stage_scene(pbf_ctx *ctx, const pbf_params *p) {
  if (int rc = check(ctx, p, false)) return rc;
  if (int rc = drop_ghosts(ctx)) return rc;
  return DISPATCH(ctx, stage_scene, ctx, p);
}

}  // extern "C"

namespace {
template <typename N> int upload_sources(pbf_ctx *ctx, const std::vector<pbf_source> &src, uint32_t &total) {
  std::vector<SceneSource<N>> img(src.size());
  uint64_t at = 0;
  for (size_t k = 0; k < src.size(); ++k) {
    SceneSource<N> &d = img[k];
    for (int a = 0; a < 3; ++a) d.centre[a] = N(src[k].centre[a]), d.velocity[a] = N(src[k].velocity[a]);
    for (int a = 0; a < 4; ++a) d.colour[a] = N(src[k].colour[a]);
    const N size = std::sqrt(static_cast<N>(src[k].rate));  // ompsph.hpp:95-97
    if (!(size < N(32768))) return fail(ctx, PBF_ERR_INVALID, "pbf_set_sources: rate beyond 2^30 particles per step");
    d.tag = src[k].tag, d.width = uint32_t(std::floor(size)), d.depth = uint32_t(std::ceil(size)), d.first = uint32_t(at), d.pad = 0;
    at += uint64_t(d.width) * d.depth;
    if (at >= (uint64_t(1) << 31)) return fail(ctx, PBF_ERR_INVALID, "pbf_set_sources: more than 2^31 particles per step");
  }
  if (!img.empty()) {
    if (int rc = ensure(ctx, ctx->sceneSources, img.size() * sizeof(SceneSource<N>))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (a step in flight may still read the previous image)
    HIPCHK(ctx, hipMemcpy(ctx->sceneSources.p, img.data(), img.size() * sizeof(SceneSource<N>), hipMemcpyHostToDevice));
  }
  total = uint32_t(at);
  return PBF_OK;
}
template <typename N> int upload_drains(pbf_ctx *ctx, const std::vector<pbf_drain> &drn) {
  std::vector<SceneDrain<N>> img(drn.size());
  for (size_t k = 0; k < drn.size(); ++k) {
    for (int a = 0; a < 3; ++a) img[k].centre[a] = N(drn[k].centre[a]);
    img[k].width = N(drn[k].width);
  }
  if (img.empty()) return PBF_OK;
  if (int rc = ensure(ctx, ctx->sceneDrains, img.size() * sizeof(SceneDrain<N>))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipMemcpy(ctx->sceneDrains.p, img.data(), img.size() * sizeof(SceneDrain<N>), hipMemcpyHostToDevice));
  return PBF_OK;
}
// The consts of `p` for a call that works on what the last step left: make_consts leaves its grid in the ctx, so the last
// step's is kept, and params that describe another one are refused (the table, the keys and the arrays on the device belong to
// the step's grid; a larger tableN would index beyond them).
template <typename N> int consts_on_last_grid(pbf_ctx *ctx, const pbf_params *p, StepConsts<N> &c, const char *who) {
  const uint32_t tableN = ctx->tableN;
  uint64_t extent[3];
  double minExtent[3];
  std::memcpy(extent, ctx->extent, sizeof(extent)), std::memcpy(minExtent, ctx->minExtent, sizeof(minExtent));
  const int made = make_consts<N>(ctx, p, c);
  const bool sameGrid = made == PBF_OK && c.tableN == tableN && std::memcmp(extent, ctx->extent, sizeof(extent)) == 0 &&
                        std::memcmp(minExtent, ctx->minExtent, sizeof(minExtent)) == 0;
  ctx->tableN = tableN;
  std::memcpy(ctx->extent, extent, sizeof(extent)), std::memcpy(ctx->minExtent, minExtent, sizeof(minExtent));
  if (made != PBF_OK) return made;
  if (!sameGrid) return fail(ctx, PBF_ERR_STATE, std::string(who) + ": bounds / scale differ from the last step's");
  return PBF_OK;
}

// pbf_diagnostics.  The stream part reads the arrays pbf_download would return; the density part runs DensityOp over the final
// pStar (pstar[cur] after finalise) on the last step's keys and table, through whichever gather kernel the ctx is set to.
// Neither touches a buffer a step reads, a ticket word or the derived state (materialise_pstar apart, which pbf_surface and
// PBF_BUF_PSTAR do alike): a step after it makes the launches and takes the graph it would have without.
static_assert(sizeof(pbf_diag) == 27 * 8 && offsetof(DiagRecord, seq) == sizeof(pbf_diag) &&
                  offsetof(pbf_diag, mass) == offsetof(DiagRecord, mass) &&
                  offsetof(pbf_diag, n_density) == offsetof(DiagRecord, n_density) &&
                  offsetof(pbf_diag, nbr_mean) == offsetof(DiagRecord, nbr_mean),
              "DiagRecord (pbf_kernels.hpp) is pbf_diag followed by the polled word");
template <typename N, bool FAST> int density_pass(pbf_ctx *ctx, const StepConsts<N> &c) {
  const int s = ctx->st.cur;
  typename DensityOp<N, FAST>::Args a{ctx->pstar[ctx->st.pcur].as<const vec4<N>>(), ctx->pos4[s].as<const vec4<N>>(),
                                      ctx->type[s].as<const uint8_t>(), ctx->diagRho.as<N>(), ctx->diagNbr.as<uint32_t>()};
  return launch_gather<N, DensityOp<N, FAST>>(ctx, c, a);
}
template <typename N> int diagnostics_impl(pbf_ctx *ctx, const pbf_params *p, bool density, pbf_diag *out) {
  StepConsts<N> c;
  if (density)
    if (int rc = consts_on_last_grid<N>(ctx, p, c, "pbf_diagnostics")) return rc;
  if (int rc = ensure_diag(ctx, /*first=*/true, density)) return rc;
  uint32_t seq;
  HIPCHK(ctx, ctx->hostDiag.arm(seq));
  const int s = ctx->st.cur;
  const uint32_t n = uint32_t(ctx->n), nb = (n + DIAG_TILE - 1) / DIAG_TILE;
  if (density && n) {
    if (int rc = materialise_pstar<N>(ctx)) return rc;
    if (int rc = DISPATCH_FAST(ctx, density_pass, ctx, c)) return rc;
    ctx->diagRhoAt = ctx->orderEpoch;
  }
  if (nb)
    hipLaunchKernelGGL((k_diag_partial<N>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n, ctx->pos4[s].as<const vec4<N>>(),
                       ctx->vel4[s].as<const vec4<N>>(), ctx->type[s].as<const uint8_t>(),
                       density ? ctx->diagRho.as<const N>() : static_cast<const N *>(nullptr),
                       ctx->diagNbr.as<const uint32_t>(), ctx->diagPartials.as<DiagPartial>());
  hipLaunchKernelGGL(k_diag_final, dim3(1), dim3(BLOCK), 0, ctx->stream, nb, ctx->diagPartials.as<const DiagPartial>(),
                     ctx->hostDiag.rec.p, seq);
  LAUNCH_CHECK(ctx);
  return receive(ctx, ctx->hostDiag, "diagnostics read-back", *out);
}

template <typename N>
int query_impl(pbf_ctx *ctx, const pbf_params *p, size_t np, const double *points, uint32_t *counts, uint64_t *ids, size_t cap) {
  StepConsts<N> c;
  if (int rc = consts_on_last_grid<N>(ctx, p, c, "pbf_query_cells")) return rc;
  std::vector<N> pts(3 * np);
  for (size_t k = 0; k < 3 * np; ++k) pts[k] = N(points[k]);
  if (int rc = ensure(ctx, ctx->queryPoints, pts.size() * sizeof(N))) return rc;
  if (int rc = ensure(ctx, ctx->queryCounts, np * 4)) return rc;
  if (int rc = ensure(ctx, ctx->queryIds, std::max<size_t>(np * cap, 1) * 8)) return rc;
  if (int rc = join_diffuse(ctx)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->queryPoints.p, pts.data(), pts.size() * sizeof(N), hipMemcpyHostToDevice, ctx->stream));
  const int s = ctx->st.cur;
  hipLaunchKernelGGL((k_query_cells<N>), dim3(unsigned(np)), dim3(64), 0, ctx->stream, c, ctx->queryPoints.as<const N>(),
                     ctx->table.as<const uint32_t>(), ctx->type[s].as<const uint8_t>(), ctx->id[s].as<const uint64_t>(),
                     ctx->queryCounts.as<uint32_t>(), ctx->queryIds.as<uint64_t>(), uint32_t(cap));
  LAUNCH_CHECK(ctx);
  std::vector<uint64_t> rows(ids && cap ? np * cap : 0);
  HIPCHK(ctx, hipMemcpyAsync(counts, ctx->queryCounts.p, np * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (!rows.empty()) HIPCHK(ctx, hipMemcpyAsync(rows.data(), ctx->queryIds.p, np * cap * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (pts and rows are temporaries; the caller reads the answers)
  if (!rows.empty())  // only what the kernel wrote reaches the caller: the rest of each row stays as it was
    for (size_t q = 0; q < np; ++q)
      std::memcpy(ids + q * cap, rows.data() + q * cap, std::min<size_t>(counts[q], cap) * 8);
  return PBF_OK;
}

// pbf_sample_points / pbf_sample_lattice: one k_sample launch over the final pStar on the last step's keys and table.  Like
// pbf_diagnostics it touches nothing a step reads (materialise_pstar apart) and is never captured.  `points` == nullptr: the
// lattice source.  The answers travel with plain async copies straight into the caller's arrays, only those it asked for.
struct SampleLatticeDesc {
  double origin[3], spacing[3];
  uint64_t dims[3];
};
// An observer's SoA outputs as planes of ONE device allocation, each 256-byte aligned: add() them all, allocate `bytes`, set
// `base`; then at() is a plane's address and back() copies a plane into the caller's array if it asked for one.
struct Planes {
  size_t bytes = 0;
  char *base = nullptr;
  size_t add(size_t n) {
    const size_t here = bytes;
    bytes += (n + 255) / 256 * 256;
    return here;
  }
  template <typename T> T *at(size_t plane) const { return reinterpret_cast<T *>(base + plane); }
  hipError_t back(void *host, size_t plane, size_t n, hipStream_t stream) const {
    return host ? hipMemcpyAsync(host, base + plane, n, hipMemcpyDeviceToHost, stream) : hipSuccess;
  }
};
// k_sample's outputs for up to `n` points of `esz`-byte elements, in SampleOut's order; `colour`: mc among them
struct SamplePlanes : Planes {
  size_t rho, weight, mv, mc, count, outside;
  bool colour;
  SamplePlanes(size_t n, size_t esz, bool withColour) : colour(withColour) {
    rho = add(n * esz), weight = add(n * esz), mv = add(3 * n * esz), mc = colour ? add(4 * n * esz) : 0;
    count = add(2 * n * 4), outside = add(n);
  }
  template <typename N> SampleOut<N> in(const DevBuf &b) {
    base = b.as<char>();
    return SampleOut<N>{at<N>(rho), at<N>(weight), at<N>(mv), colour ? at<N>(mc) : nullptr, at<uint32_t>(count),
                        at<uint8_t>(outside)};
  }
};
template <typename N, bool FAST, typename Source>
int launch_sample(pbf_ctx *ctx, const StepConsts<N> &c, const Source &src, uint64_t threads, uint32_t what,
                  const SampleOut<N> &out) {
  const int s = ctx->st.cur;
  const dim3 grid(unsigned((threads + BLOCK - 1) / BLOCK));
  const SampleExtent ext{{uint32_t(ctx->extent[0]), uint32_t(ctx->extent[1]), uint32_t(ctx->extent[2])}};
#define PBF_SAMPLE_LAUNCH(W)                                                                                              \
  hipLaunchKernelGGL((k_sample<N, FAST, W, Source>), grid, dim3(BLOCK), 0, ctx->stream, c, src, ext,                      \
                     ctx->table.as<const uint32_t>(), ctx->pstar[ctx->st.pcur].as<const vec4<N>>(),                       \
                     ctx->pos4[s].as<const vec4<N>>(), ctx->vel4[s].as<const vec4<N>>(), ctx->col4[s].as<const vec4<N>>(), \
                     ctx->type[s].as<const uint8_t>(), out)
  switch (what) {
    case 0: PBF_SAMPLE_LAUNCH(0u); break;
    case SAMPLE_VELOCITY: PBF_SAMPLE_LAUNCH(SAMPLE_VELOCITY); break;
    case SAMPLE_COLOUR: PBF_SAMPLE_LAUNCH(SAMPLE_COLOUR); break;
    default: PBF_SAMPLE_LAUNCH(SAMPLE_VELOCITY | SAMPLE_COLOUR); break;
  }
#undef PBF_SAMPLE_LAUNCH
  LAUNCH_CHECK(ctx);
  return PBF_OK;
}
template <typename N>
int sample_impl(pbf_ctx *ctx, const pbf_params *p, size_t n, const double *points, const SampleLatticeDesc *lat, uint32_t what,
                const pbf_sample_out *o, const char *who) {
  StepConsts<N> c;
  if (int rc = consts_on_last_grid<N>(ctx, p, c, who)) return rc;
  SamplePlanes l(n, sizeof(N), /*withColour=*/true);
  if (int rc = ensure(ctx, ctx->sampleOut, l.bytes)) return rc;
  std::vector<N> pts;
  if (points) {
    pts.resize(3 * n);
    for (size_t k = 0; k < 3 * n; ++k) pts[k] = N(points[k]);
    if (int rc = ensure(ctx, ctx->samplePoints, pts.size() * sizeof(N))) return rc;
  }
  if (int rc = join_diffuse(ctx)) return rc;
  if (int rc = materialise_pstar<N>(ctx)) return rc;
  const SampleOut<N> out = l.in<N>(ctx->sampleOut);
  int rc;
  if (points) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->samplePoints.p, pts.data(), pts.size() * sizeof(N), hipMemcpyHostToDevice, ctx->stream));
    const SamplePointSource<N> src{ctx->samplePoints.as<const N>(), uint32_t(n)};
    rc = DISPATCH_FAST(ctx, launch_sample, ctx, c, src, n, what, out);
  } else {
    SampleLatticeSource<N> src;
    for (int a = 0; a < 3; ++a) src.origin[a] = N(lat->origin[a]), src.spacing[a] = N(lat->spacing[a]), src.dims[a] = uint32_t(lat->dims[a]);
    src.by = (src.dims[1] + 3u) / 4u, src.bz = (src.dims[2] + 3u) / 4u;
    const uint64_t waves = uint64_t((src.dims[0] + 3u) / 4u) * src.by * src.bz;  // (at most 2^29: dims' product is below 2^31)
    rc = DISPATCH_FAST(ctx, launch_sample, ctx, c, src, waves * 64u, what, out);
  }
  if (rc != PBF_OK) return rc;
  HIPCHK(ctx, l.back(o->rho, l.rho, n * sizeof(N), ctx->stream));
  HIPCHK(ctx, l.back(o->weight, l.weight, n * sizeof(N), ctx->stream));
  HIPCHK(ctx, l.back(o->mv, l.mv, 3 * n * sizeof(N), ctx->stream));
  HIPCHK(ctx, l.back(o->mc, l.mc, 4 * n * sizeof(N), ctx->stream));
  HIPCHK(ctx, l.back(o->count, l.count, 2 * n * 4, ctx->stream));
  HIPCHK(ctx, l.back(o->outside, l.outside, n, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (pts is a temporary; the caller reads the answers)
  return PBF_OK;
}
// what both entry points refuse, in the header's order: arguments first (PBF_ERR_INVALID), then the state (PBF_ERR_STATE)
int sample_check(pbf_ctx *ctx, const pbf_params *p, uint32_t what, const pbf_sample_out *o, const char *who) {
  const std::string w(who);
  if (!p || !o) return fail(ctx, PBF_ERR_INVALID, w + ": NULL argument");
  const Refuse refuse{ctx, who};
  if (int rc = refuse.params(p)) return rc;
  if (o->mv && !(what & PBF_SAMPLE_VELOCITY)) return fail(ctx, PBF_ERR_INVALID, w + ": mv needs PBF_SAMPLE_VELOCITY");
  if (o->mc && !(what & PBF_SAMPLE_COLOUR)) return fail(ctx, PBF_ERR_INVALID, w + ": mc needs PBF_SAMPLE_COLOUR");
  if (int rc = refuse.slab_mode()) return rc;  // (a point near a cut needs both ranks' candidates)
  return refuse.no_step();
}

// pbf_anisotropy_compute: one AnisotropyOp launch over the final pStar on the last step's keys and table, through whichever
// gather kernel the ctx is set to.  Like pbf_sample_points it touches nothing a step reads (materialise_pstar apart), takes no
// ticket word and is never captured; the arrays asked for travel with plain async copies straight into the caller's memory.
// AnisotropyOp's outputs in ctx->anisoOut: the planes are sized to the capacity; a plane has n elements
struct AnisoPlanes : Planes {
  size_t centre, G, axes, radii, nbr;
  AnisoPlanes(size_t cap, size_t esz) {
    centre = add(3 * cap * esz), G = add(6 * cap * esz), axes = add(9 * cap * esz), radii = add(3 * cap * esz), nbr = add(cap * 4);
  }
};
// the launch alone: pbf_anisotropy_compute copies the planes back, pbf_surface_anisotropic packs them on the device
template <typename N, bool FAST>
int anisotropy_launch(pbf_ctx *ctx, const StepConsts<N> &c, const pbf_anisotropy *g, AnisoPlanes &l) {
  if (int rc = ensure(ctx, ctx->anisoOut, l.bytes)) return rc;
  if (int rc = join_diffuse(ctx)) return rc;
  if (int rc = materialise_pstar<N>(ctx)) return rc;
  l.base = ctx->anisoOut.as<char>();
  const int s = ctx->st.cur;
  const AnisoConsts<N> k{N(g->smoothing), N(g->k_r), N(g->k_s), N(g->k_n), g->min_neighbours};
  typename AnisotropyOp<N, FAST>::Args a{ctx->pstar[ctx->st.pcur].as<const vec4<N>>(), ctx->pos4[s].as<const vec4<N>>(),
                                         ctx->type[s].as<const uint8_t>(), l.at<N>(l.centre), l.at<N>(l.G), l.at<N>(l.axes),
                                         l.at<N>(l.radii), l.at<uint32_t>(l.nbr), k};
  return launch_gather<N, AnisotropyOp<N, FAST>>(ctx, c, a);
}
template <typename N, bool FAST>
int anisotropy_pass(pbf_ctx *ctx, const StepConsts<N> &c, const pbf_anisotropy *g, const pbf_anisotropy_out *o) {
  const size_t n = ctx->n;
  AnisoPlanes l(ctx->cap, sizeof(N));
  if (int rc = anisotropy_launch<N, FAST>(ctx, c, g, l)) return rc;
  HIPCHK(ctx, l.back(o->centre, l.centre, 3 * n * sizeof(N), ctx->stream));
  HIPCHK(ctx, l.back(o->G, l.G, 6 * n * sizeof(N), ctx->stream));
  HIPCHK(ctx, l.back(o->axes, l.axes, 9 * n * sizeof(N), ctx->stream));
  HIPCHK(ctx, l.back(o->radii, l.radii, 3 * n * sizeof(N), ctx->stream));
  HIPCHK(ctx, l.back(o->neighbours, l.nbr, n * 4, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PBF_OK;
}
// what pbf_anisotropy_compute and pbf_surface_anisotropic reject in a pbf_anisotropy alike
const char *anisotropy_config_error(const pbf_anisotropy *g) {
  if (!(g->smoothing >= 0 && g->smoothing <= 1)) return "smoothing must lie in [0, 1]";
  if (!(g->k_r >= 1) || !std::isfinite(g->k_r)) return "k_r must be finite and >= 1";
  if (!(g->k_s > 0) || !std::isfinite(g->k_s) || !(g->k_n > 0) || !std::isfinite(g->k_n)) return "k_s and k_n must be finite and > 0";
  return nullptr;
}
template <typename N> int anisotropy_impl(pbf_ctx *ctx, const pbf_params *p, const pbf_anisotropy *g, const pbf_anisotropy_out *o) {
  StepConsts<N> c;
  if (int rc = consts_on_last_grid<N>(ctx, p, c, "pbf_anisotropy_compute")) return rc;
  return DISPATCH_FAST(ctx, anisotropy_pass, ctx, c, g, o);
}

// pbf_whitewater_*: see csrc/pbf_whitewater.hpp for the passes.  Like pbf_diagnostics it reads what the last step left and
// writes only buffers of its own (materialise_pstar apart): no ticket word, no derived state, no stage timer — a step after
// it makes the launches and takes the graph it would have without.
static_assert(sizeof(pbf_whitewater_stats) == 7 * 8 && offsetof(WwRecord, seq) == sizeof(pbf_whitewater_stats) &&
                  offsetof(pbf_whitewater_stats, kind) == offsetof(WwRecord, kind),
              "WwRecord (pbf_whitewater.hpp) is pbf_whitewater_stats followed by the polled word");
template <typename N> WwPool<N> ww_pool(pbf_ctx *ctx, int set) {
  return WwPool<N>{ctx->wwPos[set].as<vec4<N>>(), ctx->wwVel[set].as<vec4<N>>(), ctx->wwKind[set].as<uint8_t>(),
                   ctx->wwParent[set].as<uint64_t>()};
}
template <typename N> WwConsts<N> ww_consts(const pbf_ctx *ctx) {
  const pbf_whitewater &g = ctx->ww;
  WwConsts<N> w;
  w.kTa = N(g.k_ta), w.kWc = N(g.k_wc), w.kB = N(g.k_b), w.kD = N(g.k_d);
  for (int k = 0; k < 2; ++k)
    w.tauTa[k] = N(g.tau_ta[k]), w.tauWc[k] = N(g.tau_wc[k]), w.tauK[k] = N(g.tau_k[k]), w.life[k] = N(g.lifetime[k]);
  w.sprayBelow = g.spray_below, w.bubbleFrom = g.bubble_from;
  w.seed = g.seed, w.frame = ctx->wwFrame;
  return w;
}
// the pool's own buffers, sized to its capacity (pbf_whitewater_configure); k_sample's SoA outputs in one allocation
int ww_resize_pool(pbf_ctx *ctx, size_t cap) {
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  DevBuf *pool[] = {&ctx->wwPos[0], &ctx->wwPos[1], &ctx->wwVel[0], &ctx->wwVel[1], &ctx->wwKind[0], &ctx->wwKind[1],
                    &ctx->wwParent[0], &ctx->wwParent[1], &ctx->wwSample, &ctx->wwAlive, &ctx->wwAliveOff, &ctx->wwSums};
  for (DevBuf *b : pool) HIPCHK(ctx, b->reset());
  ctx->wwCount = 0, ctx->wwCur = 0;
  if (!cap) return PBF_OK;
  const size_t v = ctx->fp64 ? sizeof(double4) : sizeof(float4), esz = v / 4;
  for (int s = 0; s < 2; ++s) {
    if (int rc = ensure(ctx, ctx->wwPos[s], cap * v)) return rc;
    if (int rc = ensure(ctx, ctx->wwVel[s], cap * v)) return rc;
    if (int rc = ensure(ctx, ctx->wwKind[s], cap)) return rc;
    if (int rc = ensure(ctx, ctx->wwParent[s], cap * 8)) return rc;
  }
  if (int rc = ensure(ctx, ctx->wwSample, SamplePlanes(cap, esz, /*withColour=*/false).bytes)) return rc;
  if (int rc = ensure(ctx, ctx->wwAlive, (cap + SCAN_TILE) * 4)) return rc;
  return ensure(ctx, ctx->wwAliveOff, (cap + SCAN_TILE) * 4);
}

// pbf_set_whitewater_solids: the buffers its kernels write, allocated where the setting or the pool's capacity changes and
// never inside a step.  Partials: 3 words per workgroup of k_ww_solids, then one per workgroup of k_ww_solids_children.
size_t ww_solids_pool_blocks(const pbf_ctx *ctx) { return grid_for(size_t(ctx->ww.capacity)).x; }
int ww_solids_buffers(pbf_ctx *ctx) {
  if (!ctx->wwSolidsOn || !ctx->wwOn) return PBF_OK;
  if (int rc = ensure(ctx, ctx->wwSolidsPartials, (3 * ww_solids_pool_blocks(ctx) + wwsolids::CHILD_BLOCKS) * 4)) return rc;
  return ensure(ctx, ctx->wwSolidsRec, sizeof(WwSolidsRecord));
}
static_assert(sizeof(pbf_whitewater_solids) == 24 && sizeof(struct pbf_whitewater_solids_stats) == 5 * 8 &&
                  sizeof(WwSolidsRecord) == sizeof(struct pbf_whitewater_solids_stats),
              "WwSolidsRecord (pbf_whitewater_solids.hpp) is pbf_whitewater_solids_stats");
// the solids as the whitewater kernels take them, and which instantiation reads them: bit 0 a collider, 1 its pose record,
// 2 a solid velocity (a body, else friction), 3 the scenery.  0: neither lattice is installed, nothing is launched.
template <typename N> int ww_solids_args(pbf_ctx *ctx, const StepConsts<N> &c, WwSolidsArgs<N> &a) {
  const bool col = collider_on(ctx), scn = scenery_on(ctx);
  const bool posed = col && ctx->col.posed, vel = col && (ctx->col.body || ctx->col.friction);
  a = WwSolidsArgs<N>{};
  if (col) a.collider = sdf_args<N>(ctx->solid[ColliderState::COLLIDER]);
  if (scn) a.scenery = sdf_args<N>(ctx->solid[ColliderState::SCENERY]);
  if (posed || vel) a.pose = ctx->colliderPose.as<const ColliderPose<N>>();
  if (vel)  // (addresses only, as stage_friction forms them)
    a.vw = ctx->col.body ? ctx->bodyRec.as<const colliderbody::Record>()->st.velocity
                         : ctx->frictionRec.as<const pbf_collider_friction>()->velocity;
  a.frame.scale = c.scale;
  for (int k = 0; k < 3; ++k) a.frame.minB[k] = c.minB[k], a.frame.maxB[k] = c.maxB[k];
  a.e = N(ctx->wwSolids.restitution), a.f = N(ctx->wwSolids.friction), a.absorb = ctx->wwSolids.absorb;
  return int(col) | int(posed) << 1 | int(vel) << 2 | int(scn) << 3;
}
template <typename N>
void ww_solids_pool(pbf_ctx *ctx, int mode, const WwSolidsArgs<N> &a, uint32_t m, const WwPool<N> &pool, const N *weight,
                    const uint32_t *count, uint32_t *alive, uint32_t *partials) {
#define WW_SOLIDS_CASE(COL, POSED, VEL, SCN)                                                                                  \
  case (COL | POSED << 1 | VEL << 2 | SCN << 3):                                                                              \
    hipLaunchKernelGGL((k_ww_solids<N, COL != 0, POSED != 0, VEL != 0, SCN != 0>), grid_for(m), dim3(BLOCK), 0, ctx->stream, \
                       a, m, pool, weight, count, alive, partials);                                                           \
    break;
  switch (mode) {
    WW_SOLIDS_CASE(0, 0, 0, 1)
    WW_SOLIDS_CASE(1, 0, 0, 0)
    WW_SOLIDS_CASE(1, 1, 0, 0)
    WW_SOLIDS_CASE(1, 0, 1, 0)
    WW_SOLIDS_CASE(1, 1, 1, 0)
    WW_SOLIDS_CASE(1, 0, 0, 1)
    WW_SOLIDS_CASE(1, 1, 0, 1)
    WW_SOLIDS_CASE(1, 0, 1, 1)
    WW_SOLIDS_CASE(1, 1, 1, 1)
  }
#undef WW_SOLIDS_CASE
}
template <typename N>
void ww_solids_children(pbf_ctx *ctx, int mode, const WwSolidsArgs<N> &a, uint32_t n, const uint32_t *emit, const uint32_t *offset,
                        uint32_t m, const uint32_t *alive, const uint32_t *aliveOff, uint32_t cap, vec4<N> *pos4, uint32_t *partials) {
#define WW_SOLIDS_CASE(COL, POSED, SCN)                                                                                    \
  case (COL | POSED << 1 | SCN << 3):                                                                                      \
    hipLaunchKernelGGL((k_ww_solids_children<N, COL != 0, POSED != 0, SCN != 0>), dim3(wwsolids::CHILD_BLOCKS), dim3(BLOCK), \
                       0, ctx->stream, a, n, emit, offset, m, alive, aliveOff, cap, pos4, partials);                        \
    break;
  switch (mode & ~4) {  // (a child's velocity is kept: no solid velocity is read)
    WW_SOLIDS_CASE(0, 0, 1)
    WW_SOLIDS_CASE(1, 0, 0)
    WW_SOLIDS_CASE(1, 1, 0)
    WW_SOLIDS_CASE(1, 0, 1)
    WW_SOLIDS_CASE(1, 1, 1)
  }
#undef WW_SOLIDS_CASE
}

template <typename N, bool FAST> int whitewater_passes(pbf_ctx *ctx, const StepConsts<N> &c, uint32_t seq) {
  const int s = ctx->st.cur, ws = ctx->wwCur, wd = 1 - ws;
  const uint32_t n = uint32_t(ctx->n), m = uint32_t(ctx->wwCount), cap = uint32_t(ctx->ww.capacity);
  const WwConsts<N> w = ww_consts<N>(ctx);
  const WwPool<N> src = ww_pool<N>(ctx, ws), dst = ww_pool<N>(ctx, wd);
  uint32_t *alive = ctx->wwAlive.as<uint32_t>(), *aliveOff = ctx->wwAliveOff.as<uint32_t>();
  uint32_t *emit = ctx->wwEmit.as<uint32_t>(), *offset = ctx->wwOffset.as<uint32_t>();
  // pbf_set_whitewater_solids: the pool against the lattices installed right now (solidsMode 0: none, nothing more is launched)
  WwSolidsArgs<N> solids{};
  const int solidsMode = ctx->wwSolidsOn ? ww_solids_args<N>(ctx, c, solids) : 0;
  uint32_t *poolPartials = ctx->wwSolidsPartials.as<uint32_t>();
  uint32_t *childPartials = ctx->wwSolidsOn ? poolPartials + 3 * ww_solids_pool_blocks(ctx) : nullptr;
  if (m) {  // 1: advect what is in the pool on the state the last step left
    const SampleOut<N> out = SamplePlanes(cap, sizeof(N), /*withColour=*/false).in<N>(ctx->wwSample);
    const WwPoolSource<N> from{src.pos4, m};
    if (int rc = launch_sample<N, FAST>(ctx, c, from, m, SAMPLE_VELOCITY, out)) return rc;
    hipLaunchKernelGGL((k_ww_advect<N>), grid_for(m), dim3(BLOCK), 0, ctx->stream, c, w, m, src, out.weight, out.mv, out.count,
                       alive);
    if (solidsMode) ww_solids_pool<N>(ctx, solidsMode, solids, m, src, out.weight, out.count, alive, poolPartials);
    LAUNCH_CHECK(ctx);
  }
  if (n) {  // 2, 3: normals into the whitewater state's own fields, then the potentials and the child counts
    SurfArgs<N> a{};
    a.pstar = ctx->pstar[ctx->st.pcur].as<const vec4<N>>(), a.pos4 = ctx->pos4[s].as<const vec4<N>>();
    a.type = ctx->type[s].as<const uint8_t>();
    a.fieldOut = ctx->wwFieldA.as<vec4<N>>();
    if (int rc = launch_gather<N, SurfaceDensityOp<N, FAST>>(ctx, c, a)) return rc;
    a.fieldIn = ctx->wwFieldA.as<const vec4<N>>(), a.fieldOut = ctx->wwFieldB.as<vec4<N>>();
    if (int rc = launch_gather<N, SurfaceNormalOp<N, FAST>>(ctx, c, a)) return rc;
    typename WhitewaterOp<N, FAST>::Args wa{a.pstar, a.pos4, ctx->vel4[s].as<const vec4<N>>(), ctx->wwFieldB.as<const vec4<N>>(),
                                            a.type, ctx->id[s].as<const uint64_t>(), ctx->wwPot.as<vec4<N>>(), emit,
                                            ctx->wwChildKind.as<uint8_t>(), w};
    if (int rc = launch_gather<N, WhitewaterOp<N, FAST>>(ctx, c, wa)) return rc;
  }
  // 4, 5: both exclusive scans in one set of launches — the child counts in device order, the survivor flags in pool order
  ScanJobs jobs{};
  int njobs = 0;
  uint32_t *sums = ctx->wwSums.as<uint32_t>();
  auto add_job = [&](const uint32_t *count, uint32_t len, uint32_t *table) {
    jobs.count[njobs] = count, jobs.table[njobs] = table, jobs.len[njobs] = len, jobs.sums[njobs] = sums;
    jobs.nb[njobs] = (len + SCAN_TILE - 1) / SCAN_TILE;
    sums += jobs.nb[njobs];
    ++njobs;
  };
  if (n) add_job(emit, n, offset);
  if (m) add_job(alive, m, aliveOff);
  if (njobs) launch_scans(ctx, jobs, njobs);
  if (m) hipLaunchKernelGGL((k_ww_move<N>), grid_for(m), dim3(BLOCK), 0, ctx->stream, m, src, alive, aliveOff, dst);
  if (n)
    hipLaunchKernelGGL((k_ww_emit<N>), grid_for(n), dim3(BLOCK), 0, ctx->stream, c, w, ctx->pos4[s].as<const vec4<N>>(),
                       ctx->vel4[s].as<const vec4<N>>(), ctx->id[s].as<const uint64_t>(), ctx->wwPot.as<const vec4<N>>(), emit,
                       offset, ctx->wwChildKind.as<const uint8_t>(), m, alive, aliveOff, cap, dst);
  if (n && solidsMode) ww_solids_children<N>(ctx, solidsMode, solids, n, emit, offset, m, alive, aliveOff, cap, dst.pos4, childPartials);
  if (solidsMode)
    hipLaunchKernelGGL(k_ww_solids_fold, dim3(1), dim3(BLOCK), 0, ctx->stream, m ? grid_for(m).x : 0u, poolPartials,
                       n ? wwsolids::CHILD_BLOCKS : 0u, childPartials, (unsigned long long)(ctx->wwSolidsSteps + 1),
                       ctx->wwSolidsRec.as<WwSolidsRecord>());
  ctx->wwSolidsFolded = solidsMode != 0;  // (no lattice: nothing was launched, and the stats are zero on the host's side)
  hipLaunchKernelGGL(k_ww_final, dim3(1), dim3(BLOCK), 0, ctx->stream, n, emit, offset, m, alive, aliveOff, cap, dst.kind,
                     ctx->hostWw.rec.p, seq);
  LAUNCH_CHECK(ctx);
  return PBF_OK;
}
template <typename N> int whitewater_step_impl(pbf_ctx *ctx, const pbf_params *p, pbf_whitewater_stats *out) {
  StepConsts<N> c;
  if (int rc = consts_on_last_grid<N>(ctx, p, c, "pbf_whitewater_step")) return rc;
  if (int rc = ensure_whitewater_fields(ctx)) return rc;
  const size_t nbSums = (ctx->cap + SCAN_TILE - 1) / SCAN_TILE + (size_t(ctx->ww.capacity) + SCAN_TILE - 1) / SCAN_TILE + 2;
  if (int rc = ensure(ctx, ctx->wwSums, nbSums * 4)) return rc;
  uint32_t seq;
  HIPCHK(ctx, ctx->hostWw.arm(seq));
  if (int rc = join_diffuse(ctx)) return rc;
  if (int rc = materialise_pstar<N>(ctx)) return rc;
  if (int rc = DISPATCH_FAST(ctx, whitewater_passes, ctx, c, seq)) return rc;
  pbf_whitewater_stats st;
  if (int rc = receive(ctx, ctx->hostWw, "whitewater read-back", st)) return rc;
  ctx->wwCount = size_t(st.alive), ctx->wwCur = 1 - ctx->wwCur, ctx->wwFrame++;
  if (ctx->wwSolidsOn) ctx->wwSolidsSteps++;
  ctx->wwPotAt = ctx->n ? ctx->orderEpoch : 0;
  if (out) *out = st;
  return PBF_OK;
}
template <typename N> int whitewater_upload_impl(pbf_ctx *ctx, size_t n, const N *pos, const N *vel, const N *life) {
  std::vector<vec4<N>> P(n), V(n);
  for (size_t i = 0; i < n; ++i) {
    P[i] = make_vec4<N>(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], life ? life[i] : N(ctx->ww.lifetime[1]));
    V[i] = vel ? make_vec4<N>(vel[3 * i], vel[3 * i + 1], vel[3 * i + 2], N(0)) : make_vec4<N>(N(0), N(0), N(0), N(0));
  }
  const int s = ctx->wwCur;
  if (n) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->wwPos[s].p, P.data(), n * sizeof(vec4<N>), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->wwVel[s].p, V.data(), n * sizeof(vec4<N>), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->wwKind[s].p, 0, n, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->wwParent[s].p, 0xFF, n * 8, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // P, V are temporaries
  }
  ctx->wwCount = n;
  return PBF_OK;
}
template <typename N> int whitewater_download_impl(pbf_ctx *ctx, N *pos, N *vel, N *life, uint8_t *kind, uint64_t *parent) {
  const size_t n = ctx->wwCount;
  if (!n) return PBF_OK;
  const int s = ctx->wwCur;
  std::vector<vec4<N>> tmp(n);
  if (pos || life) {
    HIPCHK(ctx, hipMemcpyAsync(tmp.data(), ctx->wwPos[s].p, n * sizeof(vec4<N>), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; ++i) {
      if (pos) pos[3 * i] = tmp[i].x, pos[3 * i + 1] = tmp[i].y, pos[3 * i + 2] = tmp[i].z;
      if (life) life[i] = tmp[i].w;
    }
  }
  if (vel) {
    HIPCHK(ctx, hipMemcpyAsync(tmp.data(), ctx->wwVel[s].p, n * sizeof(vec4<N>), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; ++i) vel[3 * i] = tmp[i].x, vel[3 * i + 1] = tmp[i].y, vel[3 * i + 2] = tmp[i].z;
  }
  if (kind) HIPCHK(ctx, hipMemcpyAsync(kind, ctx->wwKind[s].p, n, hipMemcpyDeviceToHost, ctx->stream));
  if (parent) HIPCHK(ctx, hipMemcpyAsync(parent, ctx->wwParent[s].p, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PBF_OK;
}
// what pbf_whitewater_configure refuses (the message, or NULL when the configuration is fine)
const char *whitewater_config_error(const pbf_whitewater *g) {
  auto pair = [](const double t[2]) { return std::isfinite(t[0]) && std::isfinite(t[1]) && t[1] > t[0]; };
  if (!std::isfinite(g->k_ta) || !std::isfinite(g->k_wc) || g->k_ta < 0 || g->k_wc < 0) return "k_ta and k_wc must be finite and >= 0";
  if (!pair(g->tau_ta) || !pair(g->tau_wc) || !pair(g->tau_k)) return "a tau range needs finite min < max";
  if (!std::isfinite(g->lifetime[0]) || !std::isfinite(g->lifetime[1]) || g->lifetime[1] < g->lifetime[0]) return "lifetime needs finite min <= max";
  if (!std::isfinite(g->k_b)) return "k_b must be finite";
  if (!(g->k_d >= 0 && g->k_d <= 1)) return "k_d must lie in [0, 1]";
  if (g->spray_below > g->bubble_from) return "spray_below must not exceed bubble_from";
  if (g->capacity >= (uint64_t(1) << 31)) return "capacity must be < 2^31";
  return nullptr;
}
}  // namespace

namespace {
template <typename N> int set_collider_impl(pbf_ctx *ctx, const char *who, const pbf_collider_sdf *sdf, size_t nodes, DevBuf &fresh) {
  const N *phi = static_cast<const N *>(sdf->phi);
  for (size_t k = 0; k < nodes; ++k)
    if (phi[k] != phi[k]) return fail(ctx, PBF_ERR_INVALID, std::string(who) + ": a NaN in phi");
  // an allocation of its own, exactly sized: the current lattice stays in place until the new one has arrived
  HIPCHK(ctx, hipMalloc(&fresh.p, nodes * sizeof(N)));
  fresh.cap = nodes * sizeof(N);
  ctx->allocEpoch++;
  HIPCHK(ctx, hipMemcpyAsync(fresh.p, phi, nodes * sizeof(N), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (phi is the caller's)
  return PBF_OK;
}
// what pbf_set_collider, pbf_sdf_from_mesh and pbf_set_collider_mesh refuse about a lattice, in one place and one order;
// margin and phi are the installing / uploading call's business.  *nodes receives the dims product.
int collider_lattice_check(pbf_ctx *ctx, const char *who, const pbf_collider_sdf *sdf, bool margin, bool phi, size_t *nodes) {
  const std::string w = std::string(who) + ": ";
  size_t n = 1;
  for (int a = 0; a < 3; ++a) {
    if (sdf->dims[a] < 2) return fail(ctx, PBF_ERR_INVALID, w + "every dim must be >= 2");
    if ((n *= sdf->dims[a]) >= (size_t(1) << 31)) return fail(ctx, PBF_ERR_INVALID, w + "2^31 nodes or more");
    if (!std::isfinite(sdf->origin[a])) return fail(ctx, PBF_ERR_INVALID, w + "origin must be finite");
  }
  if (!std::isfinite(sdf->spacing) || !(sdf->spacing > 0)) return fail(ctx, PBF_ERR_INVALID, w + "spacing must be finite and > 0");
  if (margin && (!std::isfinite(sdf->margin) || sdf->margin < 0)) return fail(ctx, PBF_ERR_INVALID, w + "margin must be finite and >= 0");
  if (phi && !sdf->phi) return fail(ctx, PBF_ERR_INVALID, w + "phi == NULL");
  if (int rc = collider_refuse_slab(ctx)) return rc;
  *nodes = n;
  return PBF_OK;
}

// The pose record at the identity: what the REACT kernels read while no pose is set (ColliderState::needs_identity_pose).
template <typename N> int collider_pose_store(pbf_ctx *ctx, const pbf_collider_pose *pose);
int collider_pose_identity(pbf_ctx *ctx) {
  pbf_collider_pose id{};
  id.rot[0] = id.rot[4] = id.rot[8] = 1.0;
  if (int rc = ensure(ctx, ctx->colliderPose, sizeof(ColliderPose<double>))) return rc;
  return ctx->fp64 ? collider_pose_store<double>(ctx, &id) : collider_pose_store<float>(ctx, &id);
}
// synchronise and destroy the captured steps: after an event of ColliderState that returned true none can be asked for again
int collider_drop_graphs(pbf_ctx *ctx) {
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (auto &g : ctx->graphs)
    if (g.second.exec) (void)hipGraphExecDestroy(g.second.exec);
  ctx->graphs.clear();
  return PBF_OK;
}
// Body contact off (pbf_set_collider_body_contact(NULL), a cleared body, a replaced or cleared collider, a cleared scenery):
// the step loses its passes, so the captured graphs go (which synchronises), then the buffers are freed.
int contact_clear(pbf_ctx *ctx) {
  if (!ctx->contact.cleared()) return PBF_OK;
  if (int rc = collider_drop_graphs(ctx)) return rc;
  HIPCHK(ctx, ctx->contactPoints.reset());
  HIPCHK(ctx, ctx->contactPartials.reset());
  HIPCHK(ctx, ctx->contactRec.reset());
  return PBF_OK;
}
// The one install path of both solids: `fresh` (the lattice on the device, empty when sdf == NULL clears) becomes the ctx's
// collider or scenery.  Every install moves the captured steps' key.  A collider and scenery together run
// DeltaOp<.., COLLIDE_REACT_SCENERY>, which writes the records: the call that completes the pair turns the reaction on if it
// is off — once the new lattice is on the device and BEFORE anything of the ctx is changed, so a failed allocation leaves
// everything as it was.  Clearing either solid leaves the reaction on, as a cleared body does.
int solid_install(pbf_ctx *ctx, ColliderState::Solid which, const pbf_collider_sdf *sdf, DevBuf &fresh) {
  if (ctx->col.install_needs_reaction(which, sdf != nullptr))
    if (int rc = pbf_set_collider_reaction(ctx, 1)) return rc;
  if (int rc = collider_drop_graphs(ctx)) return rc;  // (first: they hold the old lattice's address)
  if (which == ColliderState::COLLIDER || !sdf)  // (the points came from the old collider; without scenery there is nothing to touch)
    if (int rc = contact_clear(ctx)) return rc;
  ctx->solid[which].put(sdf, fresh);                  // (frees the old lattice)
  if (!(which == ColliderState::SCENERY ? ctx->col.scenery_installed(sdf != nullptr) : ctx->col.installed(sdf != nullptr)))
    return fail(ctx, PBF_ERR_STATE, "a collider beside scenery needs the reaction records");  // (enabled above: not reached)
  return ctx->col.needs_identity_pose() ? collider_pose_identity(ctx) : PBF_OK;
}
// pbf_set_collider / pbf_set_scenery: the lattice as given, uploaded into an allocation of its own, then installed
int set_solid(pbf_ctx *ctx, const char *who, ColliderState::Solid which, const pbf_collider_sdf *sdf) {
  if (!ctx) return PBF_ERR_INVALID;
  size_t nodes = 1;
  if (sdf)
    if (int rc = collider_lattice_check(ctx, who, sdf, true, true, &nodes)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevBuf fresh;
  if (sdf)
    if (int rc = ctx->fp64 ? set_collider_impl<double>(ctx, who, sdf, nodes, fresh) : set_collider_impl<float>(ctx, who, sdf, nodes, fresh))
      return rc;
  return solid_install(ctx, which, sdf, fresh);
}

// pbf_sdf_from_mesh / pbf_set_collider_mesh: the records on the host, then the fold on the device (csrc/pbf_mesh_sdf.hpp,
// launch_fold: bounded launches over triangle ranges) into `fresh` (N[nodes], an allocation of its own like pbf_set_collider's).
template <typename N>
int mesh_sdf_impl(pbf_ctx *ctx, const pbf_mesh *mesh, const pbf_collider_sdf *lat, uint32_t flags, size_t nodes, DevBuf &fresh,
                  pbf_mesh_sdf_stats *stats) {
  const size_t nt = size_t(mesh->n_triangles);
  const bool winding = (flags & PBF_MESH_SIGN_WINDING) != 0, negate = (flags & PBF_MESH_NEGATE) != 0;
  const int stride = winding ? meshsdf::SOUP_RECORD : meshsdf::RECORD;
  std::vector<N> rec(size_t(stride) * nt), bnd(4 * nt);
  const char *why = nullptr;
  const int built = winding ? meshsdf::build_soup_records(mesh, sizeof(N) == 8, rec.data(), nullptr, &why)
                            : meshsdf::build_records(mesh, sizeof(N) == 8, rec.data(), nullptr, &why);
  if (built != PBF_OK) return fail(ctx, PBF_ERR_INVALID, why);
  meshsdf::SdfLattice<N> L;
  N slack;
  meshsdf::prepare<N>(lat->dims, lat->origin, lat->spacing, rec.data(), nt, stride, &L, bnd.data(), &slack);
  const size_t bricks = meshsdf::brick_count(L);  // (< 2^31: at most the node count)

  DevBuf dRec, dBnd, dSign, dTested, dSum;
  if (winding) HIPCHK(ctx, hipMalloc(&dSum.p, nodes * sizeof(N)));
  HIPCHK(ctx, hipMalloc(&fresh.p, nodes * sizeof(N)));
  fresh.cap = nodes * sizeof(N);
  HIPCHK(ctx, hipMalloc(&dRec.p, rec.size() * sizeof(N)));
  HIPCHK(ctx, hipMalloc(&dBnd.p, bnd.size() * sizeof(N)));
  HIPCHK(ctx, hipMalloc(&dSign.p, nodes));
  HIPCHK(ctx, hipMalloc(&dTested.p, bricks * sizeof(uint64_t)));
  ctx->allocEpoch++;
  HIPCHK(ctx, hipMemcpyAsync(dRec.p, rec.data(), rec.size() * sizeof(N), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(dBnd.p, bnd.data(), bnd.size() * sizeof(N), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, meshsdf::launch_fold<N>(ctx->stream, L, dRec.as<const N>(), dBnd.as<const N>(), nt, ctx->sdfCull, negate, slack, fresh.as<N>(),
                                      dSign.as<uint8_t>(), dTested.as<unsigned long long>(), ctx->sdfLaunchPairs, winding));
  if (winding)  // the lattice holds best: the winding fold's last launch turns it into phi
    HIPCHK(ctx, meshsdf::launch_winding<N>(ctx->stream, L, dRec.as<const N>(), nt, meshsdf::FINISH_PHI, negate, dSum.as<N>(), fresh.as<N>(),
                                           ctx->sdfLaunchPairs));
  std::vector<uint64_t> slots(stats ? bricks : 0);
  if (stats) HIPCHK(ctx, hipMemcpyAsync(slots.data(), dTested.p, bricks * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (rec, bnd and the scratch buffers are locals)
  if (stats) {
    stats->pairs_total = uint64_t(nodes) * nt, stats->pairs_tested = 0;
    for (uint64_t v : slots) stats->pairs_tested += v;
  }
  return PBF_OK;
}
// the checks the two entry points share, then the fold
int mesh_sdf_run(pbf_ctx *ctx, const char *who, const pbf_mesh *mesh, const pbf_collider_sdf *lat, uint32_t flags, bool install,
                 DevBuf &fresh, size_t *nodes, pbf_mesh_sdf_stats *stats) {
  if (!lat) return fail(ctx, PBF_ERR_INVALID, std::string(who) + ": lattice == NULL");
  if (flags & ~uint32_t(PBF_MESH_NEGATE | PBF_MESH_SIGN_WINDING)) return fail(ctx, PBF_ERR_INVALID, std::string(who) + ": unknown flag bits");
  if (int rc = collider_lattice_check(ctx, who, lat, install, false, nodes)) return rc;
  {  // the mesh, before anything is allocated (mesh_sdf_impl builds the records of the ctx's type)
    const char *why = nullptr;
    const int rc = (flags & PBF_MESH_SIGN_WINDING) ? meshsdf::build_soup_records(mesh, 0, nullptr, nullptr, &why)
                                                   : meshsdf::build_records(mesh, 0, nullptr, nullptr, &why);
    if (rc != PBF_OK) return fail(ctx, PBF_ERR_INVALID, why);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return ctx->fp64 ? mesh_sdf_impl<double>(ctx, mesh, lat, flags, *nodes, fresh, stats)
                   : mesh_sdf_impl<float>(ctx, mesh, lat, flags, *nodes, fresh, stats);
}
// pbf_set_collider_mesh / pbf_set_scenery_mesh: the fold into an allocation of its own, then installed
int set_solid_mesh(pbf_ctx *ctx, const char *who, ColliderState::Solid which, const pbf_mesh *mesh, const pbf_collider_sdf *lattice,
                   uint32_t flags, pbf_mesh_sdf_stats *stats) {
  if (!ctx) return PBF_ERR_INVALID;
  DevBuf fresh;
  size_t nodes = 0;
  pbf_mesh_sdf_stats st{};
  if (int rc = mesh_sdf_run(ctx, who, mesh, lattice, flags, true, fresh, &nodes, &st)) return rc;
  if (int rc = solid_install(ctx, which, lattice, fresh)) return rc;
  if (stats) *stats = st;
  return PBF_OK;
}
// pbf_mesh_winding: the soup records on the host, the winding fold alone on the device, w copied to the caller's array
template <typename N> int mesh_winding_impl(pbf_ctx *ctx, const pbf_mesh *mesh, const pbf_collider_sdf *lat, size_t nodes, void *w) {
  const size_t nt = size_t(mesh->n_triangles);
  std::vector<N> rec(size_t(meshsdf::SOUP_RECORD) * nt);
  const char *why = nullptr;
  if (meshsdf::build_soup_records(mesh, sizeof(N) == 8, rec.data(), nullptr, &why) != PBF_OK) return fail(ctx, PBF_ERR_INVALID, why);
  meshsdf::SdfLattice<N> L;
  for (int a = 0; a < 3; ++a) L.dims[a] = lat->dims[a], L.bricks[a] = (lat->dims[a] + 3u) / 4u, L.origin[a] = N(lat->origin[a]);
  L.spacing = N(lat->spacing);
  DevBuf dRec, dSum;
  HIPCHK(ctx, hipMalloc(&dRec.p, rec.size() * sizeof(N)));
  HIPCHK(ctx, hipMalloc(&dSum.p, nodes * sizeof(N)));
  ctx->allocEpoch++;
  HIPCHK(ctx, hipMemcpyAsync(dRec.p, rec.data(), rec.size() * sizeof(N), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, meshsdf::launch_winding<N>(ctx->stream, L, dRec.as<const N>(), nt, meshsdf::FINISH_W, false, dSum.as<N>(), nullptr,
                                         ctx->sdfLaunchPairs));
  HIPCHK(ctx, hipMemcpyAsync(w, dSum.p, nodes * sizeof(N), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (rec and the device buffers are locals; w is the caller's)
  return PBF_OK;
}
// pbf_collider_reaction: the two launches of the sum and the polled read-back, as diagnostics_impl
static_assert(sizeof(struct pbf_collider_body_state) == 31 * 8 && offsetof(BodyStateRecord, seq) == sizeof(struct pbf_collider_body_state) &&
                  sizeof(colliderbody::Record) == (22 + 31) * 8,
              "the body record is doubles and 64-bit counters throughout (k_body_read copies it in 64-bit words)");
static_assert(sizeof(pbf_collider_wrench) == 15 * 8 && offsetof(WrenchRecord, seq) == sizeof(pbf_collider_wrench) &&
                  offsetof(pbf_collider_wrench, hits) == offsetof(WrenchRecord, hits) &&
                  offsetof(pbf_collider_wrench, step) == offsetof(WrenchRecord, step),
              "WrenchRecord (pbf_kernels.hpp) is pbf_collider_wrench followed by the polled word");
template <typename N> int collider_reaction_impl(pbf_ctx *ctx, pbf_collider_wrench *out) {
  uint32_t seq;
  HIPCHK(ctx, ctx->hostWrench.arm(seq));
  const uint32_t n = uint32_t(ctx->n), nb = (n + DIAG_TILE - 1) / DIAG_TILE;
  if (nb)
    hipLaunchKernelGGL((k_wrench_partial<N>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n, ctx->pushRec.as<const vec4<N>>(), push_slots(ctx),
                       ctx->pos4[ctx->st.cur].as<const vec4<N>>(), ctx->pushPartials.as<WrenchPartial>());
  hipLaunchKernelGGL(k_wrench_final, dim3(1), dim3(BLOCK), 0, ctx->stream, nb, ctx->pushPartials.as<const WrenchPartial>(),
                     ctx->pushCtl.as<const unsigned long long>(), ctx->hostWrench.rec.p, seq);
  LAUNCH_CHECK(ctx);
  return receive(ctx, ctx->hostWrench, "collider reaction read-back", *out);
}
// pbf_set_collider_pose: N(R), N(t) into the ctx's record by a one-lane kernel on the stream; no synchronisation
template <typename N> int collider_pose_store(pbf_ctx *ctx, const pbf_collider_pose *pose) {
  ColliderPose<N> v;
  for (int k = 0; k < 9; ++k) v.rot[k] = N(pose->rot[k]);
  for (int k = 0; k < 3; ++k) v.trans[k] = N(pose->trans[k]);
  hipLaunchKernelGGL((k_collider_pose_store<N>), dim3(1), dim3(1), 0, ctx->stream, v, ctx->colliderPose.as<ColliderPose<N>>());
  LAUNCH_CHECK(ctx);
  return PBF_OK;
}
template <typename N>
int collider_sample_impl(pbf_ctx *ctx, const ColliderSdf<N> &sdf, const ColliderPose<N> *pose, const pbf_params *p, size_t n,
                         const double *points, N *phi, N *moved, uint8_t *hit) {
  std::vector<N> pts(3 * n);
  for (size_t k = 0; k < 3 * n; ++k) pts[k] = N(points[k]);
  const size_t e = n * sizeof(N);
  if (int rc = ensure(ctx, ctx->samplePoints, 3 * e)) return rc;
  if (int rc = ensure(ctx, ctx->sampleOut, 4 * e + n)) return rc;  // {phi n, moved 3n, hit n bytes}
  char *out = ctx->sampleOut.as<char>();
  ColliderFrame<N> f;
  f.scale = N(p->scale);
  for (int a = 0; a < 3; ++a) f.minB[a] = N(p->min_bound[a]), f.maxB[a] = N(p->max_bound[a]);
  HIPCHK(ctx, hipMemcpyAsync(ctx->samplePoints.p, pts.data(), 3 * e, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL((k_collider_sample<N>), grid_for(n), dim3(BLOCK), 0, ctx->stream, sdf, pose, f, uint32_t(n),
                     ctx->samplePoints.as<const N>(), reinterpret_cast<N *>(out), reinterpret_cast<N *>(out + e),
                     reinterpret_cast<uint8_t *>(out + 4 * e));
  LAUNCH_CHECK(ctx);
  if (phi) HIPCHK(ctx, hipMemcpyAsync(phi, out, e, hipMemcpyDeviceToHost, ctx->stream));
  if (moved) HIPCHK(ctx, hipMemcpyAsync(moved, out + e, 3 * e, hipMemcpyDeviceToHost, ctx->stream));
  if (hit) HIPCHK(ctx, hipMemcpyAsync(hit, out + 4 * e, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (pts is a temporary; the caller reads the answers)
  return PBF_OK;
}
// pbf_set_collider_body_contact with a configuration that passed its checks, a body on and scenery installed.  The same level
// and stride as the points in place: the record alone is rewritten, by value, on the stream.  Otherwise the points are taken
// from the collider's lattice — count, scan, one read-back of the total, emit — into buffers of their own, and only when
// everything a step will need exists do they replace the ctx's: a refusal or a failed allocation leaves everything as it was.
template <typename N> int body_contact_configure(pbf_ctx *ctx, const pbf_body_contact *c) {
  if (ctx->contact.same_points(c->level, c->stride)) {
    hipLaunchKernelGGL(k_contact_store, dim3(1), dim3(1), 0, ctx->stream, bodycontact::record_of(*c, ctx->contact.points),
                       ctx->contactRec.as<bodycontact::Record>());
    LAUNCH_CHECK(ctx);
    ctx->contactCfg = *c;
    return ctx->contact.rewritten(c->iterations) ? collider_drop_graphs(ctx) : PBF_OK;  // (another number of passes: other launches)
  }
  const auto &lat = ctx->solid[ColliderState::COLLIDER];
  ColliderSdf<N> sdf = sdf_args<N>(lat);
  sdf.margin = N(c->level);
  ContactCells cells{};
  cells.stride = c->stride;
  uint64_t lanes = 1;
  for (int a = 0; a < 3; ++a) {
    cells.cells[a] = uint32_t((uint64_t(lat.dims[a]) - 2u) / c->stride + 1u);  // (ceil((dims - 1) / stride), dims >= 2)
    lanes *= cells.cells[a];
  }
  cells.lanes = uint32_t(lanes);  // (< 2^31: at most the node count)
  const uint32_t len = cells.lanes + 1, snb = (len + SCAN_TILE - 1) / SCAN_TILE;
  DevBuf counts, offsets, sums, points, partials, rec;
  HIPCHK(ctx, hipMalloc(&counts.p, (size_t(len) + SCAN_TILE) * 4));
  HIPCHK(ctx, hipMalloc(&offsets.p, (size_t(len) + SCAN_TILE) * 4));
  HIPCHK(ctx, hipMalloc(&sums.p, (size_t(snb) + 1) * 4));
  ctx->allocEpoch++;
  HIPCHK(ctx, hipMemsetAsync(counts.as<uint32_t>() + cells.lanes, 0, 4, ctx->stream));  // closing sentinel: offsets[lanes] = total
  hipLaunchKernelGGL((k_contact_count<N>), grid_for(cells.lanes), dim3(BLOCK), 0, ctx->stream, sdf, N(lat.spacing), cells, counts.as<uint32_t>());
  launch_scans(ctx, scan_job(counts.as<const uint32_t>(), len, sums.as<uint32_t>(), offsets.as<uint32_t>()), 1);
  LAUNCH_CHECK(ctx);
  uint32_t total = 0;
  HIPCHK(ctx, hipMemcpyAsync(&total, offsets.as<uint32_t>() + cells.lanes, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the point buffer is sized from the count
  if (total == 0) return fail(ctx, PBF_ERR_INVALID, "pbf_set_collider_body_contact: the lattice yields no point (no cell crosses the level)");
  const uint32_t nb = (total + DIAG_TILE - 1) / DIAG_TILE;
  HIPCHK(ctx, hipMalloc(&points.p, size_t(total) * 3 * sizeof(N)));
  points.cap = size_t(total) * 3 * sizeof(N);
  HIPCHK(ctx, hipMalloc(&partials.p, size_t(nb) * sizeof(ContactPartial)));
  partials.cap = size_t(nb) * sizeof(ContactPartial);
  HIPCHK(ctx, hipMalloc(&rec.p, sizeof(bodycontact::Record)));
  rec.cap = sizeof(bodycontact::Record);
  HIPCHK(ctx, ctx->hostContact.rec.ensure(1));  // (so that the observer allocates nothing either)
  hipLaunchKernelGGL((k_contact_emit<N>), grid_for(cells.lanes), dim3(BLOCK), 0, ctx->stream, sdf, N(lat.spacing), cells,
                     offsets.as<const uint32_t>(), total, points.as<N>());
  hipLaunchKernelGGL(k_contact_store, dim3(1), dim3(1), 0, ctx->stream, bodycontact::record_of(*c, total), rec.as<bodycontact::Record>());
  LAUNCH_CHECK(ctx);
  if (int rc = collider_drop_graphs(ctx)) return rc;  // (synchronises: the scan's scratch is local, and no replay holds the old buffers)
  ctx->contactPoints = std::move(points), ctx->contactPartials = std::move(partials), ctx->contactRec = std::move(rec);
  ctx->contactCfg = *c;
  ctx->contact.configured(total, c->iterations, c->level, c->stride);
  return PBF_OK;
}
}  // namespace

extern "C" {

int pbf_set_collider(pbf_ctx *ctx, const pbf_collider_sdf *sdf) { return set_solid(ctx, "pbf_set_collider", ColliderState::COLLIDER, sdf); }

int pbf_set_collider_pose(pbf_ctx *ctx, const pbf_collider_pose *pose) {
  if (!ctx) return PBF_ERR_INVALID;
  if (pose) {
    const char *why = nullptr;
    if (colliderpose::check(pose, &why) != PBF_OK) return fail(ctx, PBF_ERR_INVALID, why);
  }
  if (int rc = collider_needed(ctx, "pbf_set_collider_pose")) return rc;
  if (ctx->col.body)
    return fail(ctx, PBF_ERR_STATE, "pbf_set_collider_pose: a body is on and owns the pose (re-place it through pbf_set_collider_body)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (!pose) {  // back to the static kernels
    if (!ctx->col.pose_cleared()) return PBF_OK;
    if (int rc = collider_drop_graphs(ctx)) return rc;
    return ctx->col.needs_identity_pose() ? collider_pose_identity(ctx) : PBF_OK;
  }
  if (int rc = ensure(ctx, ctx->colliderPose, sizeof(ColliderPose<double>))) return rc;
  if (int rc = ctx->fp64 ? collider_pose_store<double>(ctx, pose) : collider_pose_store<float>(ctx, pose)) return rc;
  return ctx->col.pose_set() ? collider_drop_graphs(ctx) : PBF_OK;  // (an update changes no key and drops no graph)
}

int pbf_set_collider_reaction(pbf_ctx *ctx, int on) {
  if (!ctx) return PBF_ERR_INVALID;
  if (slab_ctx(ctx)) return fail(ctx, PBF_ERR_STATE, "the collider reaction is not supported in slab mode");
  const bool want = on != 0;
  if (want == ctx->col.reaction) return PBF_OK;
  if (!want && ctx->col.why_reaction_must_stay() == ColliderState::HELD_BY_BODY)
    return fail(ctx, PBF_ERR_STATE, "pbf_set_collider_reaction: a body is on and needs the records (pbf_set_collider_body(ctx, NULL) first)");
  if (!want && ctx->col.why_reaction_must_stay() == ColliderState::HELD_BY_FRICTION)
    return fail(ctx, PBF_ERR_STATE, "pbf_set_collider_reaction: friction is on and needs the records (pbf_set_collider_friction(ctx, NULL) first)");
  if (!want && ctx->col.why_reaction_must_stay() == ColliderState::HELD_BY_SCENERY)
    return fail(ctx, PBF_ERR_STATE, "pbf_set_collider_reaction: a collider beside scenery writes the records (clear either solid first)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (want) {  // everything a step will need exists before the event: the records, their counter, the pose the kernels read
    if (int rc = ensure_reaction(ctx)) return rc;
    if (int rc = ensure(ctx, ctx->pushCtl, 8)) return rc;
    if (!ctx->col.posed)
      if (int rc = collider_pose_identity(ctx)) return rc;
    if (hipMemsetAsync(ctx->pushCtl.p, 0, 8, ctx->stream) != hipSuccess) return fail(ctx, PBF_ERR_HIP, "pbf_set_collider_reaction: hipMemsetAsync failed");
  }
  // (other delta-p kernels, and the sort's clear comes or goes)
  return (want ? ctx->col.reaction_enabled() : ctx->col.reaction_disabled()) ? collider_drop_graphs(ctx) : PBF_OK;
}

int pbf_collider_reaction(pbf_ctx *ctx, pbf_collider_wrench *out) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!out) return fail(ctx, PBF_ERR_INVALID, "pbf_collider_reaction: out == NULL");
  if (!ctx->col.reaction) return fail(ctx, PBF_ERR_STATE, "pbf_collider_reaction: not enabled (pbf_set_collider_reaction)");
  if (int rc = collider_needed(ctx, "pbf_collider_reaction")) return rc;
  if (!push_current(ctx))
    return fail(ctx, PBF_ERR_STATE, "pbf_collider_reaction: no step since the reaction was enabled or the arrays last changed");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return ctx->fp64 ? collider_reaction_impl<double>(ctx, out) : collider_reaction_impl<float>(ctx, out);
}

int pbf_set_collider_body(pbf_ctx *ctx, const pbf_collider_body *body) {
  if (!ctx) return PBF_ERR_INVALID;
  if (body) {
    const char *why = nullptr;
    if (colliderbody::check(body, &why) != PBF_OK) return fail(ctx, PBF_ERR_INVALID, why);
  }
  if (int rc = collider_needed(ctx, "pbf_set_collider_body")) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (!body) {  // off: the solid stays where it is, as an ordinary pose; the reaction stays on (contact goes with the body)
    if (int rc = contact_clear(ctx)) return rc;
    return ctx->col.body_cleared() ? collider_drop_graphs(ctx) : PBF_OK;
  }
  if (int rc = pbf_set_collider_reaction(ctx, 1)) return rc;  // (a no-op when it is on already)
  if (int rc = ensure(ctx, ctx->colliderPose, sizeof(ColliderPose<double>))) return rc;
  if (int rc = ensure(ctx, ctx->bodyRec, sizeof(colliderbody::Record))) return rc;
  HIPCHK(ctx, ctx->hostBody.rec.ensure(1));  // (so that the observer allocates nothing either)
  const colliderbody::Record rec = colliderbody::record_of(*body);
  if (ctx->fp64)
    hipLaunchKernelGGL((k_body_store<double>), dim3(1), dim3(1), 0, ctx->stream, rec, ctx->bodyRec.as<colliderbody::Record>(),
                       ctx->colliderPose.as<ColliderPose<double>>());
  else
    hipLaunchKernelGGL((k_body_store<float>), dim3(1), dim3(1), 0, ctx->stream, rec, ctx->bodyRec.as<colliderbody::Record>(),
                       ctx->colliderPose.as<ColliderPose<float>>());
  // (with friction on, sums of a pass that ran before this call were taken against another pose and other velocities: the
  // body as placed here does not receive them)
  if (ctx->col.friction)
    hipLaunchKernelGGL(k_friction_pending_clear, dim3(1), dim3(1), 0, ctx->stream, ctx->frictionCtl.as<colliderfriction::Ctl>());
  if (ctx->contact.on)  // (a re-placed body keeps its contact and its points; the counters start again)
    hipLaunchKernelGGL(k_contact_store, dim3(1), dim3(1), 0, ctx->stream, bodycontact::record_of(ctx->contactCfg, ctx->contact.points),
                       ctx->contactRec.as<bodycontact::Record>());
  LAUNCH_CHECK(ctx);
  return ctx->col.body_set() ? collider_drop_graphs(ctx) : PBF_OK;  // (a re-placed body changes no key and drops no graph)
}

int pbf_collider_body_state(pbf_ctx *ctx, struct pbf_collider_body_state *out) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!out) return fail(ctx, PBF_ERR_INVALID, "pbf_collider_body_state: out == NULL");
  if (!ctx->col.body) return fail(ctx, PBF_ERR_STATE, "pbf_collider_body_state: no body set (pbf_set_collider_body)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  uint32_t seq;
  HIPCHK(ctx, ctx->hostBody.arm(seq));
  hipLaunchKernelGGL(k_body_read, dim3(1), dim3(1), 0, ctx->stream, ctx->bodyRec.as<const colliderbody::Record>(), ctx->hostBody.rec.p, seq);
  LAUNCH_CHECK(ctx);
  return receive(ctx, ctx->hostBody, "collider body read-back", *out);
}

static_assert(sizeof(struct pbf_body_contact_state) == 18 * 8 && offsetof(ContactStateRecord, seq) == sizeof(struct pbf_body_contact_state) &&
                  sizeof(bodycontact::Record) == (5 + 18) * 8,
              "the contact record is doubles and 64-bit counters throughout (k_contact_read copies it in 64-bit words)");
int pbf_set_collider_body_contact(pbf_ctx *ctx, const pbf_body_contact *contact) {
  if (!ctx) return PBF_ERR_INVALID;
  if (contact) {
    const char *why = nullptr;
    if (bodycontact::check(contact, &why) != PBF_OK) return fail(ctx, PBF_ERR_INVALID, why);
  }
  if (int rc = collider_refuse_slab(ctx)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (!contact) return contact_clear(ctx);
  if (!ctx->col.body) return fail(ctx, PBF_ERR_STATE, "pbf_set_collider_body_contact: no body set (pbf_set_collider_body)");
  if (!scenery_on(ctx)) return fail(ctx, PBF_ERR_STATE, "pbf_set_collider_body_contact: no scenery set (pbf_set_scenery)");
  return ctx->fp64 ? body_contact_configure<double>(ctx, contact) : body_contact_configure<float>(ctx, contact);
}

int pbf_collider_body_contact_points(pbf_ctx *ctx, uint64_t *n, void *points) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!n) return fail(ctx, PBF_ERR_INVALID, "pbf_collider_body_contact_points: n == NULL");
  if (!ctx->contact.on) return fail(ctx, PBF_ERR_STATE, "pbf_collider_body_contact_points: contact is off (pbf_set_collider_body_contact)");
  *n = ctx->contact.points;
  if (!points) return PBF_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(points, ctx->contactPoints.p, size_t(ctx->contact.points) * 3 * (ctx->fp64 ? 8 : 4), hipMemcpyDeviceToHost,
                             ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PBF_OK;
}

int pbf_collider_body_contact_state(pbf_ctx *ctx, struct pbf_body_contact_state *out) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!out) return fail(ctx, PBF_ERR_INVALID, "pbf_collider_body_contact_state: out == NULL");
  if (!ctx->contact.on) return fail(ctx, PBF_ERR_STATE, "pbf_collider_body_contact_state: contact is off (pbf_set_collider_body_contact)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  uint32_t seq;
  HIPCHK(ctx, ctx->hostContact.arm(seq));
  hipLaunchKernelGGL(k_contact_read, dim3(1), dim3(1), 0, ctx->stream, ctx->contactRec.as<const bodycontact::Record>(), ctx->hostContact.rec.p, seq);
  LAUNCH_CHECK(ctx);
  return receive(ctx, ctx->hostContact, "body contact read-back", *out);
}

static_assert(sizeof(pbf_collider_friction) == 7 * 8, "the friction record is seven doubles: mu, V, W");
// (k_collider_friction reads V.xyz, W.xyz as six consecutive doubles from either record)
static_assert(offsetof(pbf_collider_friction, angular_velocity) == offsetof(pbf_collider_friction, velocity) + 24 &&
                  offsetof(struct pbf_collider_body_state, angular_velocity) == offsetof(struct pbf_collider_body_state, velocity) + 24,
              "angular_velocity follows velocity directly in pbf_collider_friction and in pbf_collider_body_state");
int pbf_set_collider_friction(pbf_ctx *ctx, const pbf_collider_friction *f) {
  if (!ctx) return PBF_ERR_INVALID;
  if (f) {
    const char *why = nullptr;
    if (colliderfriction::check(f, &why) != PBF_OK) return fail(ctx, PBF_ERR_INVALID, why);
  }
  if (int rc = collider_needed(ctx, "pbf_set_collider_friction")) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (!f)  // off: the launch sequence without the pass; the reaction stays on
    return ctx->col.friction_cleared() ? collider_drop_graphs(ctx) : PBF_OK;
  const bool turnOn = !ctx->col.friction;
  if (turnOn) {  // everything a step will need is allocated here
    if (int rc = pbf_set_collider_reaction(ctx, 1)) return rc;  // (a no-op when it is on already)
    if (int rc = ensure(ctx, ctx->frictionRec, sizeof(pbf_collider_friction))) return rc;
    if (int rc = ensure(ctx, ctx->frictionCtl, sizeof(colliderfriction::Ctl))) return rc;
    if (int rc = ensure_friction_partials(ctx)) return rc;
    HIPCHK(ctx, ctx->hostFriction.rec.ensure(1));  // (so that the observer allocates nothing either)
  }
  hipLaunchKernelGGL(k_friction_store, dim3(1), dim3(1), 0, ctx->stream, *f, ctx->frictionRec.as<pbf_collider_friction>(),
                     ctx->frictionCtl.as<colliderfriction::Ctl>(), turnOn ? 1 : 0);
  LAUNCH_CHECK(ctx);
  return ctx->col.friction_set() ? collider_drop_graphs(ctx) : PBF_OK;  // (a rewritten record changes no key and drops no graph)
}

int pbf_collider_friction_reaction(pbf_ctx *ctx, pbf_collider_wrench *out) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!out) return fail(ctx, PBF_ERR_INVALID, "pbf_collider_friction_reaction: out == NULL");
  if (int rc = collider_refuse_slab(ctx)) return rc;
  if (!ctx->col.friction) return fail(ctx, PBF_ERR_STATE, "pbf_collider_friction_reaction: friction is off (pbf_set_collider_friction)");
  if (!ctx->col.friction_sums_ready()) return fail(ctx, PBF_ERR_STATE, "pbf_collider_friction_reaction: no step since friction was turned on");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  uint32_t seq;
  HIPCHK(ctx, ctx->hostFriction.arm(seq));
  hipLaunchKernelGGL(k_friction_final, dim3(1), dim3(BLOCK), 0, ctx->stream, ctx->frictionPartials.as<const WrenchPartial>(),
                     ctx->frictionCtl.as<const colliderfriction::Ctl>(), ctx->hostFriction.rec.p, seq);
  LAUNCH_CHECK(ctx);
  return receive(ctx, ctx->hostFriction, "collider friction read-back", *out);
}

int pbf_mesh_records(const pbf_mesh *mesh, int fp64, void *records, pbf_mesh_info *info) {
  const char *why = nullptr;
  const int rc = meshsdf::build_records(mesh, fp64, records, info, &why);
  if (rc != PBF_OK) g_create_error = why;  // (no ctx: read with pbf_last_error(NULL))
  return rc;
}

int pbf_mesh_soup_records(const pbf_mesh *mesh, int fp64, void *records, pbf_mesh_info *info) {
  const char *why = nullptr;
  const int rc = meshsdf::build_soup_records(mesh, fp64, records, info, &why);
  if (rc != PBF_OK) g_create_error = why;  // (no ctx: read with pbf_last_error(NULL))
  return rc;
}

int pbf_mesh_winding(pbf_ctx *ctx, const pbf_mesh *mesh, const pbf_collider_sdf *lattice, void *w) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!w) return fail(ctx, PBF_ERR_INVALID, "pbf_mesh_winding: w == NULL");
  if (!lattice) return fail(ctx, PBF_ERR_INVALID, "pbf_mesh_winding: lattice == NULL");
  size_t nodes = 0;
  if (int rc = collider_lattice_check(ctx, "pbf_mesh_winding", lattice, false, false, &nodes)) return rc;
  {  // the mesh, before anything is allocated
    const char *why = nullptr;
    if (meshsdf::build_soup_records(mesh, 0, nullptr, nullptr, &why) != PBF_OK) return fail(ctx, PBF_ERR_INVALID, why);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return ctx->fp64 ? mesh_winding_impl<double>(ctx, mesh, lattice, nodes, w) : mesh_winding_impl<float>(ctx, mesh, lattice, nodes, w);
}

int pbf_sdf_from_mesh(pbf_ctx *ctx, const pbf_mesh *mesh, const pbf_collider_sdf *lattice, uint32_t flags, void *phi,
                      pbf_mesh_sdf_stats *stats) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!phi) return fail(ctx, PBF_ERR_INVALID, "pbf_sdf_from_mesh: phi == NULL");
  DevBuf fresh;
  size_t nodes = 0;
  pbf_mesh_sdf_stats st{};
  if (int rc = mesh_sdf_run(ctx, "pbf_sdf_from_mesh", mesh, lattice, flags, false, fresh, &nodes, &st)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(phi, fresh.p, nodes * (ctx->fp64 ? sizeof(double) : sizeof(float)), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) *stats = st;
  return PBF_OK;
}

int pbf_set_collider_mesh(pbf_ctx *ctx, const pbf_mesh *mesh, const pbf_collider_sdf *lattice, uint32_t flags,
                          pbf_mesh_sdf_stats *stats) {
  return set_solid_mesh(ctx, "pbf_set_collider_mesh", ColliderState::COLLIDER, mesh, lattice, flags, stats);
}

// pbf_collider_sample / pbf_scenery_sample: one check, one launch; the scenery is the static function (pose == NULL)
static int sample_entry(pbf_ctx *ctx, const char *who, bool scenery, const pbf_params *p, size_t n, const double *points, void *phi,
                        void *moved, uint8_t *hit) {
  if (!ctx) return PBF_ERR_INVALID;
  const std::string w = std::string(who) + ": ";
  if (!p) return fail(ctx, PBF_ERR_INVALID, w + "params == NULL");
  if (!(p->scale > 0) || !(p->dt > 0)) return fail(ctx, PBF_ERR_INVALID, "dt and scale must be > 0");
  if (n >= (size_t(1) << 31)) return fail(ctx, PBF_ERR_INVALID, w + "2^31 points or more");
  if (n == 0) return PBF_OK;
  if (!points) return fail(ctx, PBF_ERR_INVALID, w + "points == NULL");
  if (scenery && !scenery_on(ctx)) return fail(ctx, PBF_ERR_STATE, w + "no scenery set (pbf_set_scenery)");
  if (!scenery && !collider_on(ctx)) return fail(ctx, PBF_ERR_STATE, w + "no collider set (pbf_set_collider)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const bool posed = !scenery && ctx->col.posed;
  const SolidLattice<DevBuf> &l = ctx->solid[scenery ? ColliderState::SCENERY : ColliderState::COLLIDER];
  if (ctx->fp64)
    return collider_sample_impl<double>(ctx, sdf_args<double>(l),
                                        posed ? ctx->colliderPose.as<const ColliderPose<double>>() : nullptr, p, n, points,
                                        static_cast<double *>(phi), static_cast<double *>(moved), hit);
  return collider_sample_impl<float>(ctx, sdf_args<float>(l),
                                     posed ? ctx->colliderPose.as<const ColliderPose<float>>() : nullptr, p, n, points,
                                     static_cast<float *>(phi), static_cast<float *>(moved), hit);
}
int pbf_collider_sample(pbf_ctx *ctx, const pbf_params *p, size_t n, const double *points, void *phi, void *moved, uint8_t *hit) {
  return sample_entry(ctx, "pbf_collider_sample", false, p, n, points, phi, moved, hit);
}

// ---- the scenery: one static lattice in the world frame beside the collider (the contract: include/pbf_hip.h) ----
int pbf_set_scenery(pbf_ctx *ctx, const pbf_collider_sdf *sdf) { return set_solid(ctx, "pbf_set_scenery", ColliderState::SCENERY, sdf); }

int pbf_set_scenery_mesh(pbf_ctx *ctx, const pbf_mesh *mesh, const pbf_collider_sdf *lattice, uint32_t flags, pbf_mesh_sdf_stats *stats) {
  return set_solid_mesh(ctx, "pbf_set_scenery_mesh", ColliderState::SCENERY, mesh, lattice, flags, stats);
}

int pbf_scenery_sample(pbf_ctx *ctx, const pbf_params *p, size_t n, const double *points, void *phi, void *moved, uint8_t *hit) {
  return sample_entry(ctx, "pbf_scenery_sample", true, p, n, points, phi, moved, hit);
}

}  // extern "C"

extern "C" {

int pbf_set_sources(pbf_ctx *ctx, size_t n, const pbf_source *sources) {
  if (!ctx) return PBF_ERR_INVALID;
  if (n && !sources) return fail(ctx, PBF_ERR_INVALID, "pbf_set_sources: n > 0 but sources == NULL");
  for (size_t k = 0; k < n; ++k) {
    bool ok = std::isfinite(sources[k].rate) && sources[k].rate >= 0;
    for (int a = 0; a < 3; ++a) ok = ok && std::isfinite(sources[k].centre[a]) && std::isfinite(sources[k].velocity[a]);
    for (int a = 0; a < 4; ++a) ok = ok && std::isfinite(sources[k].colour[a]);
    if (!ok) return fail(ctx, PBF_ERR_INVALID, "pbf_set_sources: rate must be finite and >= 0, centre / velocity / colour finite");
  }
  if (n && ctx->comm) return fail(ctx, PBF_ERR_STATE, kSceneSlabError);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<pbf_source> next(sources, sources + n);
  uint32_t total = 0;
  if (int rc = ctx->fp64 ? upload_sources<double>(ctx, next, total) : upload_sources<float>(ctx, next, total)) return rc;
  ctx->sources.swap(next), ctx->emitTotal = total;
  return PBF_OK;
}
int pbf_set_drains(pbf_ctx *ctx, size_t n, const pbf_drain *drains) {
  if (!ctx) return PBF_ERR_INVALID;
  if (n && !drains) return fail(ctx, PBF_ERR_INVALID, "pbf_set_drains: n > 0 but drains == NULL");
  for (size_t k = 0; k < n; ++k) {
    bool ok = std::isfinite(drains[k].width) && drains[k].width >= 0;
    for (int a = 0; a < 3; ++a) ok = ok && std::isfinite(drains[k].centre[a]);
    if (!ok) return fail(ctx, PBF_ERR_INVALID, "pbf_set_drains: width must be finite and >= 0, centre finite");
  }
  if (n && ctx->comm) return fail(ctx, PBF_ERR_STATE, kSceneSlabError);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<pbf_drain> next(drains, drains + n);
  if (int rc = ctx->fp64 ? upload_drains<double>(ctx, next) : upload_drains<float>(ctx, next)) return rc;
  ctx->drains.swap(next);
  return PBF_OK;
}
uint64_t pbf_scene_host_syncs(const pbf_ctx *ctx) { return ctx ? ctx->sceneHostSyncs : 0; }

int pbf_query_cells(pbf_ctx *ctx, const pbf_params *p, size_t n_points, const double *points, uint32_t *counts, uint64_t *ids,
                    size_t cap_per_point) {
  if (int rc = check(ctx, p, false)) return rc;
  const Refuse refuse{ctx, "pbf_query_cells"};
  if (int rc = refuse.slab_mode()) return rc;
  if (int rc = refuse.no_step()) return rc;
  if (n_points == 0) return PBF_OK;
  if (!points || !counts || (cap_per_point && !ids)) return fail(ctx, PBF_ERR_INVALID, "pbf_query_cells: NULL argument");
  if (n_points >= (size_t(1) << 31) || cap_per_point >= (size_t(1) << 31))
    return fail(ctx, PBF_ERR_INVALID, "pbf_query_cells: too many points / ids per point");
  for (size_t k = 0; k < 3 * n_points; ++k)
    if (!std::isfinite(points[k])) return fail(ctx, PBF_ERR_INVALID, "pbf_query_cells: points must be finite");
  return DISPATCH(ctx, query_impl, ctx, p, n_points, points, counts, ids, cap_per_point);
}

int pbf_diagnostics(pbf_ctx *ctx, const pbf_params *p, uint32_t what, pbf_diag *out) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!out) return fail(ctx, PBF_ERR_INVALID, "pbf_diagnostics: out == NULL");
  if (what & ~uint32_t(PBF_DIAG_DENSITY)) return fail(ctx, PBF_ERR_INVALID, "pbf_diagnostics: unknown bits in `what`");
  const bool density = (what & PBF_DIAG_DENSITY) != 0;
  if (density && !p) return fail(ctx, PBF_ERR_INVALID, "pbf_diagnostics: PBF_DIAG_DENSITY needs params");
  const Refuse refuse{ctx, "pbf_diagnostics"};
  if (density)
    if (int rc = refuse.params(p)) return rc;
  // global sums would need an all-reduce, and the copies of the neighbours' boundary columns would have to be left out
  if (int rc = refuse.slab_mode()) return rc;
  if (density)
    if (int rc = refuse.no_step(": the density part")) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return DISPATCH(ctx, diagnostics_impl, ctx, p, density, out);
}

int pbf_sample_points(pbf_ctx *ctx, const pbf_params *p, size_t n, const double *points, uint32_t what, const pbf_sample_out *out) {
  if (!ctx) return PBF_ERR_INVALID;
  if (what & ~uint32_t(PBF_SAMPLE_VELOCITY | PBF_SAMPLE_COLOUR)) return fail(ctx, PBF_ERR_INVALID, "pbf_sample_points: unknown bits in `what`");
  if (n >= (size_t(1) << 31)) return fail(ctx, PBF_ERR_INVALID, "pbf_sample_points: 2^31 points or more");
  if (n == 0) return PBF_OK;
  if (!points) return fail(ctx, PBF_ERR_INVALID, "pbf_sample_points: NULL argument");
  for (size_t k = 0; k < 3 * n; ++k)
    if (!std::isfinite(points[k])) return fail(ctx, PBF_ERR_INVALID, "pbf_sample_points: points must be finite");
  if (int rc = sample_check(ctx, p, what, out, "pbf_sample_points")) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return DISPATCH(ctx, sample_impl, ctx, p, n, points, nullptr, what, out, "pbf_sample_points");
}

int pbf_sample_lattice(pbf_ctx *ctx, const pbf_params *p, const double origin[3], const double spacing[3], const uint64_t dims[3],
                       uint32_t what, const pbf_sample_out *out) {
  if (!ctx) return PBF_ERR_INVALID;
  if (what & ~uint32_t(PBF_SAMPLE_VELOCITY | PBF_SAMPLE_COLOUR)) return fail(ctx, PBF_ERR_INVALID, "pbf_sample_lattice: unknown bits in `what`");
  if (!origin || !spacing || !dims) return fail(ctx, PBF_ERR_INVALID, "pbf_sample_lattice: NULL argument");
  SampleLatticeDesc lat;
  uint64_t n = 1;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(origin[a]) || !std::isfinite(spacing[a]))
      return fail(ctx, PBF_ERR_INVALID, "pbf_sample_lattice: origin and spacing must be finite");
    if (dims[a] == 0) return fail(ctx, PBF_ERR_INVALID, "pbf_sample_lattice: a zero in dims");
    if (dims[a] >= (uint64_t(1) << 31) || (n *= dims[a]) >= (uint64_t(1) << 31))
      return fail(ctx, PBF_ERR_INVALID, "pbf_sample_lattice: 2^31 points or more");
    lat.origin[a] = origin[a], lat.spacing[a] = spacing[a], lat.dims[a] = dims[a];
  }
  if (int rc = sample_check(ctx, p, what, out, "pbf_sample_lattice")) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return DISPATCH(ctx, sample_impl, ctx, p, size_t(n), nullptr, &lat, what, out, "pbf_sample_lattice");
}

int pbf_anisotropy_compute(pbf_ctx *ctx, const pbf_params *p, const pbf_anisotropy *g, const pbf_anisotropy_out *out) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!p || !g || !out) return fail(ctx, PBF_ERR_INVALID, "pbf_anisotropy_compute: NULL argument");
  const Refuse refuse{ctx, "pbf_anisotropy_compute"};
  if (int rc = refuse.params(p)) return rc;
  if (const char *why = anisotropy_config_error(g)) return fail(ctx, PBF_ERR_INVALID, std::string("pbf_anisotropy_compute: ") + why);
  // a particle near a cut needs both ranks' candidates, and the copies of the neighbours' columns would have to be left out
  if (int rc = refuse.slab_mode()) return rc;
  if (ctx->n == 0) return PBF_OK;
  if (int rc = refuse.no_step()) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return DISPATCH(ctx, anisotropy_impl, ctx, p, g, out);
}

int pbf_whitewater_configure(pbf_ctx *ctx, const pbf_whitewater *config) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!config) return fail(ctx, PBF_ERR_INVALID, "pbf_whitewater_configure: config == NULL");
  if (const char *why = whitewater_config_error(config)) return fail(ctx, PBF_ERR_INVALID, std::string("pbf_whitewater_configure: ") + why);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (!ctx->wwOn || config->capacity != ctx->ww.capacity) {  // (an unchanged capacity keeps the pool and what is in it)
    ctx->wwOn = false, ctx->ww.capacity = 0;
    if (int rc = ww_resize_pool(ctx, size_t(config->capacity))) return rc;
  }
  ctx->ww = *config, ctx->wwFrame = 0;
  ctx->wwOn = config->capacity != 0;
  if (!ctx->wwOn) {
    ctx->wwPotAt = 0;
    return PBF_OK;
  }
  if (int rc = ww_solids_buffers(ctx)) return rc;  // (pbf_set_whitewater_solids: its partials follow the capacity)
  return ensure_whitewater_fields(ctx);
}

// pbf_set_whitewater_solids: a wish — no lattice is needed, no ColliderState mode is touched and no captured graph dropped
int pbf_set_whitewater_solids(pbf_ctx *ctx, const pbf_whitewater_solids *cfg) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!cfg) {
    ctx->wwSolidsOn = false, ctx->wwSolidsSteps = 0;
    return PBF_OK;
  }
  const char *why = nullptr;
  if (wwsolids::check(cfg, &why) != PBF_OK) return fail(ctx, PBF_ERR_INVALID, why);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const bool was = ctx->wwSolidsOn;
  ctx->wwSolidsOn = true;
  if (int rc = ww_solids_buffers(ctx)) {
    ctx->wwSolidsOn = was;
    return rc;
  }
  ctx->wwSolids = *cfg;
  if (!was) ctx->wwSolidsSteps = 0;
  return PBF_OK;
}

int pbf_whitewater_solids_stats(pbf_ctx *ctx, struct pbf_whitewater_solids_stats *out) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!out) return fail(ctx, PBF_ERR_INVALID, "pbf_whitewater_solids_stats: out == NULL");
  if (!ctx->wwSolidsOn) return fail(ctx, PBF_ERR_STATE, "pbf_whitewater_solids_stats: the setting is off (pbf_set_whitewater_solids)");
  if (!ctx->wwSolidsSteps) return fail(ctx, PBF_ERR_STATE, "pbf_whitewater_solids_stats: no whitewater step since the setting was turned on");
  if (!ctx->wwSolidsFolded) {  // the last step found no lattice and launched nothing: there is nothing to copy
    out->hit_collider = out->hit_scenery = out->absorbed = out->born_inside = 0;
    out->step = ctx->wwSolidsSteps;
    return PBF_OK;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(out, ctx->wwSolidsRec.p, sizeof(*out), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PBF_OK;
}

int pbf_whitewater_upload(pbf_ctx *ctx, size_t n, const void *pos, const void *vel, const void *life) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!ctx->wwOn) return fail(ctx, PBF_ERR_STATE, "pbf_whitewater_upload: no pool (pbf_whitewater_configure)");
  if (n > ctx->ww.capacity) return fail(ctx, PBF_ERR_INVALID, "pbf_whitewater_upload: n exceeds the pool's capacity");
  if (n && !pos) return fail(ctx, PBF_ERR_INVALID, "pbf_whitewater_upload: n > 0 but pos == NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->fp64) return whitewater_upload_impl<double>(ctx, n, (const double *)pos, (const double *)vel, (const double *)life);
  return whitewater_upload_impl<float>(ctx, n, (const float *)pos, (const float *)vel, (const float *)life);
}

int pbf_whitewater_step(pbf_ctx *ctx, const pbf_params *p, pbf_whitewater_stats *out) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!p) return fail(ctx, PBF_ERR_INVALID, "pbf_whitewater_step: params == NULL");
  const Refuse refuse{ctx, "pbf_whitewater_step"};
  if (int rc = refuse.params(p)) return rc;
  // a diffuse particle near a cut needs both ranks' candidates, and the pool would have to migrate with the fluid
  if (int rc = refuse.slab_mode()) return rc;
  if (!ctx->wwOn) return fail(ctx, PBF_ERR_STATE, "pbf_whitewater_step: not configured (pbf_whitewater_configure)");
  if (int rc = refuse.no_step()) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return DISPATCH(ctx, whitewater_step_impl, ctx, p, out);
}

size_t pbf_whitewater_count(const pbf_ctx *ctx) { return ctx && ctx->wwOn ? ctx->wwCount : 0; }

int pbf_whitewater_download(pbf_ctx *ctx, void *pos, void *vel, void *life, uint8_t *kind, uint64_t *parent_id) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!ctx->wwOn) return PBF_OK;  // (no pool: nothing to copy)
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->fp64) return whitewater_download_impl<double>(ctx, (double *)pos, (double *)vel, (double *)life, kind, parent_id);
  return whitewater_download_impl<float>(ctx, (float *)pos, (float *)vel, (float *)life, kind, parent_id);
}

int pbf_read_buffer(pbf_ctx *ctx, int which, void *host, size_t bytes) {
  if (!ctx || !host) return PBF_ERR_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (which != PBF_BUF_NBR_COUNT)  // (the list lengths are indexed like the arrays the last build saw)
    if (int rc = drop_ghosts(ctx)) return rc;
  const void *src = nullptr;
  size_t avail = 0;
  const size_t v = ctx->fp64 ? sizeof(double4) : sizeof(float4);
  switch (which) {
    case PBF_BUF_KEYS: src = ctx->key[ctx->st.cur].p, avail = ctx->n * 4; break;
    case PBF_BUF_TABLE:
      if (!ctx->st.sorted) return fail(ctx, PBF_ERR_STATE, "table not built yet");
      src = ctx->table.p, avail = size_t(ctx->tableN) * 4;
      break;
    case PBF_BUF_PSTAR:
      if (int rc = ctx->fp64 ? materialise_pstar<double>(ctx) : materialise_pstar<float>(ctx)) return rc;
      src = ctx->pstar[ctx->st.pcur].p, avail = ctx->n * v;
      break;
    case PBF_BUF_NBR_COUNT: src = ctx->nbrCount.p, avail = (ctx->ghostsPending ? ctx->nOwned : ctx->n) * 4; break;
    case PBF_BUF_OMEGA:
      if (!ctx->st.omegaValid) return fail(ctx, PBF_ERR_STATE, "no vorticity pass since the arrays last changed (pbf_params.vorticity)");
      src = ctx->pstar[2].p, avail = ctx->n * v;
      break;
    case PBF_BUF_SURFACE:
      if (!ctx->st.surfaceValid) return fail(ctx, PBF_ERR_STATE, "no surface-tension pass since the arrays last changed (pbf_set_surface_tension)");
      src = ctx->surfB.p, avail = std::min(ctx->n * v, ctx->surfB.cap);
      break;
    case PBF_BUF_WHITEWATER:
      if (!record_current(ctx, ctx->wwPotAt))
        return fail(ctx, PBF_ERR_STATE, "no whitewater step since the arrays last changed (pbf_whitewater_step)");
      src = ctx->wwPot.p, avail = std::min(ctx->n * v, ctx->wwPot.cap);
      break;
    case PBF_BUF_COLLIDER_PUSH:
      if (!ctx->col.reaction || !push_current(ctx))
        return fail(ctx, PBF_ERR_STATE, "no sort since the collider reaction was enabled or the arrays last changed (pbf_set_collider_reaction)");
      if (ctx->col.records_by_row()) {  // the records are in row order: into the Morton order, as PBF_BUF_PSTAR's are
        if (int rc = ensure(ctx, ctx->pushOut, std::max<size_t>(ctx->cap, 1) * 2 * v)) return rc;
        if (ctx->fp64)
          hipLaunchKernelGGL((k_push_to_morton<double>), grid_for(std::max<size_t>(ctx->n, 1)), dim3(BLOCK), 0, ctx->stream, uint32_t(ctx->n),
                             ctx->pushRec.as<const vec4<double>>(), ctx->rowSlotOf.as<const uint32_t>(), ctx->pushOut.as<vec4<double>>());
        else
          hipLaunchKernelGGL((k_push_to_morton<float>), grid_for(std::max<size_t>(ctx->n, 1)), dim3(BLOCK), 0, ctx->stream, uint32_t(ctx->n),
                             ctx->pushRec.as<const vec4<float>>(), ctx->rowSlotOf.as<const uint32_t>(), ctx->pushOut.as<vec4<float>>());
        LAUNCH_CHECK(ctx);
        src = ctx->pushOut.p;
      } else {
        src = ctx->pushRec.p;
      }
      avail = ctx->n * 2 * v;
      break;
    case PBF_BUF_DENSITY:
      if (!record_current(ctx, ctx->diagRhoAt))
        return fail(ctx, PBF_ERR_STATE, "no density pass since the arrays last changed (pbf_diagnostics with PBF_DIAG_DENSITY)");
      src = ctx->diagRho.p, avail = std::min(ctx->n * (v / 4), ctx->diagRho.cap);
      break;
    default: return fail(ctx, PBF_ERR_INVALID, "unknown buffer");
  }
  if (bytes > avail) return fail(ctx, PBF_ERR_INVALID, "read beyond buffer");
  if (!src) return fail(ctx, PBF_ERR_STATE, "buffer not allocated yet");
  HIPCHK(ctx, hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PBF_OK;
}

// fp64 sweeps: 2^20 threads x 10240 rounds = 1.07e10 pseudo-random operands per category
constexpr uint32_t kSelftestRounds64 = 10240, kSelftestBlocks64 = 4096;
// the four categories of k_selftest_math / k_selftest_math64 into totals[0 .. 3], their visited counts into totals[4 .. 7]
static int launch_selftest_math(pbf_ctx *ctx, unsigned long long *totals) {
  if (ctx->fp64) {  // 1.07e10 pseudo-random operands per category and run (exhaustive is impossible in fp64): 2^20 threads x 10240
    const double h = ctx->desc.h;
    const double p6 = poly6_factor<double>(h), r = double(CorrDeltaQ * h), d = (h * h) - r * r;
    hipLaunchKernelGGL(k_selftest_math64, dim3(kSelftestBlocks64), dim3(BLOCK), 0, ctx->stream, totals, p6 * (d * d * d),
                       double(RHO), h, kSelftestRounds64);
    LAUNCH_CHECK(ctx);
    return PBF_OK;
  }
  // the two per-launch constant divisors of delta-p for this context's h: poly6(0.3 h) and the reference density
  const float h = float(ctx->desc.h);
  const float p6 = poly6_factor<float>(h), r = float(CorrDeltaQ * h), d = (h * h) - r * r;
  const float p6DeltaQ = p6 * (d * d * d);
  hipLaunchKernelGGL(k_selftest_math, dim3(uint32_t(ctx->numCUs) * 8), dim3(BLOCK), 0, ctx->stream, totals, p6DeltaQ,
                     float(RHO), h);
  LAUNCH_CHECK(ctx);
  return PBF_OK;
}

int pbf_selftest_math(pbf_ctx *ctx, uint64_t mismatches[4]) {
  if (!ctx || !mismatches) return PBF_ERR_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = ensure(ctx, ctx->selTotals, 128)) return rc;
  HIPCHK(ctx, hipMemsetAsync(ctx->selTotals.p, 0, 64, ctx->stream));
  if (int rc = launch_selftest_math(ctx, ctx->selTotals.as<unsigned long long>())) return rc;
  unsigned long long hst[4] = {0, 0, 0, 0};
  HIPCHK(ctx, hipMemcpyAsync(hst, ctx->selTotals.p, 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 4; ++k) mismatches[k] = hst[k];
  return PBF_OK;
}

int pbf_selftest_divides(pbf_ctx *ctx, uint32_t numerators, uint64_t mismatches[8], uint64_t visited[8]) {
  if (!ctx || !mismatches || !visited) return PBF_ERR_INVALID;
  if (numerators > 64u) return fail(ctx, PBF_ERR_INVALID, "pbf_selftest_divides: at most 64 numerators per divisor");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = ensure(ctx, ctx->selTotals, 128)) return rc;
  HIPCHK(ctx, hipMemsetAsync(ctx->selTotals.p, 0, 128, ctx->stream));
  unsigned long long *totals = ctx->selTotals.as<unsigned long long>();
  if (int rc = launch_selftest_math(ctx, totals)) return rc;
  if (ctx->fp64) hipLaunchKernelGGL(k_selftest_divides64, dim3(kSelftestBlocks64), dim3(BLOCK), 0, ctx->stream, totals + 8,
                                    kSelftestRounds64);
  else hipLaunchKernelGGL(k_selftest_divides, dim3(uint32_t(ctx->numCUs) * 8), dim3(BLOCK), 0, ctx->stream, totals + 8,
                          numerators);
  LAUNCH_CHECK(ctx);
  unsigned long long hst[16] = {};
  HIPCHK(ctx, hipMemcpyAsync(hst, ctx->selTotals.p, 128, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 4; ++k) {
    mismatches[k] = hst[k], visited[k] = hst[4 + k];
    mismatches[4 + k] = hst[8 + k], visited[4 + k] = hst[12 + k];
  }
  return PBF_OK;
}

size_t pbf_table_size(const pbf_ctx *ctx) { return ctx ? ctx->tableN : 0; }
int pbf_grid_extent(const pbf_ctx *ctx, uint64_t extent[3], double min_extent[3]) {
  if (!ctx) return PBF_ERR_INVALID;
  for (int i = 0; i < 3; ++i) {
    if (extent) extent[i] = ctx->extent[i];
    if (min_extent) min_extent[i] = ctx->minExtent[i];
  }
  return PBF_OK;
}

int pbf_stage_times(pbf_ctx *ctx, const char **names, double *mean_ms, uint64_t *calls, int cap) {
  if (!ctx) return PBF_ERR_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = resolve_events(ctx)) return rc;
  int k = 0;
  for (; k < ST_COUNT && k < cap; ++k) {
    if (names) names[k] = kStageNames[k];
    if (mean_ms) mean_ms[k] = ctx->stageCalls[k] ? ctx->stageMs[k] / double(ctx->stageCalls[k]) : 0.0;
    if (calls) calls[k] = ctx->stageCalls[k];
  }
  return k;
}
int pbf_reset_stage_times(pbf_ctx *ctx) {
  if (!ctx) return PBF_ERR_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = resolve_events(ctx)) return rc;
  for (int k = 0; k < ST_COUNT; ++k) ctx->stageMs[k] = 0, ctx->stageCalls[k] = 0;
  return PBF_OK;
}

}  // extern "C"

// ================================================================================================
// Slab decomposition entry points (include/pbf_hip.h "multi-GPU").  The caller (one process per
// GPU) owns the wire buffers and moves them with RCCL (torch.distributed "nccl" send/recv over
// xGMI); this library only selects, packs, appends and unpacks on the device.
// ================================================================================================
namespace {

template <typename N, int MODE>
int run_select(pbf_ctx *ctx, const pbf_slab_cut *cut, void *sendL, void *sendR, uint32_t cap, uint32_t totals[3],
               bool readback = true) {
  const uint32_t n = uint32_t(ctx->n);
  const uint32_t nb = (n + SEL_TILE - 1) / SEL_TILE;
  if (int rc = ensure(ctx, ctx->selCounts, size_t(3) * std::max(nb, 1u) * 4)) return rc;
  if (int rc = ensure(ctx, ctx->selTotals, 16)) return rc;
  if (int rc = ensure(ctx, ctx->ghostSrcL, size_t(std::max(cap, 1u)) * 4)) return rc;
  if (int rc = ensure(ctx, ctx->ghostSrcR, size_t(std::max(cap, 1u)) * 4)) return rc;
  totals[0] = totals[1] = totals[2] = 0;
  if (n == 0) return PBF_OK;
  const uint32_t xo = ctx->slabConfigured ? ctx->xoff : 0u;  // the keys' x frame
  SlabCut s{cut->xlo - std::min(cut->xlo, xo), cut->xhi == 0xFFFFFFFFu ? cut->xhi : cut->xhi - std::min(cut->xhi, xo),
            cut->has_left ? 1u : 0u, cut->has_right ? 1u : 0u};
  const int a = ctx->st.cur, b = 1 - a;
  uint32_t *counts = ctx->selCounts.as<uint32_t>(), *tot = ctx->selTotals.as<uint32_t>();
  hipLaunchKernelGGL((k_sel_count<MODE>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n, s, ctx->key[a].as<const uint32_t>(),
                     ctx->type[a].as<const uint8_t>(), nb, counts);
  hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(BLOCK), 0, ctx->stream, nb, counts, tot);
  hipLaunchKernelGGL((k_sel_emit<N, MODE>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n, s, arrays<N>(ctx, a, ctx->st.pcur),
                     arrays<N>(ctx, b, b), nb, counts, sendL, sendR, cap, ctx->ghostSrcL.as<uint32_t>(),
                     ctx->ghostSrcR.as<uint32_t>());
  LAUNCH_CHECK(ctx);
  if (!readback) return PBF_OK;  // (pbf_slab_step reads selTotals back together with the received headers)
  HIPCHK(ctx, hipMemcpyAsync(totals, tot, 12, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the caller needs the counts to size its sends
  return PBF_OK;
}

template <typename N> int slab_migrate(pbf_ctx *ctx, const pbf_slab_cut *cut, void *sL, void *sR, uint32_t cap, uint32_t out[2]) {
  if (int rc = drop_histogram(ctx)) return rc;  // predict's histogram describes the pre-migration set
  uint32_t t[3];
  if (int rc = run_select<N, SEL_MIGRATE>(ctx, cut, sL, sR, cap, t)) return rc;
  if (t[1] > cap || t[2] > cap) return fail(ctx, PBF_ERR_INVALID, "migrant buffer too small");
  ctx->st.compacted(/*flipped=*/ctx->n != 0);  // the keeps were compacted into the other array set
  ctx->n = t[0];
  ctx->nOwned = t[0];
  out[0] = t[1], out[1] = t[2];
  return PBF_OK;
}

template <typename N> int slab_add_migrants(pbf_ctx *ctx, const void *rL, uint32_t nL, const void *rR, uint32_t nR) {
  if (ctx->n + nL + nR > ctx->cap) return fail(ctx, PBF_ERR_INVALID, "particle capacity exceeded: call pbf_reserve");
  if (nL + nR)
    hipLaunchKernelGGL((k_append_migrants<N>), grid_for(nL + nR), dim3(BLOCK), 0, ctx->stream, uint32_t(ctx->n),
                       static_cast<const MigrantRec<N> *>(rL), nL, static_cast<const MigrantRec<N> *>(rR), nR,
                       ctx->shiftL, ctx->shiftR, arrays<N>(ctx, ctx->st.cur, ctx->st.pcur));
  LAUNCH_CHECK(ctx);
  ctx->n += nL + nR;
  ctx->nOwned = uint32_t(ctx->n);
  return PBF_OK;
}

template <typename N> int slab_ghosts(pbf_ctx *ctx, const pbf_slab_cut *cut, void *sL, void *sR, uint32_t cap, uint32_t out[2]) {
  uint32_t t[3];
  if (int rc = run_select<N, SEL_GHOST>(ctx, cut, sL, sR, cap, t)) return rc;
  if (t[0] > cap || t[1] > cap) return fail(ctx, PBF_ERR_INVALID, "ghost buffer too small");
  ctx->sentL = t[0], ctx->sentR = t[1];
  out[0] = t[0], out[1] = t[1];
  return PBF_OK;
}

template <typename N> int slab_add_ghosts(pbf_ctx *ctx, const void *rL, uint32_t nL, const void *rR, uint32_t nR) {
  if (ctx->n + nL + nR > ctx->cap) return fail(ctx, PBF_ERR_INVALID, "particle capacity exceeded: call pbf_reserve");
  if (nL + nR)
    hipLaunchKernelGGL((k_append_ghosts<N>), grid_for(nL + nR), dim3(BLOCK), 0, ctx->stream, uint32_t(ctx->n),
                       static_cast<const GhostRec<N> *>(rL), nL, static_cast<const GhostRec<N> *>(rR), nR,
                       ctx->shiftL, ctx->shiftR, arrays<N>(ctx, ctx->st.cur, ctx->st.pcur));
  ctx->gotL = nL, ctx->gotR = nR;
  ctx->ghostAt = uint32_t(ctx->n);
  ctx->n += nL + nR;
  if (nL + nR) ctx->hasObstacles = true;  // "special" particles exist: the kernels must look at type[]
  // histogram of the re-assembled set (owned + copies) for the sort
  if (ctx->n)
    hipLaunchKernelGGL(k_count_keys, grid_for(ctx->n), dim3(BLOCK), 0, ctx->stream, uint32_t(ctx->n), ctx->tableN,
                       ctx->key[ctx->st.cur].as<const uint32_t>(), ctx->count.as<uint32_t>(), ctx->cellSlot.as<uint32_t>());
  LAUNCH_CHECK(ctx);
  ctx->st.histogram_current(ctx->tableN);
  ctx->slabActive = true;
  return PBF_OK;
}

template <typename N> int slab_pack(pbf_ctx *ctx, void *sL, void *sR, const void *field = nullptr) {
  const uint32_t m = ctx->sentL + ctx->sentR;
  // {pStar, lambda}: from wherever it currently lives — the row-major copy while the iterations run on it
  const bool rows = !field && ctx->st.pstar_in_live_rows();
  if (!field && ctx->st.pstarInRows && !rows) return fail(ctx, PBF_ERR_STATE, "slab pack: no current pStar");
  const vec4<N> *src = field ? static_cast<const vec4<N> *>(field)
                             : rows ? ctx->rowPstar[ctx->st.rcur].as<const vec4<N>>() : ctx->pstar[ctx->st.pcur].as<const vec4<N>>();
  if (m)
    hipLaunchKernelGGL((k_pack_field<N>), grid_for(m), dim3(BLOCK), 0, ctx->stream, ctx->sentL, ctx->sentR,
                       ctx->ghostSrcL.as<const uint32_t>(), ctx->ghostSrcR.as<const uint32_t>(),
                       ctx->slotOf.as<const uint32_t>(), src,
                       static_cast<vec4<N> *>(sL), static_cast<vec4<N> *>(sR), rows ? ctx->rowSlotOf.as<const uint32_t>() : nullptr);
  LAUNCH_CHECK(ctx);
  return PBF_OK;
}

template <typename N> int slab_unpack(pbf_ctx *ctx, const void *rL, const void *rR, void *field = nullptr) {
  const uint32_t m = ctx->gotL + ctx->gotR;
  StepConsts<N> c;
  if (!ctx->haveParams) return fail(ctx, PBF_ERR_STATE, "pbf_slab_unpack before any stage");
  if (int rc = make_consts<N>(ctx, &ctx->lastParams, c)) return rc;
  const bool rows = !field && ctx->st.pstar_in_live_rows();
  if (m)
    hipLaunchKernelGGL((k_unpack_field<N>), grid_for(m), dim3(BLOCK), 0, ctx->stream, c, ctx->ghostAt, ctx->gotL, ctx->gotR,
                       static_cast<const vec4<N> *>(rL), static_cast<const vec4<N> *>(rR),
                       ctx->slotOf.as<const uint32_t>(),
                       field ? static_cast<vec4<N> *>(field) : rows ? ctx->rowPstar[ctx->st.rcur].as<vec4<N>>() : ctx->pstar[ctx->st.pcur].as<vec4<N>>(),
                       field ? nullptr : rows ? ctx->rowQpos.as<uint2>() : ctx->qpos.as<uint2>(),
                       rows ? ctx->rowSlotOf.as<const uint32_t>() : nullptr);
  LAUNCH_CHECK(ctx);
  return PBF_OK;
}

template <typename N> int slab_finish(pbf_ctx *ctx, bool knownOwned = false) {
  // drop the copies: the MIGRATE select with no neighbours keeps exactly the non-ghost particles
  pbf_slab_cut none{0, 0xFFFFFFFFu, 0, 0};
  uint32_t t[3];
  // (pbf_slab_step knows the count — every non-copy is owned — and skips the synchronising read-back)
  if (int rc = run_select<N, SEL_MIGRATE>(ctx, &none, nullptr, nullptr, 0, t, !knownOwned)) return rc;
  if (knownOwned) t[0] = ctx->n ? ctx->nOwned : 0;
  ctx->st.compacted(/*flipped=*/ctx->n != 0);
  ctx->n = t[0];
  ctx->nOwned = t[0];
  ctx->hasObstacles = ctx->realObstacles;
  ctx->slabActive = false;
  ctx->sentL = ctx->sentR = ctx->gotL = ctx->gotR = 0;
  return PBF_OK;
}

int slab_check(pbf_ctx *ctx) {
  if (!ctx) return PBF_ERR_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return PBF_OK;
}

int drop_ghosts(pbf_ctx *ctx) {
  if (!ctx->ghostsPending) return PBF_OK;
  ctx->ghostsPending = false;
  return DISPATCH(ctx, slab_finish, ctx, /*knownOwned=*/true);
}

}  // namespace

extern "C" {

int pbf_reserve(pbf_ctx *ctx, size_t capacity) {
  if (!ctx) return PBF_ERR_INVALID;
  if (ctx->n && capacity > ctx->cap) return fail(ctx, PBF_ERR_STATE, "pbf_reserve must precede pbf_upload");
  ctx->reserve = capacity;
  return PBF_OK;
}
int pbf_slab_configure(pbf_ctx *ctx, const pbf_slab_cut *cut, uint32_t left_xlo, uint32_t right_xlo) {
  if (!ctx) return PBF_ERR_INVALID;
  if (!cut) {  // back to the global x frame
    ctx->slabConfigured = false, ctx->xoff = 0, ctx->shiftL = ctx->shiftR = 0;
    return PBF_OK;
  }
  if (cut->xhi <= cut->xlo) return fail(ctx, PBF_ERR_INVALID, "empty slab");
  // frame origin = PBF_SLAB_FRAME_MARGIN columns left of the first owned column (the left ghost column is the one
  // next to it); rank 0 keeps the padding columns.  The margin keeps local x coordinates non-negative — a negative one
  // would wrap in the 10-bit Morton field and send the particle to the wrong neighbour — for every particle this rank
  // can hold at predict time: owned ones that moved left (< 2 columns per step) and, after a re-cut, the owners of
  // columns just handed to the left neighbour (a cut moves by <= 2 columns).
  auto origin = [](uint32_t xlo, bool hasLeft) {
    return hasLeft && xlo > 0 ? xlo - std::min<uint32_t>(xlo, PBF_SLAB_FRAME_MARGIN) : 0u;
  };
  ctx->slabCut = *cut;
  ctx->xoff = origin(cut->xlo, cut->has_left != 0);
  // a neighbour's records arrive keyed in ITS frame: x_mine = x_theirs + their_origin - my_origin
  ctx->shiftL = int32_t(origin(left_xlo, left_xlo > 0)) - int32_t(ctx->xoff);
  ctx->shiftR = int32_t(origin(right_xlo, true)) - int32_t(ctx->xoff);
  ctx->slabConfigured = true;
  ctx->st.compacted(/*flipped=*/false);  // (the keys' frame changed)
  return PBF_OK;
}
size_t pbf_slab_record_bytes(const pbf_ctx *ctx, int kind) {
  if (!ctx) return 0;
  switch (kind) {
    case PBF_REC_MIGRANT: return ctx->fp64 ? sizeof(MigrantRec<double>) : sizeof(MigrantRec<float>);
    case PBF_REC_GHOST: return ctx->fp64 ? sizeof(GhostRec<double>) : sizeof(GhostRec<float>);
    case PBF_REC_FIELD: return ctx->fp64 ? sizeof(double4) : sizeof(float4);
    default: return 0;
  }
}
int pbf_slab_migrate(pbf_ctx *ctx, const pbf_slab_cut *cut, void *send_left, void *send_right, uint32_t cap_records,
                     uint32_t counts[2]) {
  if (int rc = slab_check(ctx)) return rc;
  if (!cut || !counts) return fail(ctx, PBF_ERR_INVALID, "NULL argument");
  return DISPATCH(ctx, slab_migrate, ctx, cut, send_left, send_right, cap_records, counts);
}
int pbf_slab_add_migrants(pbf_ctx *ctx, const void *recv_left, uint32_t n_left, const void *recv_right, uint32_t n_right) {
  if (int rc = slab_check(ctx)) return rc;
  return DISPATCH(ctx, slab_add_migrants, ctx, recv_left, n_left, recv_right, n_right);
}
int pbf_slab_ghosts(pbf_ctx *ctx, const pbf_slab_cut *cut, void *send_left, void *send_right, uint32_t cap_records,
                    uint32_t counts[2]) {
  if (int rc = slab_check(ctx)) return rc;
  if (!cut || !counts) return fail(ctx, PBF_ERR_INVALID, "NULL argument");
  return DISPATCH(ctx, slab_ghosts, ctx, cut, send_left, send_right, cap_records, counts);
}
int pbf_slab_add_ghosts(pbf_ctx *ctx, const void *recv_left, uint32_t n_left, const void *recv_right, uint32_t n_right) {
  if (int rc = slab_check(ctx)) return rc;
  return DISPATCH(ctx, slab_add_ghosts, ctx, recv_left, n_left, recv_right, n_right);
}
int pbf_slab_pack(pbf_ctx *ctx, void *send_left, void *send_right) {
  if (int rc = slab_check(ctx)) return rc;
  if (!ctx->st.sorted) return fail(ctx, PBF_ERR_STATE, "pbf_slab_pack needs pbf_stage_sort first");
  return DISPATCH(ctx, slab_pack, ctx, send_left, send_right);
}
int pbf_slab_unpack(pbf_ctx *ctx, const void *recv_left, const void *recv_right) {
  if (int rc = slab_check(ctx)) return rc;
  if (!ctx->st.sorted) return fail(ctx, PBF_ERR_STATE, "pbf_slab_unpack needs pbf_stage_sort first");
  return DISPATCH(ctx, slab_unpack, ctx, recv_left, recv_right);
}
int pbf_slab_finish(pbf_ctx *ctx) {
  if (int rc = slab_check(ctx)) return rc;
  ctx->ghostsPending = false;
  return DISPATCH(ctx, slab_finish, ctx);
}
size_t pbf_owned_count(const pbf_ctx *ctx) { return ctx ? (ctx->slabActive ? ctx->nOwned : ctx->n) : 0; }

int pbf_slab_column_histogram(pbf_ctx *ctx, uint32_t out[1024]) {
  if (int rc = slab_check(ctx)) return rc;
  if (!out) return fail(ctx, PBF_ERR_INVALID, "NULL argument");
  if (int rc = ensure(ctx, ctx->selTotals, 16)) return rc;
  if (int rc = ensure(ctx, ctx->colHist, 1024 * 4)) return rc;
  HIPCHK(ctx, hipMemsetAsync(ctx->colHist.p, 0, 1024 * 4, ctx->stream));
  if (ctx->n) {
    const uint32_t blocks = uint32_t(std::min<size_t>((ctx->n + BLOCK - 1) / BLOCK, size_t(ctx->numCUs) * 4));
    hipLaunchKernelGGL(k_column_histogram, dim3(blocks), dim3(BLOCK), 0, ctx->stream, uint32_t(ctx->n),
                       ctx->slabConfigured ? ctx->xoff : 0u, ctx->key[ctx->st.cur].as<const uint32_t>(),
                       ctx->type[ctx->st.cur].as<const uint8_t>(), ctx->colHist.as<uint32_t>());
    LAUNCH_CHECK(ctx);
  }
  HIPCHK(ctx, hipMemcpyAsync(out, ctx->colHist.p, 1024 * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PBF_OK;
}

}  // extern "C"

// ================================================================================================
// Communicator + the whole slab step inside the library (include/pbf_hip.h "communicator")
// ================================================================================================
namespace {

thread_local std::string g_comm_error;

pbf_slab_cut cut_of(const pbf_ctx *ctx) {
  const int r = ctx->comm->rank, n = ctx->comm->nranks;
  return pbf_slab_cut{ctx->cuts[r], ctx->cuts[r + 1], r > 0 ? 1 : 0, r + 1 < n ? 1 : 0};
}

int apply_cuts(pbf_ctx *ctx) {
  const int r = ctx->comm->rank, n = ctx->comm->nranks;
  if (n == 1) return pbf_slab_configure(ctx, nullptr, 0, 0);
  const pbf_slab_cut c = cut_of(ctx);
  return pbf_slab_configure(ctx, &c, r > 0 ? ctx->cuts[r - 1] : 0, r + 1 < n ? ctx->cuts[r + 1] : 0);
}

int exchange(pbf_ctx *ctx, size_t nSL, size_t nSR, size_t nRL, size_t nRR, size_t offset = 0) {
  const int rc = comm_exchange(ctx->comm, ctx->stream, ctx->wireSend[0].as<uint8_t>() + offset, nSL,
                               ctx->wireSend[1].as<uint8_t>() + offset, nSR, ctx->wireRecv[0].as<uint8_t>() + offset, nRL,
                               ctx->wireRecv[1].as<uint8_t>() + offset, nRR);
  if (rc) ctx->err = "slab exchange: " + ctx->comm->err;
  return rc;
}

// The opt-in extras in slab mode: the same three gather ops as extras_impl, with the owners refreshing their copies'
// velocity / vorticity before each op that reads them (the copies' velocities are not part of the ghost records).
template <typename N, bool FAST> int slab_extras_impl(pbf_ctx *ctx, const pbf_params *p) {
  StepConsts<N> c;
  if (int rc = make_consts<N>(ctx, p, c)) return rc;
  const uint8_t *type = ctx->type[ctx->st.cur].as<const uint8_t>();
  const vec4<N> *ps = ctx->pstar[ctx->st.cur].as<const vec4<N>>();
  const size_t fb = sizeof(vec4<N>);
  auto refresh = [&](void *field) -> int {
    if (int rc = slab_pack<N>(ctx, ctx->wireSend[0].p, ctx->wireSend[1].p, field)) return rc;
    if (int rc = exchange(ctx, ctx->sentL * fb, ctx->sentR * fb, ctx->gotL * fb, ctx->gotR * fb)) return rc;
    return slab_unpack<N>(ctx, ctx->wireRecv[0].p, ctx->wireRecv[1].p, field);
  };
  auto vel = [&](int k) { return ctx->vel4[k].as<vec4<N>>(); };
  int s = ctx->st.cur, o = 1 - s;
  if (int rc = refresh(vel(s))) return rc;
  if (p->vorticity) {
    vec4<N> *omega = ctx->pstar[2].as<vec4<N>>();
    typename VorticityOp<N, FAST>::Args a1{ps, vel(s), omega, type};
    if (int rc = launch_gather<N, VorticityOp<N, FAST>>(ctx, c, a1)) return rc;
    if (int rc = refresh(omega)) return rc;
    typename VorticityForceOp<N, FAST>::Args a2{ps, omega, vel(s), vel(o), type};
    if (int rc = launch_gather<N, VorticityForceOp<N, FAST>>(ctx, c, a2)) return rc;
    std::swap(ctx->vel4[s], ctx->vel4[o]);
    if (p->xsph)
      if (int rc = refresh(vel(s))) return rc;
  }
  if (p->xsph) {
    typename XsphOp<N, FAST>::Args a3{ps, vel(s), vel(o), type};
    if (int rc = launch_gather<N, XsphOp<N, FAST>>(ctx, c, a3)) return rc;
    std::swap(ctx->vel4[s], ctx->vel4[o]);
  }
  return PBF_OK;
}

// Spin on the pinned word k_slab_counts writes last (wait_for_word).
int wait_for_counts(pbf_ctx *ctx, uint32_t seq) { return wait_for_word(ctx, ctx->hostCounts.p + 7, seq, "slab read-back"); }

// One step of the slab protocol, everything on the solver's stream (round 3: ONE select pass, no compaction, no
// re-histogram, finalise + predict fused between the steps of one pbf_slab_steps call):
//   predict (classifies: stayers into the histogram, leavers and last step's copies not)
//   select: leavers -> migrant wire (their slots die), copies of the boundary stayers -> ghost wire       [3 small kernels]
//   [migrants]  exchange, read-back #1 (how many arrived), append + histogram, copies of boundary arrivals -> ghost wire
//   [copies]    exchange, read-back #2 (how many copies each way), append + histogram
//   sort (skips the dead slots: this is where the leavers and the old copies disappear) -> diffuse -> K x { lambda ->
//   [field] -> delta -> [field] } -> finalise (+ next predict)
template <typename N> int slab_step_impl(pbf_ctx *ctx, const pbf_params *p) {
  struct ModeGuard {
    pbf_ctx *c;
    ~ModeGuard() { c->slabStepMode = false; }
  } guard{ctx};
  ctx->slabStepMode = true;
  if (!ctx->st.take_prediction())  // (else the previous step of this pbf_slab_steps call has predicted already)
    if (int rc = stage_predict<N>(ctx, p)) return rc;
  StepConsts<N> c;
  if (int rc = make_consts<N>(ctx, p, c)) return rc;
  const uint32_t nPrev = uint32_t(ctx->n), oldCopies = ctx->ghostsPending ? ctx->gotL + ctx->gotR : 0u;
  const pbf_slab_cut cut = cut_of(ctx);
  const SlabCut sc{c.sxlo, c.sxhi, c.sHasL, c.sHasR};
  (void)cut;
  uint8_t *mL = ctx->wireSend[0].as<uint8_t>(), *mR = ctx->wireSend[1].as<uint8_t>();
  uint8_t *gL = ctx->wireGhost[0].as<uint8_t>(), *gR = ctx->wireGhost[1].as<uint8_t>();
  uint8_t *rL = ctx->wireRecv[0].as<uint8_t>(), *rR = ctx->wireRecv[1].as<uint8_t>();
  const int a = ctx->st.cur;
  const uint32_t nb = std::max(1u, (nPrev + SEL_TILE - 1) / SEL_TILE);
  if (int rc = ensure(ctx, ctx->selCounts, size_t(4) * nb * 4)) return rc;
  if (int rc = ensure(ctx, ctx->selTotals, 16)) return rc;
  if (int rc = ensure(ctx, ctx->ghostSrcL, size_t(ctx->wireCap) * 4)) return rc;
  if (int rc = ensure(ctx, ctx->ghostSrcR, size_t(ctx->wireCap) * 4)) return rc;
  uint32_t *counts = ctx->selCounts.as<uint32_t>(), *tot = ctx->selTotals.as<uint32_t>();
  volatile uint32_t *h = ctx->hostCounts.p;
  // ---- the select: one pass for both rounds --------------------------------------------------------------------
  hipLaunchKernelGGL(k_slab_count, dim3(nb), dim3(BLOCK), 0, ctx->stream, nPrev, sc, ctx->key[a].as<const uint32_t>(),
                     ctx->type[a].as<const uint8_t>(), nb, counts);
  hipLaunchKernelGGL(k_slab_scan, dim3(1), dim3(BLOCK), 0, ctx->stream, nb, counts, tot, reinterpret_cast<uint32_t *>(mL),
                     reinterpret_cast<uint32_t *>(mR), reinterpret_cast<uint32_t *>(gL), reinterpret_cast<uint32_t *>(gR),
                     reinterpret_cast<uint32_t *>(rL), reinterpret_cast<uint32_t *>(rR));
  hipLaunchKernelGGL((k_slab_emit<N>), dim3(nb), dim3(BLOCK), 0, ctx->stream, nPrev, sc, arrays<N>(ctx, a, ctx->st.pcur), nb, counts,
                     reinterpret_cast<MigrantRec<N> *>(mL + WIRE_HDR), reinterpret_cast<MigrantRec<N> *>(mR + WIRE_HDR),
                     reinterpret_cast<GhostRec<N> *>(gL + WIRE_HDR), reinterpret_cast<GhostRec<N> *>(gR + WIRE_HDR), ctx->wireCap,
                     ctx->ghostSrcL.as<uint32_t>(), ctx->ghostSrcR.as<uint32_t>());
  LAUNCH_CHECK(ctx);
  // an exchange round: fixed-size first message {header | first `chunk` records}; the rest, when a side holds more
  // (a re-cut hands whole columns over), in a second, exactly sized exchange once both ends know the counts
  auto round = [&](uint8_t *sL, uint8_t *sR, uint32_t chunk, size_t recBytes, int idxL, int idxR, uint32_t got[2]) -> int {
    const size_t first = WIRE_HDR + size_t(chunk) * recBytes;
    if (int rc = comm_exchange(ctx->comm, ctx->stream, sL, first, sR, first, rL, first, rR, first)) {
      ctx->err = "slab exchange: " + ctx->comm->err;
      return rc;
    }
    const uint32_t seq = ++ctx->slabSeq;
    hipLaunchKernelGGL(k_slab_counts, dim3(1), dim3(64), 0, ctx->stream, tot, reinterpret_cast<uint32_t *>(rL),
                       reinterpret_cast<uint32_t *>(rR), h, seq);
    LAUNCH_CHECK(ctx);
    // the one read-back of this round (the counts size the launches below): the host POLLS the pinned sequence word the
    // kernel writes last — a few microseconds after the kernel retires, where hipStreamSynchronize took 15-30
    if (int rc = wait_for_counts(ctx, seq)) return rc;
    ctx->slabHostSyncs++;
    got[0] = h[4], got[1] = h[5];
    const uint32_t ownL = h[idxL], ownR = h[idxR];
    const uint32_t most = std::max(std::max(ownL, ownR), std::max(got[0], got[1]));
    if (most > ctx->wireCap)
      return fail(ctx, PBF_ERR_COMM, "slab wire buffers too small (" + std::to_string(most) + " records > " +
                                         std::to_string(ctx->wireCap) + "): pbf_reserve a larger particle capacity before attaching");
    auto rest = [&](uint32_t count) { return count > chunk ? size_t(count - chunk) * recBytes : size_t(0); };
    if (most > chunk)
      if (int rc = comm_exchange(ctx->comm, ctx->stream, sL + first, rest(ownL), sR + first, rest(ownR), rL + first,
                                 rest(got[0]), rR + first, rest(got[1]))) {
        ctx->err = "slab exchange: " + ctx->comm->err;
        return rc;
      }
    return PBF_OK;
  };
  // ---- round 1: particles whose cell column left the slab move to the neighbour -------------------------------
  uint32_t got[2];
  if (int rc = round(mL, mR, ctx->capMig, sizeof(MigrantRec<N>), 0, 1, got)) return rc;
  const uint32_t leavers = h[0] + h[1], arrived = got[0] + got[1];
  if (size_t(nPrev) + arrived > ctx->cap) return fail(ctx, PBF_ERR_INVALID, "particle capacity exceeded: call pbf_reserve");
  if (arrived) {
    hipLaunchKernelGGL((k_append_migrants_h<N>), grid_for(arrived), dim3(BLOCK), 0, ctx->stream, nPrev,
                       reinterpret_cast<const MigrantRec<N> *>(rL + WIRE_HDR), got[0],
                       reinterpret_cast<const MigrantRec<N> *>(rR + WIRE_HDR), got[1], ctx->shiftL, ctx->shiftR,
                       arrays<N>(ctx, a, ctx->st.pcur), c.tableN, ctx->count.as<uint32_t>(), ctx->cellSlot.as<uint32_t>());
    hipLaunchKernelGGL((k_slab_arrival_ghosts<N>), dim3(1), dim3(BLOCK), 0, ctx->stream, nPrev, arrived, sc,
                       arrays<N>(ctx, a, ctx->st.pcur), tot, reinterpret_cast<GhostRec<N> *>(gL + WIRE_HDR),
                       reinterpret_cast<GhostRec<N> *>(gR + WIRE_HDR), reinterpret_cast<uint32_t *>(gL),
                       reinterpret_cast<uint32_t *>(gR), ctx->wireCap, ctx->ghostSrcL.as<uint32_t>(), ctx->ghostSrcR.as<uint32_t>());
    LAUNCH_CHECK(ctx);
  }
  // ---- round 2: copies of the boundary columns -------------------------------------------------------------------
  if (int rc = round(gL, gR, ctx->capGhost, sizeof(GhostRec<N>), 2, 3, got)) return rc;
  ctx->sentL = h[2], ctx->sentR = h[3];
  const uint32_t copies = got[0] + got[1];
  if (size_t(nPrev) + arrived + copies > ctx->cap) return fail(ctx, PBF_ERR_INVALID, "particle capacity exceeded: call pbf_reserve");
  ctx->ghostAt = nPrev + arrived;
  if (copies) {
    hipLaunchKernelGGL((k_append_ghosts_h<N>), grid_for(copies), dim3(BLOCK), 0, ctx->stream, ctx->ghostAt,
                       reinterpret_cast<const GhostRec<N> *>(rL + WIRE_HDR), got[0],
                       reinterpret_cast<const GhostRec<N> *>(rR + WIRE_HDR), got[1], ctx->shiftL, ctx->shiftR,
                       arrays<N>(ctx, a, ctx->st.pcur), c.tableN, ctx->count.as<uint32_t>(), ctx->cellSlot.as<uint32_t>());
    LAUNCH_CHECK(ctx);
    ctx->hasObstacles = true;  // "special" particles exist: the kernels must look at type[]
  }
  ctx->gotL = got[0], ctx->gotR = got[1];
  ctx->n = size_t(nPrev) + arrived + copies;                      // slots, dead ones included
  ctx->sortLive = ctx->n - oldCopies - leavers;                   // what the sort keeps
  ctx->nOwned = uint32_t(ctx->sortLive - copies);
  ctx->slabActive = true;
  ctx->st.histogram_current(c.tableN);
  if (int rc = stage_sort<N>(ctx, p)) return rc;
  if (int rc = stage_diffuse<N>(ctx, p, /*overlap=*/p->iteration > 0)) return rc;  // beside the iterations, like pbf_step
  // ---- K x { lambda, delta-p }, each followed by the owners refreshing their copies' {pStar, lambda} ------
  const size_t fb = sizeof(vec4<N>);
  auto refresh = [&]() -> int {
    if (int rc = slab_pack<N>(ctx, ctx->wireSend[0].p, ctx->wireSend[1].p)) return rc;
    if (int rc = exchange(ctx, ctx->sentL * fb, ctx->sentR * fb, ctx->gotL * fb, ctx->gotR * fb)) return rc;
    return slab_unpack<N>(ctx, ctx->wireRecv[0].p, ctx->wireRecv[1].p);
  };
  for (uint64_t it = 0; it < p->iteration; ++it) {
    if (int rc = stage_lambda<N>(ctx, p)) return rc;
    if (int rc = refresh()) return rc;
    if (int rc = stage_delta<N>(ctx, p)) return rc;
    if (int rc = refresh()) return rc;
  }
  if (int rc = stage_finalise<N>(ctx, p)) return rc;
  if (extras_on(ctx, p))  // (surface tension is refused by pbf_slab_steps before anything runs)
    if (int rc = DISPATCH_FAST(ctx, slab_extras_impl, ctx, p)) return rc;
  if (int rc = join_diffuse(ctx)) return rc;
  // The copies stay where they are: the next step's predict marks them dead and its sort drops them; whoever looks at
  // the arrays from outside calls drop_ghosts() first.
  ctx->ghostsPending = true;
  return PBF_OK;
}

}  // namespace

extern "C" {

const char *pbf_comm_last_error(const pbf_comm *comm) { return comm ? comm->err.c_str() : g_comm_error.c_str(); }
uint64_t pbf_comm_rounds(const pbf_comm *comm) { return comm ? comm->rounds : 0; }

int pbf_comm_unique_id(void *id128) {
  if (!id128) return PBF_ERR_INVALID;
  pbf_comm tmp;
  if (!comm_load_rccl(&tmp)) {
    g_comm_error = tmp.err;
    return PBF_ERR_COMM;
  }
  ncclUniqueId id;
  const ncclResult_t r = tmp.fGetUniqueId(&id);
  if (r != ncclSuccess) {
    g_comm_error = std::string("ncclGetUniqueId: ") + tmp.fErrorString(r);
    return PBF_ERR_COMM;
  }
  static_assert(sizeof(id) == PBF_COMM_ID_BYTES, "ncclUniqueId size");
  std::memcpy(id128, &id, sizeof(id));
  return PBF_OK;
}

int pbf_comm_create_rccl(const void *id128, int nranks, int rank, int device, pbf_comm **out) {
  if (!id128 || !out || nranks < 1 || rank < 0 || rank >= nranks) {
    g_comm_error = "pbf_comm_create_rccl: bad argument";
    return PBF_ERR_INVALID;
  }
  *out = nullptr;
  auto *c = new pbf_comm();
  c->nranks = nranks, c->rank = rank, c->device = device;
  if (!comm_load_rccl(c)) {
    g_comm_error = c->err;
    delete c;
    return PBF_ERR_COMM;
  }
  if (hipSetDevice(device) != hipSuccess) {
    g_comm_error = "hipSetDevice failed";
    delete c;
    return PBF_ERR_HIP;
  }
  ncclUniqueId id;
  std::memcpy(&id, id128, sizeof(id));
  const ncclResult_t r = c->fCommInitRank(&c->comm, nranks, id, rank);
  if (r != ncclSuccess) {
    g_comm_error = std::string("ncclCommInitRank: ") + c->fErrorString(r);
    delete c;
    return PBF_ERR_COMM;
  }
  *out = c;
  return PBF_OK;
}

int pbf_comm_create_host_callback(pbf_exchange_fn fn, void *user, int nranks, int rank, pbf_comm **out) {
  if (!fn || !out || nranks < 1 || rank < 0 || rank >= nranks) {
    g_comm_error = "pbf_comm_create_host_callback: bad argument";
    return PBF_ERR_INVALID;
  }
  auto *c = new pbf_comm();
  c->nranks = nranks, c->rank = rank, c->fn = fn, c->user = user;
  *out = c;
  return PBF_OK;
}

void pbf_comm_destroy(pbf_comm *c) {
  if (!c) return;
  if (c->comm && c->fCommDestroy) (void)c->fCommDestroy(c->comm);
  for (void *h : c->host)
    if (h) (void)hipHostFree(h);
  delete c;  // (the dlopen handle stays: other communicators / the hosting process may use librccl)
}

int pbf_comm_allreduce_u32(pbf_comm *c, void *device_u32, size_t count, void *stream) {
  if (!c || !device_u32) return PBF_ERR_INVALID;
  if (!c->comm) {
    c->err = "pbf_comm_allreduce_u32 needs an RCCL communicator";
    return PBF_ERR_COMM;
  }
  const ncclResult_t r = c->fAllReduce(device_u32, device_u32, count, ncclUint32, ncclSum, c->comm, static_cast<hipStream_t>(stream));
  return r == ncclSuccess ? PBF_OK : comm_fail(c, "ncclAllReduce", r);
}

int pbf_slab_set_cuts(pbf_ctx *ctx, const uint32_t *cuts) {
  if (int rc = slab_check(ctx)) return rc;
  if (!ctx->comm || !cuts) return fail(ctx, PBF_ERR_STATE, "pbf_slab_set_cuts needs pbf_slab_attach first");
  const int n = ctx->comm->nranks;
  for (int g = 0; g < n; ++g)
    if (cuts[g + 1] <= cuts[g]) return fail(ctx, PBF_ERR_INVALID, "cuts must be strictly increasing");
  ctx->cuts.assign(cuts, cuts + n + 1);
  return apply_cuts(ctx);
}

int pbf_slab_attach(pbf_ctx *ctx, pbf_comm *comm, const uint32_t *cuts, uint32_t cap_migrants, uint32_t cap_ghosts) {
  if (int rc = slab_check(ctx)) return rc;
  if (!comm || !cuts || !cap_migrants || !cap_ghosts) return fail(ctx, PBF_ERR_INVALID, "NULL / zero argument");
  ctx->comm = comm;
  ctx->capMig = cap_migrants, ctx->capGhost = cap_ghosts;
  const size_t mig = ctx->fp64 ? sizeof(MigrantRec<double>) : sizeof(MigrantRec<float>);
  const size_t gho = ctx->fp64 ? sizeof(GhostRec<double>) : sizeof(GhostRec<float>);
  // the buffers hold far more than the first message: half the particle capacity per neighbour (whole columns change
  // hands after a re-cut) — a few hundred MB at most, nothing against 288 GB of HBM
  ctx->wireCap = uint32_t(std::max<size_t>(std::max<size_t>(ctx->cap, ctx->reserve) / 2, 4 * size_t(std::max(cap_migrants, cap_ghosts))));
  const size_t bytes = WIRE_HDR + size_t(ctx->wireCap) * std::max(mig, gho);
  for (int k = 0; k < 2; ++k) {
    if (int rc = ensure(ctx, ctx->wireSend[k], bytes)) return rc;
    if (int rc = ensure(ctx, ctx->wireRecv[k], bytes)) return rc;
    if (int rc = ensure(ctx, ctx->wireGhost[k], bytes)) return rc;
  }
  HIPCHK(ctx, ctx->hostCounts.ensure(16));
  return pbf_slab_set_cuts(ctx, cuts);
}

int pbf_slab_step(pbf_ctx *ctx, const pbf_params *p) { return pbf_slab_steps(ctx, p, 1); }
int pbf_slab_steps(pbf_ctx *ctx, const pbf_params *p, uint32_t count) {
  if (int rc = check(ctx, p, false)) return rc;
  if (collider_on(ctx) || scenery_on(ctx)) return fail(ctx, PBF_ERR_STATE, kColliderSlabError);  // (set before the ctx was configured or attached)
  if (!ctx->comm) return fail(ctx, PBF_ERR_STATE, "pbf_slab_step needs pbf_slab_attach first");
  if (surface_on(ctx))
    return fail(ctx, PBF_ERR_STATE, "surface tension is not supported in slab mode (pbf_set_surface_tension(ctx, 0, 0) turns it off)");
  if (scene_on(ctx)) return fail(ctx, PBF_ERR_STATE, kSceneSlabError);
  // finalise(t) + predict(t + 1) as one kernel between two steps of THIS call (same parameters, same cuts, nothing looks
  // at the state in between) — like pbf_steps
  const bool timed = (ctx->desc.flags & PBF_FLAG_STAGE_TIMING) != 0 &&
                     (((ctx->timingMask >> ST_PREDICT) & 1u) != 0 || ((ctx->timingMask >> ST_FINALISE) & 1u) != 0);
  const bool fusable = ctx->fusePredict && !timed && !extras_on(ctx, p);
  for (uint32_t i = 0; i < count; ++i) {
    ctx->fuseNextPredict = fusable && i + 1 < count;
    if (int rc = DISPATCH(ctx, slab_step_impl, ctx, p)) {
      ctx->fuseNextPredict = false;
      (void)ctx->st.take_prediction();
      return rc;
    }
  }
  ctx->fuseNextPredict = false;
  return PBF_OK;
}
uint64_t pbf_slab_host_syncs(const pbf_ctx *ctx) { return ctx ? ctx->slabHostSyncs : 0; }

}  // extern "C"

// ================================================================================================
// Marching-cubes surface (pbf_surface / pbf_download_mesh): reference src/omp/ompsph.hpp:277-477
// ================================================================================================
namespace {

// pbf_surface_anisotropic's field stage (csrc/pbf_aniso_field.hpp): AnisotropyOp into ctx->anisoOut exactly as
// pbf_anisotropy_compute launches it, with no copies back; its planes packed into one record per particle; the field; the far
// nodes' colours.  mcNear is already marked.
template <typename N, bool FAST>
int aniso_field_stage(pbf_ctx *ctx, const StepConsts<N> &c, const McConsts<N> &m, const pbf_anisotropy *kernel) {
  const uint32_t n = uint32_t(ctx->n);
  const int s = ctx->st.cur;
  AnisoPlanes l(ctx->cap, sizeof(N));
  if (int rc = ensure(ctx, ctx->anisoRec, size_t(3) * std::max<size_t>(ctx->cap, n) * sizeof(vec4<N>))) return rc;
  if (int rc = anisotropy_launch<N, FAST>(ctx, c, kernel, l)) return rc;
  hipLaunchKernelGGL((k_aniso_pack<N>), grid_for(n), dim3(BLOCK), 0, ctx->stream, n, N(c.h * c.scale), c.scale, c.hasObstacles,
                     ctx->pos4[s].as<const vec4<N>>(), ctx->type[s].as<const uint8_t>(), l.at<const N>(l.centre),
                     l.at<const N>(l.G), l.at<const N>(l.radii), ctx->anisoRec.as<vec4<N>>());
  const uint64_t nodeBlocks = uint64_t((m.planes + 3) / 4) * ((m.sample[1] + 3) / 4) * ((m.sample[2] + 3) / 4);
  hipLaunchKernelGGL((k_mc_field_aniso<N>), grid_for(nodeBlocks * 64), dim3(BLOCK), 0, ctx->stream, m,
                     ctx->table.as<const uint32_t>(), ctx->anisoRec.as<const vec4<N>>(), ctx->col4[s].as<const vec4<N>>(),
                     ctx->mcNear.as<const uint32_t>(), ctx->latticePN.as<vec4<N>>(), ctx->latticeC.as<vec4<N>>());
  hipLaunchKernelGGL((k_mc_fill_far<N>), grid_for(size_t(m.sample[0]) * m.sample[1] * m.sample[2]), dim3(BLOCK), 0, ctx->stream,
                     m.sample[0], m.sample[1], m.sample[2], ctx->latticePN.as<const vec4<N>>(), ctx->latticeC.as<vec4<N>>());
  return PBF_OK;
}

// `nVertices` non-NULL: the indexed mesh (pbf_surface_indexed) — same field, count and scan, then one vertex per crossed
// lattice edge and index triples instead of k_mc_emit's three private vertices per triangle
// `aniso` non-NULL: pbf_surface_anisotropic — the same lattice, count, scans and emission around another field stage; never in
// slab mode, and nothing is launched or changed before its last refusal
template <typename N>
int surface_impl(pbf_ctx *ctx, const pbf_params *p, const pbf_mc_params *mp, uint64_t *nTriangles, uint64_t *nVertices,
                 const pbf_anisotropy *aniso = nullptr) {
  const bool indexed = nVertices != nullptr;
  StepConsts<N> c;
  if (aniso) {
    if (int rc = consts_on_last_grid<N>(ctx, p, c, "pbf_surface_anisotropic")) return rc;
  } else if (int rc = make_consts<N>(ctx, p, c)) {
    return rc;
  }
  // Slab mode (after pbf_slab_step; the copies of the neighbours' boundary columns are still in the arrays): every rank
  // extracts the part of the GLOBAL lattice whose nodes lie in its own cell columns — the ghost layer supplies exactly the
  // 27-cell neighbourhoods those nodes need — after refreshing the copies' colours (the owners diffused them during the
  // step), receives the one node plane its last cubes share with the right-hand neighbour, and emits its cubes'
  // triangles: the ranks' meshes, concatenated in rank order, ARE the single-device mesh's cube order (x-major).
  if (!aniso)
    if (int rc = materialise_pstar<N>(ctx)) return rc;  // (slab mode reads the copies' pStar)
  const bool slab = ctx->slabConfigured && ctx->comm && ctx->comm->nranks > 1;
  if (ctx->slabConfigured && !slab) return fail(ctx, PBF_ERR_STATE, "pbf_surface in slab mode needs pbf_slab_attach");
  if (slab && !ctx->ghostsPending) return fail(ctx, PBF_ERR_STATE, "pbf_surface in slab mode must follow pbf_slab_step directly");
  McConsts<N> m;
  m.scale = c.scale, m.res = N(mp->resolution), m.isolevel = N(mp->isolevel), m.particleSize = N(mp->particle_size);
  m.particleInfluence = N(mp->particle_influence);
  m.step = c.h / m.res;           // ompsph.hpp:291
  m.threshold = c.h * c.scale * 1;  // ompsph.hpp:293
  uint64_t sampleG[3];
  for (int k = 0; k < 3; ++k) {
    m.minExtent[k] = c.minExtent[k];
    m.extent[k] = uint32_t(ctx->extent[k]);   // (global: make_consts leaves ctx->extent untouched by the slab frame)
    sampleG[k] = uint64_t(std::floor(N(ctx->extent[k]) * m.res)) + 1;  // ompsph.hpp:283-284
    m.sample[k] = uint32_t(sampleG[k]);
  }
  m.xoff = 0, m.nodeX0 = 0, m.planes = m.sample[0];
  bool hasRight = false;
  if (slab) {
    const int r = ctx->comm->rank, nr = ctx->comm->nranks;
    // first global node x whose cell column floor(x / res) is >= col: the smallest integer x with x / res >= col (in N,
    // like the kernel's own division)
    auto first_node = [&](uint32_t col) {
      uint64_t x = uint64_t(std::ceil(N(col) * m.res));
      while (x > 0 && uint64_t(N(x - 1) / m.res) >= col) --x;
      while (uint64_t(N(x) / m.res) < col) ++x;
      return std::min<uint64_t>(x, sampleG[0]);
    };
    // every rank's first node plane, from the cuts all ranks share: rank g owns the planes [firstX[g], firstX[g + 1])
    std::vector<uint64_t> firstX(size_t(nr) + 1, 0);
    for (int g = 1; g < nr; ++g) firstX[g] = first_node(ctx->cuts[g]);
    firstX[nr] = sampleG[0];
    // A rank between two others that owns no plane while nodes remain to its right cannot hand its left neighbour the plane
    // that neighbour's last cubes need (it belongs to a rank further right; the exchange reaches one rank).  Refused on
    // every rank alike, before anything is exchanged.  (A rank with no plane and none to its right is fine.)
    for (int g = 1; g + 1 < nr; ++g)
      if (firstX[g] == firstX[g + 1] && firstX[g + 1] < sampleG[0]) {
        std::string cuts;
        for (int k = 0; k <= nr; ++k) cuts += (k ? ", " : "") + std::to_string(ctx->cuts[k]);
        return fail(ctx, PBF_ERR_INVALID,
                    "pbf_surface in slab mode: rank " + std::to_string(g) + " (columns [" + std::to_string(ctx->cuts[g]) + ", " +
                        std::to_string(ctx->cuts[g + 1]) + ") of the cuts {" + cuts + "}) owns no lattice node plane at resolution " +
                        std::to_string(mp->resolution) + ": widen the slab or raise the resolution");
      }
    const uint64_t x0 = firstX[r], x1 = firstX[r + 1];
    hasRight = r + 1 < nr && x1 < sampleG[0];
    m.xoff = ctx->xoff, m.nodeX0 = uint32_t(x0), m.planes = uint32_t(x1 - x0);
    m.sample[0] = m.planes + (hasRight ? 1u : 0u);
    // the owners' diffused colours -> their copies on the neighbours (one more field round; the copies' pStar is current)
    const size_t fb = sizeof(vec4<N>);
    vec4<N> *col = ctx->col4[ctx->st.cur].as<vec4<N>>();
    if (int rc = slab_pack<N>(ctx, ctx->wireSend[0].p, ctx->wireSend[1].p, col)) return rc;
    if (int rc = exchange(ctx, ctx->sentL * fb, ctx->sentR * fb, ctx->gotL * fb, ctx->gotR * fb)) return rc;
    if (int rc = slab_unpack<N>(ctx, ctx->wireRecv[0].p, ctx->wireRecv[1].p, col)) return rc;
  }
  const uint64_t planeN = uint64_t(m.sample[1]) * m.sample[2];
  const uint64_t latticeN = uint64_t(m.sample[0]) * planeN;
  if (latticeN >= (uint64_t(1) << 31)) return fail(ctx, PBF_ERR_INVALID, "surface lattice too large (resolution x extent)");
  // (the 32-bit scan of up to three vertices per node must not wrap before the 2^29 test below sees its total)
  if (indexed && 3 * latticeN >= (uint64_t(1) << 32)) return fail(ctx, PBF_ERR_INVALID, "surface lattice too large for an indexed mesh");
  for (int k = 0; k < 3; ++k) ctx->mcSample[k] = m.sample[k];  // (from here on the readers see this call's lattice)
  m.tableN = c.tableN, m.hasObstacles = c.hasObstacles;
  const int s = ctx->st.cur;
  if (int rc = ensure(ctx, ctx->latticePN, (latticeN + 1) * sizeof(vec4<N>))) return rc;
  if (int rc = ensure(ctx, ctx->latticeC, (latticeN + 1) * sizeof(vec4<N>))) return rc;
  *nTriangles = 0;
  ctx->mcTriangles = 0;
  ctx->meshStaged = false;
  ctx->meshKind = indexed ? pbf_ctx::MESH_INDEXED : pbf_ctx::MESH_SOUP;
  ctx->mcVertices = 0;
  if (indexed) *nVertices = 0;
  if (m.planes) {
    // which of a cell's 27 slots hold particles (most lattice nodes sit in empty space and skip their gather)
    if (int rc = ensure(ctx, ctx->mcNear, (size_t(c.tableN) + 64) * 4)) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->mcNear.p, 0, size_t(c.tableN) * 4, ctx->stream));
    hipLaunchKernelGGL(k_mc_mark_near, grid_for(c.tableN), dim3(BLOCK), 0, ctx->stream, c.tableN,
                       make_uint3(m.extent[0], m.extent[1], m.extent[2]), m.xoff, ctx->table.as<const uint32_t>(),
                       ctx->mcNear.as<uint32_t>());
    const uint64_t nodeBlocks = uint64_t((m.planes + 3) / 4) * ((m.sample[1] + 3) / 4) * ((m.sample[2] + 3) / 4);
    if (aniso) {
      if (int rc = DISPATCH_FAST(ctx, aniso_field_stage, ctx, c, m, aniso)) return rc;
    } else {
      hipLaunchKernelGGL((k_mc_field<N>), grid_for(nodeBlocks * 64), dim3(BLOCK), 0, ctx->stream, m, ctx->table.as<const uint32_t>(),
                         ctx->pos4[s].as<const vec4<N>>(), ctx->pstar[ctx->st.pcur].as<const vec4<N>>(), ctx->col4[s].as<const vec4<N>>(),
                         ctx->type[s].as<const uint8_t>(), ctx->mcNear.as<const uint32_t>(), ctx->latticePN.as<vec4<N>>(),
                         ctx->latticeC.as<vec4<N>>());
    }
    LAUNCH_CHECK(ctx);
  }
  if (slab) {  // my first node plane -> the left neighbour's extra plane (two rounds: {v, normal} and colours)
    const size_t pb = size_t(planeN) * sizeof(vec4<N>);
    const bool sendLeft = ctx->comm->rank > 0 && m.planes > 0;
    for (DevBuf *lat : {&ctx->latticePN, &ctx->latticeC}) {
      uint8_t *base = lat->as<uint8_t>();
      if (int rc = comm_exchange(ctx->comm, ctx->stream, base, sendLeft ? pb : 0, nullptr, 0, nullptr, 0,
                                 base + size_t(m.planes) * pb, hasRight ? pb : 0)) {
        ctx->err = "slab surface exchange: " + ctx->comm->err;
        return rc;
      }
    }
  }
  if (m.sample[0] < 2 || m.sample[1] < 2 || m.sample[2] < 2) return PBF_OK;
  const uint64_t march64 = uint64_t(m.sample[0] - 1) * (m.sample[1] - 1) * (m.sample[2] - 1);
  const uint32_t marchVolume = uint32_t(march64), len = marchVolume + 1;
  const uint32_t nb = (len + SCAN_TILE - 1) / SCAN_TILE;
  if (int rc = ensure(ctx, ctx->mcCounts, (size_t(len) + SCAN_TILE) * 4)) return rc;
  if (int rc = ensure(ctx, ctx->mcOffsets, (size_t(len) + SCAN_TILE) * 4)) return rc;
  if (int rc = ensure(ctx, ctx->mcSums, (size_t(nb) + 1) * 4)) return rc;
  uint32_t *counts = ctx->mcCounts.as<uint32_t>(), *offsets = ctx->mcOffsets.as<uint32_t>(), *sums = ctx->mcSums.as<uint32_t>();
  HIPCHK(ctx, hipMemsetAsync(counts + marchVolume, 0, 4, ctx->stream));  // closing sentinel: offsets[marchVolume] = total
  hipLaunchKernelGGL((k_mc_count<N>), grid_for(marchVolume), dim3(BLOCK), 0, ctx->stream, m, marchVolume,
                     ctx->latticePN.as<const vec4<N>>(), counts);
  launch_scans(ctx, scan_job(counts, len, sums, offsets), 1);
  LAUNCH_CHECK(ctx);
  uint32_t total = 0, totalV = 0;
  const uint32_t nodes = uint32_t(latticeN);
  if (indexed) {  // crossed edges per owner node and their scan, ahead of the one read-back both totals share
    const uint32_t elen = nodes + 1, enb = (elen + SCAN_TILE - 1) / SCAN_TILE;
    if (int rc = ensure(ctx, ctx->mcEdgeWord, (size_t(elen) + SCAN_TILE) * 4)) return rc;
    if (int rc = ensure(ctx, ctx->mcEdgeOffsets, (size_t(elen) + SCAN_TILE) * 4)) return rc;
    if (int rc = ensure(ctx, ctx->mcEdgeSums, (size_t(enb) + 1) * 4)) return rc;
    uint32_t *ew = ctx->mcEdgeWord.as<uint32_t>(), *eo = ctx->mcEdgeOffsets.as<uint32_t>();
    HIPCHK(ctx, hipMemsetAsync(ew + nodes, 0, 4, ctx->stream));  // closing sentinel: eo[nodes] = total
    hipLaunchKernelGGL((k_mc_edge_mark<N>), grid_for(nodes), dim3(BLOCK), 0, ctx->stream, m, nodes,
                       ctx->latticePN.as<const vec4<N>>(), ew);
    launch_scans(ctx, scan_job(ew, elen, ctx->mcEdgeSums.as<uint32_t>(), eo), 1);
    LAUNCH_CHECK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(&totalV, eo + nodes, 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(ctx, hipMemcpyAsync(&total, offsets + marchVolume, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the mesh buffers are sized from the count
  if (indexed) {
    if (totalV >= (1u << 29)) return fail(ctx, PBF_ERR_INVALID, "indexed mesh: 2^29 vertices or more");
    ctx->mcTriangles = total, ctx->mcVertices = totalV;
    *nTriangles = total, *nVertices = totalV;
    if (total == 0) return PBF_OK;  // (no triangle <=> no crossed edge: every lattice edge belongs to a cube)
    if (int rc = ensure(ctx, ctx->meshV, size_t(totalV) * 3 * sizeof(N))) return rc;
    if (int rc = ensure(ctx, ctx->meshN, size_t(totalV) * 3 * sizeof(N))) return rc;
    if (int rc = ensure(ctx, ctx->meshC, size_t(totalV) * 4 * sizeof(N))) return rc;
    if (int rc = ensure(ctx, ctx->meshT, size_t(total) * 3 * 4)) return rc;
    hipLaunchKernelGGL((k_mc_emit_vertices<N>), grid_for(nodes), dim3(BLOCK), 0, ctx->stream, m, nodes,
                       ctx->latticePN.as<const vec4<N>>(), ctx->latticeC.as<const vec4<N>>(),
                       ctx->mcEdgeOffsets.as<const uint32_t>(), ctx->mcEdgeWord.as<uint32_t>(), ctx->meshV.as<N>(),
                       ctx->meshN.as<N>(), ctx->meshC.as<N>());
    hipLaunchKernelGGL((k_mc_emit_indices<N>), grid_for(marchVolume), dim3(BLOCK), 0, ctx->stream, m, marchVolume,
                       ctx->latticePN.as<const vec4<N>>(), offsets, ctx->mcEdgeWord.as<const uint32_t>(),
                       ctx->meshT.as<uint32_t>());
    LAUNCH_CHECK(ctx);
    return PBF_OK;
  }
  ctx->mcTriangles = total;
  *nTriangles = total;
  if (total == 0) return PBF_OK;
  if (int rc = ensure(ctx, ctx->meshV, size_t(total) * 9 * sizeof(N))) return rc;
  if (int rc = ensure(ctx, ctx->meshN, size_t(total) * 9 * sizeof(N))) return rc;
  if (int rc = ensure(ctx, ctx->meshC, size_t(total) * 12 * sizeof(N))) return rc;
  hipLaunchKernelGGL((k_mc_emit<N>), grid_for(marchVolume), dim3(BLOCK), 0, ctx->stream, m, marchVolume,
                     ctx->latticePN.as<const vec4<N>>(), ctx->latticeC.as<const vec4<N>>(), offsets, ctx->meshV.as<N>(),
                     ctx->meshN.as<N>(), ctx->meshC.as<N>());
  LAUNCH_CHECK(ctx);
  return PBF_OK;
}

// The last mesh's arrays, as (device buffer, bytes) parts in the order the caller names them.
struct MeshPart {
  const DevBuf *dev;
  size_t bytes;
};
// each part the caller asked for, straight into its array
int download_mesh_parts(pbf_ctx *ctx, std::initializer_list<MeshPart> parts, void *const *host) {
  for (const MeshPart &part : parts)
    if (void *to = *host++) HIPCHK(ctx, hipMemcpyAsync(to, part.dev->p, part.bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PBF_OK;
}
// the parts staged once per surface, back to back in the pinned buffer (grown when they do not fit); at[k]: where part k begins
int map_mesh_parts(pbf_ctx *ctx, std::initializer_list<MeshPart> parts, const void **at) {
  size_t total = 0;
  for (const MeshPart &part : parts) total += part.bytes;
  if (ctx->meshHost.count < total) {
    HIPCHK(ctx, ctx->meshHost.ensure(total + total / 4 + 4096, /*zero=*/false));
    ctx->meshStaged = false;
  }
  char *h = ctx->meshHost.p;
  for (const MeshPart &part : parts) {
    if (!ctx->meshStaged) HIPCHK(ctx, hipMemcpyAsync(h, part.dev->p, part.bytes, hipMemcpyDeviceToHost, ctx->stream));
    *at++ = h, h += part.bytes;
  }
  // (one wait behind all the parts: handing the arrays out one by one, an event behind each, so that the caller's copy of the
  // vertices overlaps the normals' DMA was measured — no faster at 0.75 M vertices, 11 % slower at 1.35 M: the host copies
  // and the DMA share the memory system)
  if (!ctx->meshStaged) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->meshStaged = true;
  return PBF_OK;
}

}  // namespace

extern "C" {

int pbf_surface(pbf_ctx *ctx, const pbf_params *params, const pbf_mc_params *mc, uint64_t *n_triangles) {
  if (int rc = check(ctx, params, true)) return rc;

  if (!mc || !n_triangles) return fail(ctx, PBF_ERR_INVALID, "NULL argument");
  if (!(mc->resolution > 0)) return fail(ctx, PBF_ERR_INVALID, "resolution must be > 0");
  return DISPATCH(ctx, surface_impl, ctx, params, mc, n_triangles, static_cast<uint64_t *>(nullptr));
}

int pbf_surface_indexed(pbf_ctx *ctx, const pbf_params *params, const pbf_mc_params *mc, uint64_t *n_vertices,
                        uint64_t *n_triangles) {
  // an edge on a cut plane has its owner on another rank: the vertex numbering would need a scan across ranks
  if (ctx && ctx->slabConfigured) return fail(ctx, PBF_ERR_STATE, "pbf_surface_indexed is not supported in slab mode");
  if (int rc = check(ctx, params, true)) return rc;

  if (!mc || !n_vertices || !n_triangles) return fail(ctx, PBF_ERR_INVALID, "NULL argument");
  if (!(mc->resolution > 0)) return fail(ctx, PBF_ERR_INVALID, "resolution must be > 0");
  return DISPATCH(ctx, surface_impl, ctx, params, mc, n_triangles, n_vertices);
}

int pbf_surface_anisotropic(pbf_ctx *ctx, const pbf_params *params, const pbf_aniso_surface *cfg, int indexed,
                            uint64_t *n_vertices, uint64_t *n_triangles) {
  if (!ctx) return PBF_ERR_INVALID;
  const std::string who("pbf_surface_anisotropic: ");
  if (!params || !cfg || !n_triangles) return fail(ctx, PBF_ERR_INVALID, who + "NULL argument");
  if (indexed && !n_vertices) return fail(ctx, PBF_ERR_INVALID, who + "an indexed mesh needs n_vertices");
  const Refuse refuse{ctx, "pbf_surface_anisotropic"};
  if (int rc = refuse.params(params)) return rc;
  if (!(cfg->resolution > 0) || !std::isfinite(cfg->resolution) || !(cfg->isolevel > 0) || !std::isfinite(cfg->isolevel))
    return fail(ctx, PBF_ERR_INVALID, who + "resolution and isolevel must be finite and > 0");
  if (const char *why = anisotropy_config_error(&cfg->kernel)) return fail(ctx, PBF_ERR_INVALID, who + why);
  // a particle near a cut needs both ranks' candidates (pbf_anisotropy_compute), and so does a node
  if (int rc = refuse.slab_mode()) return rc;
  if (ctx->n == 0) {  // an empty surface of this call's kind, and no lattice
    ctx->mcTriangles = ctx->mcVertices = 0;
    ctx->meshStaged = false;
    ctx->meshKind = indexed ? pbf_ctx::MESH_INDEXED : pbf_ctx::MESH_SOUP;
    ctx->mcSample[0] = ctx->mcSample[1] = ctx->mcSample[2] = 0;
    *n_triangles = 0;
    if (indexed) *n_vertices = 0;
    return PBF_OK;
  }
  if (int rc = refuse.no_step()) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const pbf_mc_params mc{cfg->resolution, cfg->isolevel, 0.0, 0.0};  // (size and influence belong to the stock field)
  return DISPATCH(ctx, surface_impl, ctx, params, &mc, n_triangles, indexed ? n_vertices : static_cast<uint64_t *>(nullptr),
                  &cfg->kernel);
}

int pbf_download_mesh_indexed(pbf_ctx *ctx, void *vs, void *ns, void *cs, uint32_t *tris) {
  if (!ctx) return PBF_ERR_INVALID;
  if (ctx->meshKind == pbf_ctx::MESH_SOUP)
    return fail(ctx, PBF_ERR_STATE, "the last surface is a triangle soup (pbf_surface): pbf_download_mesh reads it");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t nv = ctx->mcVertices, nt = ctx->mcTriangles, e = ctx->fp64 ? 8 : 4;
  if (nt == 0) return PBF_OK;
  void *const host[] = {vs, ns, cs, tris};
  return download_mesh_parts(
      ctx, {{&ctx->meshV, nv * 3 * e}, {&ctx->meshN, nv * 3 * e}, {&ctx->meshC, nv * 4 * e}, {&ctx->meshT, nt * 3 * 4}}, host);
}

int pbf_map_mesh_indexed(pbf_ctx *ctx, const void **vs, const void **ns, const void **cs, const uint32_t **tris) {
  if (!ctx || !vs || !ns || !cs || !tris) return PBF_ERR_INVALID;
  *vs = *ns = *cs = nullptr, *tris = nullptr;
  if (ctx->meshKind == pbf_ctx::MESH_SOUP)
    return fail(ctx, PBF_ERR_STATE, "the last surface is a triangle soup (pbf_surface): pbf_map_mesh reads it");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t nv = ctx->mcVertices, nt = ctx->mcTriangles, e = ctx->fp64 ? 8 : 4;
  if (nt == 0) return PBF_OK;
  const void *at[4];
  const int rc = map_mesh_parts(
      ctx, {{&ctx->meshV, nv * 3 * e}, {&ctx->meshN, nv * 3 * e}, {&ctx->meshC, nv * 4 * e}, {&ctx->meshT, nt * 3 * 4}}, at);
  if (rc) return rc;
  *vs = at[0], *ns = at[1], *cs = at[2], *tris = static_cast<const uint32_t *>(at[3]);
  return PBF_OK;
}

int pbf_download_mesh(pbf_ctx *ctx, void *vs, void *ns, void *cs) {
  if (!ctx) return PBF_ERR_INVALID;
  if (ctx->meshKind == pbf_ctx::MESH_INDEXED)
    return fail(ctx, PBF_ERR_STATE, "the last surface is indexed (pbf_surface_indexed): pbf_download_mesh_indexed reads it");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t n = ctx->mcTriangles, e = ctx->fp64 ? 8 : 4;
  if (n == 0) return PBF_OK;
  void *const host[] = {vs, ns, cs};
  return download_mesh_parts(ctx, {{&ctx->meshV, n * 9 * e}, {&ctx->meshN, n * 9 * e}, {&ctx->meshC, n * 12 * e}}, host);
}

int pbf_map_mesh(pbf_ctx *ctx, const void **vs, const void **ns, const void **cs) {
  if (!ctx || !vs || !ns || !cs) return PBF_ERR_INVALID;
  if (ctx->meshKind == pbf_ctx::MESH_INDEXED)
    return fail(ctx, PBF_ERR_STATE, "the last surface is indexed (pbf_surface_indexed): pbf_map_mesh_indexed reads it");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t n = ctx->mcTriangles, e = ctx->fp64 ? 8 : 4;
  *vs = *ns = *cs = nullptr;
  if (n == 0) return PBF_OK;
  const void *at[3];
  if (int rc = map_mesh_parts(ctx, {{&ctx->meshV, n * 9 * e}, {&ctx->meshN, n * 9 * e}, {&ctx->meshC, n * 12 * e}}, at)) return rc;
  *vs = at[0], *ns = at[1], *cs = at[2];
  return PBF_OK;
}

int pbf_read_lattice(pbf_ctx *ctx, uint64_t sample[3], void *pn, void *c) {
  if (!ctx || !sample) return PBF_ERR_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  size_t n = 1;
  for (int k = 0; k < 3; ++k) sample[k] = ctx->mcSample[k], n *= ctx->mcSample[k];
  const size_t v = ctx->fp64 ? sizeof(double4) : sizeof(float4);
  if (n && pn) HIPCHK(ctx, hipMemcpyAsync(pn, ctx->latticePN.p, n * v, hipMemcpyDeviceToHost, ctx->stream));
  if (n && c) HIPCHK(ctx, hipMemcpyAsync(c, ctx->latticeC.p, n * v, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PBF_OK;
}

}  // extern "C"
