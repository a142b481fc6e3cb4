// hipsph.hpp — sph::hip_impl::Solver<T, N, V>: the MI355X backend behind the reference's
// Solver::advance() surface (reference src/sph.hpp:119-125; sibling of omp_impl::Solver,
// src/omp/ompsph.hpp:77-83).  A thin shim: every number is computed by libpbf_hip.so through the
// C ABI in include/pbf_hip.h.  There is no CPU fallback — construction throws if no gfx950 device
// is usable.
//
//   advance()          the reference's contract: xs is uploaded, stepped once, downloaded in Z-order
//                      (like the reference's OpenCL backend re-uploads every frame,
//                      src/ocl/oclsph.cpp:427-473);
//   upload()/step()/download()   the device-resident fast path the benchmark times as well.
//
//   Solver(h, {d0, d1, ...})     several GPUs of one node (reference: the -d/--devices list, src/args.cpp:20-24):
//                      the box is cut into x-slabs with equal particle counts, one ctx + one host thread per
//                      device, every step runs pbf_slab_step on all of them concurrently with the neighbour
//                      exchange over RCCL (ncclSend/ncclRecv, xGMI) inside the library; cuts are re-balanced
//                      every few steps from the all-device column histogram.  Devices listed more than once share
//                      a GPU and exchange through an in-process transport (RCCL refuses two ranks on one GPU):
//                      the same code path, used by the tests on a one-GPU box.
//
// Host-side scene handling restates the observable behaviour of ompsph.hpp:91-126 (sources emit,
// drains erase, empty -> "Particles depleted") and :167-186 (queries).  config.surface runs the
// marching-cubes kernels (pbf_surface) and fills Result::mesh like ompsph.hpp:277-477.
#pragma once

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "pbf_hip.h"
#include "sph.hpp"

namespace sph::hip_impl {

namespace detail {

// One direction of a link between two slabs that share a GPU: the sender posts its (pinned host) buffer, the receiver
// copies it out.  Used through pbf_comm_create_host_callback; never on the RCCL path.
struct Mailbox {
  std::mutex m;
  std::condition_variable cv;
  const void *data = nullptr;
  size_t bytes = 0;
  bool full = false;
  void post(const void *d, size_t n) {
    std::unique_lock<std::mutex> l(m);
    cv.wait(l, [&] { return !full; });
    data = d, bytes = n, full = true;
    cv.notify_all();
  }
  void take(void *dst, size_t n) {
    std::unique_lock<std::mutex> l(m);
    cv.wait(l, [&] { return full; });
    std::memcpy(dst, data, std::min(n, bytes));
    full = false;
    cv.notify_all();
  }
  void drained() {
    std::unique_lock<std::mutex> l(m);
    cv.wait(l, [&] { return !full; });
  }
};
struct InProcessLink {  // rank's view: mailboxes to / from both neighbours
  Mailbox *toLeft = nullptr, *toRight = nullptr, *fromLeft = nullptr, *fromRight = nullptr;
  static int exchange(void *user, const void *sL, size_t nSL, const void *sR, size_t nSR, void *rL, size_t nRL, void *rR,
                      size_t nRR) {
    auto *k = static_cast<InProcessLink *>(user);
    if (nSL && k->toLeft) k->toLeft->post(sL, nSL);
    if (nSR && k->toRight) k->toRight->post(sR, nSR);
    if (nRL && k->fromLeft) k->fromLeft->take(rL, nRL);
    if (nRR && k->fromRight) k->fromRight->take(rR, nRR);
    if (nSL && k->toLeft) k->toLeft->drained();  // our staging buffers are free again once the neighbours copied
    if (nSR && k->toRight) k->toRight->drained();
    return 0;
  }
};

// A fixed crew of host threads, one per slab, that runs f(0) .. f(n - 1) concurrently on every run() call.
class Workers {
  std::vector<std::thread> threads_;
  std::mutex m_;
  std::condition_variable go_, done_;
  std::function<void(size_t)> task_;
  std::vector<std::string> errs_;
  uint64_t epoch_ = 0;
  size_t pending_ = 0;
  bool stop_ = false;

public:
  size_t size() const { return threads_.size(); }
  void start(size_t n) {
    shutdown();
    stop_ = false;
    errs_.assign(n, std::string());
    for (size_t g = 0; g < n; ++g)
      threads_.emplace_back([this, g] {
        uint64_t seen = 0;
        for (;;) {
          std::function<void(size_t)> job;
          {
            std::unique_lock<std::mutex> l(m_);
            go_.wait(l, [&] { return stop_ || epoch_ != seen; });
            if (stop_) return;
            seen = epoch_;
            job = task_;
          }
          std::string err;
          try {
            job(g);
          } catch (const std::exception &e) {
            err = e.what();
          }
          std::unique_lock<std::mutex> l(m_);
          errs_[g] = err;
          if (--pending_ == 0) done_.notify_all();
        }
      });
  }
  void run(std::function<void(size_t)> f) {
    std::unique_lock<std::mutex> l(m_);
    task_ = std::move(f);
    pending_ = threads_.size();
    ++epoch_;
    go_.notify_all();
    done_.wait(l, [&] { return pending_ == 0; });
    for (const auto &e : errs_)
      if (!e.empty()) throw std::runtime_error(e);
  }
  void shutdown() {
    {
      std::unique_lock<std::mutex> l(m_);
      stop_ = true;
      go_.notify_all();
    }
    for (auto &t : threads_) t.join();
    threads_.clear();
  }
  ~Workers() { shutdown(); }
};

// slab.py recut(): particle-count quantiles of the column histogram, each cut moved by at most `maxMove` columns
// (a transferred column always goes to the ADJACENT slab) and slabs kept >= minWidth columns wide.
inline std::vector<uint32_t> recut(const std::vector<uint32_t> &old, const std::vector<uint64_t> &hist, int maxMove = 2,
                                   int minWidth = 4) {
  const int n = int(old.size()) - 1;
  std::vector<uint64_t> cum(hist.size() + 1, 0);
  for (size_t c = 0; c < hist.size(); ++c) cum[c + 1] = cum[c] + hist[c];
  const double total = double(cum.back());
  std::vector<long> nw(old.begin(), old.end());
  auto clampMove = [&](int g) { nw[g] = std::min<long>(std::max<long>(nw[g], long(old[g]) - maxMove), long(old[g]) + maxMove); };
  for (int g = 1; g < n; ++g) {
    const double target = total * g / n;
    nw[g] = long(std::lower_bound(cum.begin(), cum.end(), target, [](uint64_t a, double t) { return double(a) < t; }) - cum.begin());
    clampMove(g);
  }
  for (int g = 1; g < n; ++g) nw[g] = std::max(nw[g], nw[g - 1] + (g > 1 ? minWidth : 1));
  for (int g = n - 1; g > 0; --g) nw[g] = std::min(nw[g], nw[g + 1] - (g < n - 1 ? minWidth : 1));
  for (int g = 1; g < n; ++g) clampMove(g);
  return std::vector<uint32_t>(nw.begin(), nw.end());
}

}  // namespace detail

// V: the vector template of the hosting code base — the reference instantiates its API with glm::vec (src/omp/ompsph.hpp:33),
// this repo's host/sph.hpp ships sph::vec and announces it with PBF_SPH_HAS_VEC, which only supplies a default here.  Built
// against the REFERENCE's own src/sph.hpp (no sph::vec there) the argument is mandatory: oracle/ref_shim.cpp does exactly
// that, so the "copy two headers, add a case" recipe of INTEGRATION.md is compiled, linked and run by the test-suite.
// What V must offer (glm::vec does): x / y / z[/ w] members, V<3>(a, b, c) from mixed arithmetic types, V<3> + V<3>,
// V<3> - V<3>, V<3> * N, and a packed layout.
// The surface as an indexed mesh (pbf_surface_indexed; no reference counterpart, hence declared here and not in sph.hpp):
// one vertex per crossed lattice edge, triangle t = {tris[3t], tris[3t + 1], tris[3t + 2]}; vs[tris[k]] is vertex k of the
// ColouredMesh soup.
template <typename N, template <size_t S, typename C = N> typename V> struct IndexedMesh {
  std::vector<V<3>> vs{}, ns{};
  std::vector<V<4>> cs{};
  std::vector<uint32_t> tris{};
};

// What Solver::sample() / sampleLattice() return: the raw sums of pbf_sample_out (include/pbf_hip.h), one entry per point —
// mv 3 and mc 4 values per point, filled when asked for, count {fluid, obstacle} per point — plus the caller's division:
// velocity = mv / weight and colour = mc / weight, 0 where weight == 0.
template <typename N> struct Samples {
  std::vector<N> rho{}, weight{}, mv{}, mc{}, velocity{}, colour{};
  std::vector<uint32_t> count{};
  std::vector<uint8_t> outside{};
};

// Solver::surfaceAnisotropic()'s configuration: {resolution, isolevel, kernel} (include/pbf_hip.h)
using AnisoSurface = pbf_aniso_surface;

// What Solver::anisotropy() returns: the arrays of pbf_anisotropy_out (include/pbf_hip.h) in device order, COMPONENT-MAJOR —
// value k of particle i at [k * n + i], n = neighbours.size(): centre 3 planes (world), G 6 (xx yy zz xy xz yz, solver frame),
// axes 9 (three unit rows, descending), radii 3.
template <typename N> struct Anisotropy {
  std::vector<N> centre{}, G{}, axes{}, radii{};
  std::vector<uint32_t> neighbours{};
};

// What Solver::whitewaterParticles() returns: the pool of diffuse particles (pbf_whitewater_download, include/pbf_hip.h) —
// positions in world units, velocities as the solver stores them, kind = PBF_WW_SPRAY / _FOAM / _BUBBLE.
template <typename N, template <size_t, typename C = N> typename V> struct WhitewaterParticles {
  std::vector<V<3>> positions{}, velocities{};
  std::vector<N> life{};
  std::vector<uint8_t> kind{};
  std::vector<uint64_t> parentId{};
};

// What Solver::diagnostics() returns: pbf_diag (include/pbf_hip.h) as a plain struct; the density fields are 0 unless asked for.
struct Diagnostics {
  uint64_t fluid = 0, obstacles = 0, nonFinite = 0;
  double mass = 0, moment[3] = {0, 0, 0}, momentum[3] = {0, 0, 0}, kinetic = 0, maxSpeed = 0;
  double aabbMin[3] = {0, 0, 0}, aabbMax[3] = {0, 0, 0};
  uint64_t densityParticles = 0, nbrMax = 0;
  double rhoMin = 0, rhoMax = 0, rhoMean = 0, errMean = 0, errMax = 0, compressionMean = 0, nbrMean = 0;
};

#ifdef PBF_SPH_HAS_VEC
template <typename T, typename N, template <size_t, typename C = N> typename V = sph::vec>
#else
template <typename T, typename N, template <size_t, typename C = N> typename V>
#endif
class Solver final : public sph::Solver<T, N, V> {
  static_assert(std::is_same_v<N, float> || std::is_same_v<N, double>, "N must be float or double");
  static_assert(sizeof(T) == 8, "ids travel as 64-bit (the reference instantiates T = size_t)");
  static_assert(sizeof(V<3>) == 3 * sizeof(N) && sizeof(V<4>) == 4 * sizeof(N), "V must be packed");

  pbf_ctx *ctx_ = nullptr;
  const N h_;
  std::vector<double> wells_;
  std::vector<pbf_source> sources_;  // what step() last pushed to the context (pbf_set_sources / pbf_set_drains)
  std::vector<pbf_drain> drains_;
  // ---- several devices (slabs): ctx_ aliases slabs_[0] ----------------------------------------
  std::vector<int> devices_;
  std::vector<pbf_ctx *> slabs_;
  std::vector<pbf_comm *> comms_;
  std::vector<std::unique_ptr<detail::Mailbox>> boxes_;
  std::vector<detail::InProcessLink> links_;
  std::vector<uint32_t> cuts_;
  uint32_t flags_ = 0;
  uint64_t frame_ = 0;
  unsigned rebalanceEvery_ = 8;
  bool attached_ = false;
  bool indexedFrames_ = false;       // indexedMesh(true): advance() extracts the indexed mesh instead of Result::mesh
  IndexedMesh<N, V> lastIndexed_;
  bool whitewaterOn_ = false;        // whitewater(config) with capacity > 0: advance() runs a whitewater step after the fluid's
  pbf_whitewater_stats whitewaterStats_{};
  bool multi() const { return slabs_.size() > 1; }

  // PBF_SHIM_TIMING=1: mean host time of advance()'s phases, printed by the destructor (diagnostic)
  struct Phases {
    bool on = std::getenv("PBF_SHIM_TIMING") != nullptr;
    double ms[5] = {0, 0, 0, 0, 0};
    uint64_t frames = 0;
  } phase_;
  struct PhaseClock {
    Phases &p;
    std::chrono::steady_clock::time_point t;
    explicit PhaseClock(Phases &ph) : p(ph), t(std::chrono::steady_clock::now()) { p.frames += p.on; }
    void lap(int k) {
      if (!p.on) return;
      const auto n = std::chrono::steady_clock::now();
      p.ms[k] += std::chrono::duration<double, std::milli>(n - t).count();
      t = n;
    }
  };
  // One PERSISTENT host thread per device (round 3: fresh std::threads every step cost ~50 us of creation and join per
  // step): the workers sleep on a condition variable between tasks; errors are rethrown on the caller's thread.
  detail::Workers workers_;
  template <typename F> void parallel(F &&f) {
    if (workers_.size() != slabs_.size()) workers_.start(slabs_.size());
    workers_.run(std::function<void(size_t)>(std::forward<F>(f)));
  }
  void checkOn(size_t g, int rc, const char *what) const {
    if (rc < 0) throw std::runtime_error(std::string(what) + " (device " + std::to_string(devices_[g]) + "): " + pbf_last_error(slabs_[g]));
  }
  uint32_t columnOf(const sph::SphParams<T, N, V> &c, N x) const {  // ompsph.hpp:132-135,152 in N
    const N minExtent = c.minBound.x / c.scale - h_ * 2;
    return uint32_t(int64_t((x / c.scale - minExtent) / h_));
  }

  void check(int rc, const char *what) const {
    if (rc < 0) throw std::runtime_error(std::string(what) + ": " + pbf_last_error(ctx_));
  }

  static pbf_aos_layout layout() {
    using P = sph::Particle<T, N, V>;
    const P probe{};
    auto off = [&](const void *m) {
      return uint32_t(reinterpret_cast<const char *>(m) - reinterpret_cast<const char *>(&probe));
    };
    return {uint32_t(sizeof(P)), off(&probe.id),       off(&probe.type),    off(&probe.mass),
            off(&probe.position), off(&probe.velocity), off(&probe.colour)};
  }

  pbf_params params(const sph::SphParams<T, N, V> &c, const sph::Scene<T, N, V> &scene) {
    pbf_params p{};
    p.dt = double(c.dt), p.scale = double(c.scale), p.iteration = c.iteration;
    p.constant_force[0] = c.constantForce.x, p.constant_force[1] = c.constantForce.y,
    p.constant_force[2] = c.constantForce.z;
    p.min_bound[0] = c.minBound.x, p.min_bound[1] = c.minBound.y, p.min_bound[2] = c.minBound.z;
    p.max_bound[0] = c.maxBound.x, p.max_bound[1] = c.maxBound.y, p.max_bound[2] = c.maxBound.z;
    wells_.clear();
    for (const auto &w : scene.wells) {
      wells_.push_back(w.centre.x), wells_.push_back(w.centre.y), wells_.push_back(w.centre.z);
      wells_.push_back(double(w.force));
    }
    p.n_wells = int32_t(scene.wells.size());
    p.wells = wells_.empty() ? nullptr : wells_.data();
    return p;
  }

  // Solver::sample / sampleLattice: the output arrays sized for n points and handed to the C ABI; then the stated division
  static pbf_sample_out sampleArrays(Samples<N> &o, size_t n, uint32_t what) {
    o.rho.assign(n, N(0)), o.weight.assign(n, N(0)), o.count.assign(2 * n, 0u), o.outside.assign(n, uint8_t(0));
    if (what & PBF_SAMPLE_VELOCITY) o.mv.assign(3 * n, N(0));
    if (what & PBF_SAMPLE_COLOUR) o.mc.assign(4 * n, N(0));
    return {o.rho.data(), o.weight.data(), o.mv.empty() ? nullptr : o.mv.data(), o.mc.empty() ? nullptr : o.mc.data(),
            o.count.data(), o.outside.data()};
  }
  static void normalise(Samples<N> &o, uint32_t what) {
    const size_t n = o.weight.size();
    if (what & PBF_SAMPLE_VELOCITY) o.velocity.assign(3 * n, N(0));
    if (what & PBF_SAMPLE_COLOUR) o.colour.assign(4 * n, N(0));
    for (size_t i = 0; i < n; ++i) {
      if (o.weight[i] == N(0)) continue;
      for (size_t a = 0; a < 3 && !o.velocity.empty(); ++a) o.velocity[3 * i + a] = o.mv[3 * i + a] / o.weight[i];
      for (size_t a = 0; a < 4 && !o.colour.empty(); ++a) o.colour[4 * i + a] = o.mc[4 * i + a] / o.weight[i];
    }
  }

  // The collider and the scenery are given and built from a mesh alike: the lattice and the mesh as the C ABI takes them, and
  // the two setters behind setCollider / setScenery and setColliderMesh / setSceneryMesh (`set`, `who`: the entry point;
  // `single`: what is refused across several devices)
  static pbf_collider_sdf latticeOf(const std::array<uint32_t, 3> &dims, const std::array<double, 3> &origin, double spacing, double margin,
                                    const void *phi) {
    pbf_collider_sdf sdf{};
    for (int a = 0; a < 3; ++a) sdf.dims[a] = dims[a], sdf.origin[a] = origin[a];
    sdf.spacing = spacing, sdf.margin = margin, sdf.phi = phi;
    return sdf;
  }
  static pbf_mesh meshOf(const std::vector<double> &vertices, const std::vector<uint32_t> &triangles) {
    pbf_mesh mesh{};
    mesh.n_vertices = vertices.size() / 3, mesh.n_triangles = triangles.size() / 3;
    mesh.vertices = vertices.data(), mesh.triangles = triangles.data();
    return mesh;
  }
  Solver &setSolid(int (*set)(pbf_ctx *, const pbf_collider_sdf *), const char *who, const char *single, const pbf_collider_sdf &sdf) {
    if (multi()) throw std::runtime_error(single);
    check(set(ctx_, &sdf), who);
    return *this;
  }
  Solver &setSolidMesh(int (*set)(pbf_ctx *, const pbf_mesh *, const pbf_collider_sdf *, uint32_t, pbf_mesh_sdf_stats *), const char *who,
                       const char *single, const pbf_mesh &mesh, const pbf_collider_sdf &sdf, bool negate, pbf_mesh_sdf_stats *stats,
                       bool winding) {
    if (multi()) throw std::runtime_error(single);
    const uint32_t flags = (negate ? uint32_t(PBF_MESH_NEGATE) : 0u) | (winding ? uint32_t(PBF_MESH_SIGN_WINDING) : 0u);
    check(set(ctx_, &mesh, &sdf, flags, stats), who);
    return *this;
  }

public:
  explicit Solver(N h, int device = 0, uint32_t flags = 0) : h_(h) {
    pbf_desc d{};
    d.abi_version = PBF_ABI_VERSION;
    d.fp64 = std::is_same_v<N, double> ? 1 : 0;
    d.device = device;
    d.flags = flags;
    d.h = double(h);
    d.stream = nullptr;
    const int rc = pbf_create(&d, &ctx_);
    if (rc != PBF_OK) throw std::runtime_error(std::string("pbf_create: ") + pbf_last_error(nullptr));
  }
  // Several GPUs of one node: x-slabs, one ctx per entry of `devices` (an entry may repeat: see the file header).
  Solver(N h, std::vector<int> devices, uint32_t flags = 0) : h_(h), devices_(std::move(devices)), flags_(flags) {
    if (devices_.empty()) devices_.push_back(0);
    for (int dev : devices_) {
      pbf_desc d{};
      d.abi_version = PBF_ABI_VERSION;
      d.fp64 = std::is_same_v<N, double> ? 1 : 0;
      d.device = dev, d.flags = flags, d.h = double(h), d.stream = nullptr;
      pbf_ctx *c = nullptr;
      if (pbf_create(&d, &c) != PBF_OK) {
        const std::string msg = pbf_last_error(nullptr);
        for (auto *s : slabs_) pbf_destroy(s);
        throw std::runtime_error("pbf_create: " + msg);
      }
      slabs_.push_back(c);
    }
    ctx_ = slabs_[0];
    if (!multi()) return;
    const int n = int(slabs_.size());
    comms_.assign(n, nullptr);
    const bool distinct = std::set<int>(devices_.begin(), devices_.end()).size() == devices_.size();
    if (distinct) {  // RCCL over xGMI: ncclCommInitRank must be entered by all ranks concurrently
      unsigned char id[PBF_COMM_ID_BYTES];
      if (pbf_comm_unique_id(id) != PBF_OK) throw std::runtime_error(std::string("pbf_comm_unique_id: ") + pbf_comm_last_error(nullptr));
      parallel([&](size_t g) {
        if (pbf_comm_create_rccl(id, n, int(g), devices_[g], &comms_[g]) != PBF_OK)
          throw std::runtime_error(std::string("pbf_comm_create_rccl: ") + pbf_comm_last_error(nullptr));
      });
    } else {  // slabs sharing a GPU: in-process mailboxes behind the library's host-callback transport
      for (int k = 0; k < 2 * (n - 1); ++k) boxes_.emplace_back(new detail::Mailbox());
      links_.resize(n);
      for (int g = 0; g < n; ++g) {
        if (g > 0) links_[g].toLeft = boxes_[2 * (g - 1) + 1].get(), links_[g].fromLeft = boxes_[2 * (g - 1)].get();
        if (g + 1 < n) links_[g].toRight = boxes_[2 * g].get(), links_[g].fromRight = boxes_[2 * g + 1].get();
      }
      for (int g = 0; g < n; ++g)
        if (pbf_comm_create_host_callback(&detail::InProcessLink::exchange, &links_[g], n, g, &comms_[g]) != PBF_OK)
          throw std::runtime_error("pbf_comm_create_host_callback failed");
    }
  }
  ~Solver() override {
    if (phase_.on && phase_.frames)
      std::fprintf(stderr, "advance() phases, mean ms over %llu frames: upload %.3f | step %.3f | surface kernels + mesh DMA %.3f | "
                           "particle download %.3f | mesh vectors (rest) %.3f\n", (unsigned long long)phase_.frames,
                   phase_.ms[0] / phase_.frames, phase_.ms[1] / phase_.frames, phase_.ms[2] / phase_.frames,
                   phase_.ms[3] / phase_.frames, phase_.ms[4] / phase_.frames);
    workers_.shutdown();
    if (slabs_.empty()) pbf_destroy(ctx_);
    for (auto *s : slabs_) pbf_destroy(s);
    for (auto *c : comms_) pbf_comm_destroy(c);
  }
  size_t deviceCount() const { return slabs_.empty() ? 1 : slabs_.size(); }
  const std::vector<uint32_t> &cuts() const { return cuts_; }
  void setRebalanceEvery(unsigned steps) { rebalanceEvery_ = steps; }
  Solver(const Solver &) = delete;
  Solver &operator=(const Solver &) = delete;

  pbf_ctx *context() { return ctx_; }

  // Opt-in surface tension (cohesion) and adhesion to obstacles after Akinci et al. 2013 (pbf_set_surface_tension; no
  // reference counterpart): persists for every later step, 0 / 0 = off.  A single-device feature (not in slab mode).
  Solver &surfaceTension(N cohesion, N adhesion = 0) {
    if (multi()) throw std::runtime_error("surface tension is a single-device feature");
    check(pbf_set_surface_tension(ctx_, double(cohesion), double(adhesion)), "pbf_set_surface_tension");
    return *this;
  }

  // Opt-in static collider (pbf_set_collider; no reference counterpart): a signed-distance lattice — phi[(i * dims[1] + j) *
  // dims[2] + k] at origin + (i, j, k) * spacing, world units, negative inside the solid — that delta-p keeps the fluid out
  // of, at phi >= margin.  Copied to the device; persists for every later step and advance() until clearCollider().  A
  // single-device feature (not in slab mode).
  Solver &setCollider(const std::array<uint32_t, 3> &dims, const std::array<double, 3> &origin, double spacing, double margin,
                      const N *phi) {
    return setSolid(pbf_set_collider, "pbf_set_collider", "a collider is a single-device feature", latticeOf(dims, origin, spacing, margin, phi));
  }
  // The same collider from a closed triangle mesh (pbf_set_collider_mesh; no reference counterpart): vertices = 3 doubles per
  // vertex in world units, triangles = 3 indices per triangle, counter-clockwise seen from outside.  The lattice of `dims`
  // nodes at origin + (i, j, k) * spacing is filled with the signed distance on the device (negative inside the mesh; negate:
  // the solid is OUTSIDE, a cavity the fluid lives in) and installed.  winding: the mesh is a triangle soup signed by the
  // winding number (PBF_MESH_SIGN_WINDING) — open, misoriented and non-manifold meshes are accepted.  A single-device
  // feature, like setCollider.
  Solver &setColliderMesh(const std::vector<double> &vertices, const std::vector<uint32_t> &triangles, const std::array<uint32_t, 3> &dims,
                          const std::array<double, 3> &origin, double spacing, double margin, bool negate = false,
                          pbf_mesh_sdf_stats *stats = nullptr, bool winding = false) {
    return setSolidMesh(pbf_set_collider_mesh, "pbf_set_collider_mesh", "a collider is a single-device feature", meshOf(vertices, triangles),
                        latticeOf(dims, origin, spacing, margin, nullptr), negate, stats, winding);
  }
  // The winding-number field of a triangle soup on that lattice (pbf_mesh_winding): 1 inside a closed outward mesh, 0
  // outside, the covered share of the sphere of directions for an open one; node (i, j, k) at (i * dims[1] + j) * dims[2] + k.
  std::vector<N> meshWinding(const std::vector<double> &vertices, const std::vector<uint32_t> &triangles, const std::array<uint32_t, 3> &dims,
                             const std::array<double, 3> &origin, double spacing) {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    const pbf_mesh mesh = meshOf(vertices, triangles);
    const pbf_collider_sdf sdf = latticeOf(dims, origin, spacing, 0.0, nullptr);
    std::vector<N> w(size_t(dims[0]) * dims[1] * dims[2]);
    check(pbf_mesh_winding(ctx_, &mesh, &sdf, w.data()), "pbf_mesh_winding");
    return w;
  }
  Solver &clearCollider() {
    if (!multi()) check(pbf_set_collider(ctx_, nullptr), "pbf_set_collider");
    return *this;
  }
  // Scenery (pbf_set_scenery; no reference counterpart): a second, STATIC lattice in the world frame beside the collider, given
  // as setCollider's is.  It never has a pose, a body, friction or a reaction; delta-p projects the fluid out of it after the
  // collider, and with both installed the reaction records are on.  Persists until clearScenery(); installing or clearing the
  // collider leaves it alone.  A single-device feature, like setCollider.
  Solver &setScenery(const std::array<uint32_t, 3> &dims, const std::array<double, 3> &origin, double spacing, double margin,
                     const N *phi) {
    return setSolid(pbf_set_scenery, "pbf_set_scenery", "scenery is a single-device feature", latticeOf(dims, origin, spacing, margin, phi));
  }
  // setColliderMesh's build, installed as the scenery (pbf_set_scenery_mesh)
  Solver &setSceneryMesh(const std::vector<double> &vertices, const std::vector<uint32_t> &triangles, const std::array<uint32_t, 3> &dims,
                         const std::array<double, 3> &origin, double spacing, double margin, bool negate = false,
                         pbf_mesh_sdf_stats *stats = nullptr, bool winding = false) {
    return setSolidMesh(pbf_set_scenery_mesh, "pbf_set_scenery_mesh", "scenery is a single-device feature", meshOf(vertices, triangles),
                        latticeOf(dims, origin, spacing, margin, nullptr), negate, stats, winding);
  }
  Solver &clearScenery() {
    if (!multi()) check(pbf_set_scenery(ctx_, nullptr), "pbf_set_scenery");
    return *this;
  }
  // The static device function on the scenery's lattice at world points (pbf_scenery_sample; it synchronises): points = 3
  // doubles per point; phi, moved (3 per point, solver frame) and hit are resized to the point count.
  // The scale and the box are config's.
  void sampleScenery(const sph::SphParams<T, N, V> &config, const std::vector<double> &points, std::vector<N> &phi, std::vector<N> &moved,
                     std::vector<uint8_t> &hit) {
    if (multi()) throw std::runtime_error("scenery is a single-device feature");
    const size_t n = points.size() / 3;
    phi.resize(n), moved.resize(3 * n), hit.resize(n);
    const pbf_params p = params(config, sph::Scene<T, N, V>{});
    check(pbf_scenery_sample(ctx_, &p, n, points.data(), phi.data(), moved.data(), hit.data()), "pbf_scenery_sample");
  }
  // Moving colliders (pbf_set_collider_pose; no reference counterpart): the installed lattice is read in a body frame, a world
  // point being w = rot b + trans (rot row-major, body -> world).  No upload, no synchronisation and no recapture per call;
  // persists until it is changed, clearColliderPose() or a new collider.  A single-device feature, like setCollider.
  Solver &setColliderPose(const std::array<double, 9> &rot, const std::array<double, 3> &trans) {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    pbf_collider_pose pose{};
    for (size_t k = 0; k < 9; ++k) pose.rot[k] = rot[k];
    for (size_t k = 0; k < 3; ++k) pose.trans[k] = trans[k];
    check(pbf_set_collider_pose(ctx_, &pose), "pbf_set_collider_pose");
    return *this;
  }
  Solver &clearColliderPose() {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    check(pbf_set_collider_pose(ctx_, nullptr), "pbf_set_collider_pose");
    return *this;
  }
  // The reaction (pbf_set_collider_reaction / pbf_collider_reaction): what the collider gave the fluid in the last step, raw
  // sums — the body received the negatives.
  Solver &enableColliderReaction(bool on = true) {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    check(pbf_set_collider_reaction(ctx_, on ? 1 : 0), "pbf_set_collider_reaction");
    return *this;
  }
  pbf_collider_wrench colliderReaction() {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    pbf_collider_wrench w{};
    check(pbf_collider_reaction(ctx_, &w), "pbf_collider_reaction");
    return w;
  }
  // Floating bodies (pbf_set_collider_body): the installed collider as a rigid body the fluid moves — every later step sums the
  // reaction, advances the body and writes the next step's pose on the device, pbf_steps and graph replays included.  body.pose
  // is the start pose (trans = the centre of mass).  Calling it again re-places the body without a recapture;
  // clearColliderBody() leaves the solid where it is, as an ordinary pose.  colliderBody() synchronises.
  Solver &setColliderBody(const pbf_collider_body &body) {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    check(pbf_set_collider_body(ctx_, &body), "pbf_set_collider_body");
    return *this;
  }
  Solver &clearColliderBody() {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    check(pbf_set_collider_body(ctx_, nullptr), "pbf_set_collider_body");
    return *this;
  }
  struct pbf_collider_body_state colliderBody() {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    struct pbf_collider_body_state st {};
    check(pbf_collider_body_state(ctx_, &st), "pbf_collider_body_state");
    return st;
  }
  // Body contact (pbf_set_collider_body_contact): the body collides with the scenery — its surface, phi == level of the
  // collider's lattice sampled every `stride` cells, is tested against the scenery after every advance and answered with one
  // impulse and a shift of the centre on the device, pbf_steps and graph replays included.  Needs a body and scenery.  Calling
  // it again with the same level and stride rewrites the record without a recapture.  colliderBodyContact() synchronises;
  // colliderBodyContactPoints() returns the surface points, 3 values of N each, in the body frame.
  Solver &setColliderBodyContact(const pbf_body_contact &contact) {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    check(pbf_set_collider_body_contact(ctx_, &contact), "pbf_set_collider_body_contact");
    return *this;
  }
  Solver &clearColliderBodyContact() {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    check(pbf_set_collider_body_contact(ctx_, nullptr), "pbf_set_collider_body_contact");
    return *this;
  }
  struct pbf_body_contact_state colliderBodyContact() {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    struct pbf_body_contact_state st {};
    check(pbf_collider_body_contact_state(ctx_, &st), "pbf_collider_body_contact_state");
    return st;
  }
  std::vector<N> colliderBodyContactPoints() {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    uint64_t n = 0;
    check(pbf_collider_body_contact_points(ctx_, &n, nullptr), "pbf_collider_body_contact_points");
    std::vector<N> points(size_t(n) * 3);
    check(pbf_collider_body_contact_points(ctx_, &n, points.data()), "pbf_collider_body_contact_points");
    return points;
  }
  // Collider friction (pbf_set_collider_friction): Coulomb drag against the installed collider, relative to the solid's contact
  // velocity (velocity + angular_velocity x (x - the pose's t); a body's own while a body is on), one pass after every finalise,
  // pbf_steps and graph replays included.  mu = +inf is no-slip.  Calling it again rewrites the record without a recapture.
  // colliderFrictionReaction() synchronises: the last pass's raw sums; the solid received -impulse and -angular.
  Solver &setColliderFriction(double mu, const std::array<double, 3> &velocity = {0, 0, 0}, const std::array<double, 3> &angular_velocity = {0, 0, 0}) {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    pbf_collider_friction f{};
    f.mu = mu;
    for (size_t k = 0; k < 3; ++k) f.velocity[k] = velocity[k], f.angular_velocity[k] = angular_velocity[k];
    check(pbf_set_collider_friction(ctx_, &f), "pbf_set_collider_friction");
    return *this;
  }
  Solver &clearColliderFriction() {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    check(pbf_set_collider_friction(ctx_, nullptr), "pbf_set_collider_friction");
    return *this;
  }
  pbf_collider_wrench colliderFrictionReaction() {
    if (multi()) throw std::runtime_error("a collider is a single-device feature");
    pbf_collider_wrench w{};
    check(pbf_collider_friction_reaction(ctx_, &w), "pbf_collider_friction_reaction");
    return w;
  }

  // ---- device-resident path -------------------------------------------------------------------
  // Several devices: `config` places the cuts (its bounds and scale define the grid columns); the slabs start with
  // equal particle counts.
  void upload(const std::vector<sph::Particle<T, N, V>> &xs, const sph::SphParams<T, N, V> *config = nullptr) {
    const auto l = layout();
    if (!multi()) {
      check(pbf_upload_aos(ctx_, xs.size(), xs.data(), &l), "pbf_upload_aos");
      return;
    }
    if (!config) throw std::runtime_error("upload() on several devices needs the SphParams (grid columns for the cuts)");
    const int n = int(slabs_.size());
    std::vector<uint32_t> col(xs.size());
    for (size_t i = 0; i < xs.size(); ++i) col[i] = std::min<uint32_t>(columnOf(*config, xs[i].position.x), 1023u);
    if (!attached_) {  // first upload: cuts at the particle-count quantiles of the columns
      std::vector<uint32_t> sorted(col);
      std::sort(sorted.begin(), sorted.end());
      cuts_.assign(n + 1, 0);
      for (int g = 1; g < n; ++g) cuts_[g] = sorted.empty() ? uint32_t(g) : sorted[std::min(sorted.size() - 1, sorted.size() * g / n)];
      cuts_[n] = 1024;
      for (int g = 1; g <= n; ++g) cuts_[g] = std::max(cuts_[g], cuts_[g - 1] + 1);
    }
    std::vector<std::vector<sph::Particle<T, N, V>>> part(n);
    for (size_t i = 0; i < xs.size(); ++i) {
      const int g = int(std::upper_bound(cuts_.begin() + 1, cuts_.end() - 1, col[i]) - (cuts_.begin() + 1));
      part[g].push_back(xs[i]);
    }
    const size_t per = std::max<size_t>(xs.size() / n, 1);
    // records in the first message of the two assembly rounds (the remainder follows when needed)
    const uint32_t capGhost = uint32_t(std::max<size_t>(per / 8, 1u << 14)), capMig = uint32_t(std::max<size_t>(per / 64, 1u << 12));
    for (int g = 0; g < n; ++g) {
      if (!attached_) checkOn(g, pbf_reserve(slabs_[g], 3 * per + (1u << 16)), "pbf_reserve");
      checkOn(g, pbf_upload_aos(slabs_[g], part[g].size(), part[g].data(), &l), "pbf_upload_aos");
      if (!attached_) checkOn(g, pbf_slab_attach(slabs_[g], comms_[g], cuts_.data(), capMig, capGhost), "pbf_slab_attach");
    }
    attached_ = true;
  }
  // The whole Scene rides along: wells in the params, sources and drains pushed to the context when they differ from what
  // it last got (emitted / drained on the device at the top of each of the `count` steps, as `count` advance() calls would).
  void step(const sph::SphParams<T, N, V> &config, const sph::Scene<T, N, V> &scene = {}, uint32_t count = 1) {
    const pbf_params p = params(config, scene);
    if (!multi()) {
      pushScene(scene);
      check(pbf_steps(ctx_, &p, count), "pbf_steps");
      return;
    }
    if (!scene.sources.empty() || !scene.drains.empty()) throw std::runtime_error("sources and drains are a single-device feature");
    if (!attached_) throw std::runtime_error("step() before upload()");
    for (uint32_t k = 0; k < count; ++k) {
      if (rebalanceEvery_ && frame_ && frame_ % rebalanceEvery_ == 0) rebalance();
      ++frame_;
      parallel([&](size_t g) { checkOn(g, pbf_slab_step(slabs_[g], &p), "pbf_slab_step"); });
    }
  }
  // Load balance: all-device column histogram -> new cuts (detail::recut) -> every ctx.
  bool rebalance() {
    std::vector<uint64_t> hist(1024, 0);
    for (size_t g = 0; g < slabs_.size(); ++g) {
      uint32_t h[1024];
      checkOn(g, pbf_slab_column_histogram(slabs_[g], h), "pbf_slab_column_histogram");
      for (int c = 0; c < 1024; ++c) hist[c] += h[c];
    }
    const auto nw = detail::recut(cuts_, hist);
    if (nw == cuts_) return false;
    cuts_ = nw;
    for (size_t g = 0; g < slabs_.size(); ++g) checkOn(g, pbf_slab_set_cuts(slabs_[g], cuts_.data()), "pbf_slab_set_cuts");
    return true;
  }
  // Particle capacity for what sources will emit on the resident path; before upload().
  void reserve(size_t capacity) {
    if (multi()) throw std::runtime_error("reserve() is a single-device call (upload() sizes the slabs itself)");
    check(pbf_reserve(ctx_, capacity), "pbf_reserve");
  }
  void sync() {
    if (!multi()) check(pbf_sync(ctx_), "pbf_sync");
    else
      for (size_t g = 0; g < slabs_.size(); ++g) checkOn(g, pbf_sync(slabs_[g]), "pbf_sync");
  }
  size_t count() const {
    if (!multi()) return pbf_count(ctx_);
    size_t n = 0;
    for (auto *s : slabs_) n += pbf_owned_count(s);
    return n;
  }
  // Several devices: slab after slab (each slab in its own Z-order).
  void download(std::vector<sph::Particle<T, N, V>> &xs) {
    const auto l = layout();
    if (!multi()) {
      xs.resize(pbf_count(ctx_));
      check(pbf_download_aos(ctx_, xs.data(), &l), "pbf_download_aos");
      return;
    }
    xs.resize(count());
    size_t at = 0;
    for (size_t g = 0; g < slabs_.size(); ++g) {
      checkOn(g, pbf_download_aos(slabs_[g], xs.data() + at, &l), "pbf_download_aos");
      at += pbf_owned_count(slabs_[g]);
    }
  }

  // ---- the reference's contract ---------------------------------------------------------------
  sph::Result<T, N, V> advance(const sph::SphParams<T, N, V> &config, const sph::Scene<T, N, V> &scene,
                               std::vector<sph::Particle<T, N, V>> &xs) final {
    // sources: a floor(sqrt(rate)) x ceil(sqrt(rate)) sheet at spacing h*scale/2 (ompsph.hpp:93-105)
    const N spacing = h_ * config.scale / 2;
    for (const auto &src : scene.sources) {
      const N size = std::sqrt(N(src.rate));
      const size_t width = size_t(std::floor(size)), depth = size_t(std::ceil(size));
      const V<3> corner = src.centre - (V<3>(width, 0, depth) * N(0.5)) * spacing;
      for (size_t x = 0; x < width; ++x)
        for (size_t z = 0; z < depth; ++z)
          xs.emplace_back(src.tag, sph::Type::Fluid, N(1), src.colour, corner + V<3>(x, 0, z) * spacing, src.velocity);
    }
    // drains: fluid within `width` of a drain centre disappears (ompsph.hpp:107-118)
    if (!scene.drains.empty())
      xs.erase(std::remove_if(xs.begin(), xs.end(),
                              [&](const sph::Particle<T, N, V> &p) {
                                if (p.type == sph::Type::Obstacle) return false;
                                for (const auto &d : scene.drains) {
                                  const V<3> r = p.position - d.centre;
                                  if (std::sqrt(r.x * r.x + r.y * r.y + r.z * r.z) < d.width) return true;
                                }
                                return false;
                              }),
               xs.end());
    if (xs.empty()) {  // ompsph.hpp:122-126
      std::cout << "Particles depleted" << std::endl;
      std::this_thread::sleep_for(std::chrono::milliseconds(5));
      return {};
    }
    // (sources and drains were applied above, on the host: the device step gets the wells alone)
    sph::Scene<T, N, V> wellsOnly;
    wellsOnly.wells = scene.wells;
    if (multi()) {
      if (!scene.queries.empty()) throw std::runtime_error("queries are a single-device feature");
      upload(xs, &config);
      step(config, wellsOnly, 1);
      sph::Result<T, N, V> result;
      if (config.surface) result.mesh = surface(config, scene);  // every slab its part of the lattice, concatenated
      download(xs);
      return result;
    }
    PhaseClock clk(phase_);
    upload(xs);
    clk.lap(0);
    step(config, wellsOnly, 1);
    if (whitewaterOn_) whitewaterStep(config);  // (reads the state only: before the download sets off)
    if (phase_.on) sync();
    clk.lap(1);
    sph::Result<T, N, V> result;
    if (!scene.queries.empty()) result.queries = queryHost(config, scene);
    if (config.surface && indexedFrames_) {  // the same order of events as below, with the indexed mesh
      const auto l = layout();
      xs.resize(pbf_count(ctx_));
      check(pbf_download_aos_begin(ctx_, xs.data(), &l), "pbf_download_aos_begin");
      IndexedCopy copy(*this, config, scene, lastIndexed_);
      clk.lap(2);
      check(pbf_download_aos_end(ctx_), "pbf_download_aos_end");
      clk.lap(3);
      copy.join();
      clk.lap(4);
    } else if (config.surface) {  // ompsph.hpp:277-477
      // the mesh lands in page-locked staging (one DMA); its three vectors are then built on host threads WHILE the
      // particles travel back over PCIe
      // — and the particles set off BEFORE the surface kernels start (pbf_download_aos_begin: their DMA runs on a copy
      // stream while the field / count / emit kernels, which only read the state, execute)
      static const bool early = std::getenv("PBF_SHIM_LATE_DOWNLOAD") == nullptr;  // (A/B switch: the round-2 order)
      const auto l = layout();
      xs.resize(pbf_count(ctx_));
      if (early) check(pbf_download_aos_begin(ctx_, xs.data(), &l), "pbf_download_aos_begin");
      MeshCopy copy(*this, config, scene, result.mesh);
      clk.lap(2);
      if (early) check(pbf_download_aos_end(ctx_), "pbf_download_aos_end");
      else check(pbf_download_aos(ctx_, xs.data(), &l), "pbf_download_aos");
      clk.lap(3);
      copy.join();
      clk.lap(4);
    } else {
      download(xs);
      clk.lap(3);
    }
    return result;
  }

  // Marching-cubes surface of the state the last step left (reference: config.surface, ompsph.hpp:277-477).
  // Several devices: every slab extracts the cubes of its own node planes (pbf_surface is collective there: the slabs
  // refresh their copies' colours and hand one node plane to the left), the parts are concatenated in slab order — the
  // single-device mesh's cube order.
  sph::ColouredMesh<N, V> surface(const sph::SphParams<T, N, V> &config, const sph::Scene<T, N, V> &scene = {}) {
    sph::ColouredMesh<N, V> mesh;
    if (!multi()) {
      MeshCopy(*this, config, scene, mesh).join();
      return mesh;
    }
    const pbf_params p = params(config, scene);
    const pbf_mc_params mc{double(config.surface->resolution), double(config.surface->isolevel),
                           double(config.surface->particleSize), double(config.surface->particleInfluence)};
    std::vector<uint64_t> tri(slabs_.size(), 0);
    parallel([&](size_t g) { checkOn(g, pbf_surface(slabs_[g], &p, &mc, &tri[g]), "pbf_surface"); });
    size_t total = 0;
    for (uint64_t t : tri) total += size_t(t) * 3;
    mesh.vs.reserve(total), mesh.ns.reserve(total), mesh.cs.reserve(total);
    for (size_t g = 0; g < slabs_.size(); ++g) {
      const void *pv = nullptr, *pn = nullptr, *pc = nullptr;
      checkOn(g, pbf_map_mesh(slabs_[g], &pv, &pn, &pc), "pbf_map_mesh");
      const size_t nv = size_t(tri[g]) * 3;
      if (!nv) continue;
      const V<3> *v3 = static_cast<const V<3> *>(pv), *n3 = static_cast<const V<3> *>(pn);
      const V<4> *c4 = static_cast<const V<4> *>(pc);
      mesh.vs.insert(mesh.vs.end(), v3, v3 + nv), mesh.ns.insert(mesh.ns.end(), n3, n3 + nv);
      mesh.cs.insert(mesh.cs.end(), c4, c4 + nv);
    }
    return mesh;
  }

  // Conserved sums, extrema and — `density` — the density residual of the resident state, computed and reduced on the device
  // (pbf_diagnostics; the fields are pbf_diag's, include/pbf_hip.h).  The density part needs a step() first and the config
  // of that step.  Single device: on several the library's own refusal is thrown.
  Diagnostics diagnostics(const sph::SphParams<T, N, V> &config, bool density = false) {
    const pbf_params p = params(config, sph::Scene<T, N, V>{});
    pbf_diag d{};
    check(pbf_diagnostics(ctx_, &p, density ? uint32_t(PBF_DIAG_DENSITY) : 0u, &d), "pbf_diagnostics");
    Diagnostics o;
    o.fluid = d.n_fluid, o.obstacles = d.n_obstacle, o.nonFinite = d.n_nonfinite;
    o.mass = d.mass, o.kinetic = d.kinetic, o.maxSpeed = d.max_speed;
    for (int k = 0; k < 3; ++k)
      o.moment[k] = d.moment[k], o.momentum[k] = d.momentum[k], o.aabbMin[k] = d.aabb_min[k], o.aabbMax[k] = d.aabb_max[k];
    o.densityParticles = d.n_density, o.nbrMax = d.nbr_max;
    o.rhoMin = d.rho_min, o.rhoMax = d.rho_max, o.rhoMean = d.rho_mean;
    o.errMean = d.err_mean, o.errMax = d.err_max, o.compressionMean = d.compression_mean, o.nbrMean = d.nbr_mean;
    return o;
  }

  // The SPH sums at world points / on the lattice origin + (i, j, k) * spacing (pbf_sample_points / pbf_sample_lattice,
  // include/pbf_hip.h): `what` = PBF_SAMPLE_VELOCITY | PBF_SAMPLE_COLOUR.  Needs a step() first and the config of that step.
  // No numerics here beyond the stated division.  Single device: on several the library's own refusal is thrown.
  Samples<N> sample(const sph::SphParams<T, N, V> &config, const std::vector<V<3>> &points, uint32_t what = 0) {
    std::vector<double> pts(3 * points.size());
    for (size_t i = 0; i < points.size(); ++i) pts[3 * i] = points[i].x, pts[3 * i + 1] = points[i].y, pts[3 * i + 2] = points[i].z;
    const pbf_params p = params(config, sph::Scene<T, N, V>{});
    Samples<N> o;
    const pbf_sample_out out = sampleArrays(o, points.size(), what);
    check(pbf_sample_points(ctx_, &p, points.size(), pts.data(), what, &out), "pbf_sample_points");
    normalise(o, what);
    return o;
  }
  Samples<N> sampleLattice(const sph::SphParams<T, N, V> &config, const V<3> &origin, const V<3> &spacing,
                           const std::array<uint64_t, 3> &dims, uint32_t what = 0) {
    const double o3[3] = {double(origin.x), double(origin.y), double(origin.z)};
    const double s3[3] = {double(spacing.x), double(spacing.y), double(spacing.z)};
    const uint64_t n = dims[0] * dims[1] * dims[2];
    const pbf_params p = params(config, sph::Scene<T, N, V>{});
    Samples<N> o;
    const pbf_sample_out out = sampleArrays(o, n < (uint64_t(1) << 31) ? size_t(n) : 0, what);
    check(pbf_sample_lattice(ctx_, &p, o3, s3, dims.data(), what, &out), "pbf_sample_lattice");
    normalise(o, what);
    return o;
  }

  // Per-particle smoothed centres and anisotropy matrices after Yu & Turk 2013 (pbf_anisotropy_compute, include/pbf_hip.h; no
  // reference counterpart) on the state the last step() left; `config` and `scene` are that step's.  No numerics here.
  // Single device: on several the library's own refusal is thrown.
  Anisotropy<N> anisotropy(const sph::SphParams<T, N, V> &config, const sph::Scene<T, N, V> &scene, const pbf_anisotropy &cfg) {
    const pbf_params p = params(config, scene);
    const size_t n = pbf_count(ctx_);
    Anisotropy<N> o;
    o.centre.resize(3 * n), o.G.resize(6 * n), o.axes.resize(9 * n), o.radii.resize(3 * n), o.neighbours.resize(n);
    const pbf_anisotropy_out out{o.centre.data(), o.G.data(), o.axes.data(), o.radii.data(), o.neighbours.data()};
    check(pbf_anisotropy_compute(ctx_, &p, &cfg, &out), "pbf_anisotropy_compute");
    return o;
  }

  // Whitewater — spray, foam and air bubbles after Ihmsen et al. 2012 (pbf_whitewater_*, include/pbf_hip.h; no reference
  // counterpart): a pool of diffuse particles owned by the solver.  whitewater(config) configures it (capacity 0 frees it);
  // from then on advance() runs one whitewater step after each fluid step, and the resident path calls whitewaterStep()
  // after step().  Single device.
  Solver &whitewater(const pbf_whitewater &config) {
    if (multi()) throw std::runtime_error("whitewater is a single-device feature");
    check(pbf_whitewater_configure(ctx_, &config), "pbf_whitewater_configure");
    whitewaterOn_ = config.capacity != 0;
    whitewaterStats_ = pbf_whitewater_stats{};
    return *this;
  }
  // one whitewater step on the state the last step() left; `config` is that step's
  pbf_whitewater_stats whitewaterStep(const sph::SphParams<T, N, V> &config) {
    const pbf_params p = params(config, sph::Scene<T, N, V>{});
    check(pbf_whitewater_step(ctx_, &p, &whitewaterStats_), "pbf_whitewater_step");
    return whitewaterStats_;
  }
  const pbf_whitewater_stats &whitewaterStats() const { return whitewaterStats_; }  // the record of the last whitewater step
  // The diffuse particles collide with the collider and the scenery (pbf_set_whitewater_solids, include/pbf_hip.h): a wish
  // that needs no installed solid and outlives them all.  NULL turns it off.  whitewaterSolidsStats(): the counts of the last
  // whitewater step (synchronises).
  Solver &setWhitewaterSolids(const pbf_whitewater_solids *config) {
    if (multi()) throw std::runtime_error("whitewater is a single-device feature");
    check(pbf_set_whitewater_solids(ctx_, config), "pbf_set_whitewater_solids");
    return *this;
  }
  struct pbf_whitewater_solids_stats whitewaterSolidsStats() {
    struct pbf_whitewater_solids_stats s {};
    check(pbf_whitewater_solids_stats(ctx_, &s), "pbf_whitewater_solids_stats");
    return s;
  }
  WhitewaterParticles<N, V> whitewaterParticles() {
    WhitewaterParticles<N, V> o;
    const size_t n = pbf_whitewater_count(ctx_);
    o.positions.resize(n), o.velocities.resize(n), o.life.resize(n), o.kind.resize(n), o.parentId.resize(n);
    check(pbf_whitewater_download(ctx_, o.positions.data(), o.velocities.data(), o.life.data(), o.kind.data(), o.parentId.data()),
          "pbf_whitewater_download");
    return o;
  }
  // The potentials {I_ta, I_wc, E_k, n_d} of the last whitewater step, 4 values per particle in device order.
  std::vector<N> whitewaterPotentials() {
    std::vector<N> pot(4 * pbf_count(ctx_));
    check(pbf_read_buffer(ctx_, PBF_BUF_WHITEWATER, pot.data(), pot.size() * sizeof(N)), "pbf_read_buffer(whitewater)");
    return pot;
  }
  // tau ranges for a scene nobody has looked at yet: the 10 % and 90 % quantiles of the positive values of the potentials
  // the last whitewater step left (what tools/whitewater_probe.py prints), written into `config`
  void whitewaterQuantileTaus(pbf_whitewater &config) {
    const std::vector<N> pot = whitewaterPotentials();
    double *tau[3] = {config.tau_ta, config.tau_wc, config.tau_k};
    for (int c = 0; c < 3; ++c) {
      std::vector<double> v;
      for (size_t i = size_t(c); i < pot.size(); i += 4)
        if (pot[i] > N(0)) v.push_back(double(pot[i]));
      std::sort(v.begin(), v.end());
      tau[c][0] = v.empty() ? 0.0 : v[size_t(0.1 * double(v.size() - 1))];
      tau[c][1] = v.empty() ? 1.0 : v[size_t(0.9 * double(v.size() - 1))];
      if (!(tau[c][1] > tau[c][0])) tau[c][1] = tau[c][0] + 1.0;
    }
  }

  // The same surface as an indexed mesh: 40 V + 12 T bytes in fp32 instead of 120 T, watertight by index.  Single device (an
  // edge on a slab's cut plane belongs to a node of another device).
  IndexedMesh<N, V> surfaceIndexed(const sph::SphParams<T, N, V> &config, const sph::Scene<T, N, V> &scene = {}) {
    if (multi()) throw std::runtime_error("the indexed mesh is a single-device feature");
    IndexedMesh<N, V> mesh;
    IndexedCopy(*this, config, scene, mesh).join();
    return mesh;
  }
  // indexedMesh(true): advance() runs config.surface through the indexed path; Result::mesh stays empty and the frame's mesh
  // is lastIndexedMesh() until the next advance().  Off by default: advance() is the reference's.
  Solver &indexedMesh(bool on) {
    if (on && multi()) throw std::runtime_error("the indexed mesh is a single-device feature");
    indexedFrames_ = on;
    return *this;
  }
  const IndexedMesh<N, V> &lastIndexedMesh() const { return lastIndexed_; }

  // The iso-surface of Yu & Turk's anisotropic-kernel field over the ellipsoids of anisotropy() (pbf_surface_anisotropic,
  // include/pbf_hip.h; no reference counterpart) on the state the last step() left, as a soup or as an indexed mesh: the stock
  // count, scans and emission around another field.  config.surface is not read — the resolution and the isolevel (no
  // default: the field's scale is not the stock one's) are `cfg`'s.  Single device: on several the library's refusal is thrown.
  sph::ColouredMesh<N, V> surfaceAnisotropic(const sph::SphParams<T, N, V> &config, const AnisoSurface &cfg,
                                             const sph::Scene<T, N, V> &scene = {}) {
    sph::ColouredMesh<N, V> mesh;
    MeshCopy(*this, config, scene, mesh, &cfg).join();
    return mesh;
  }
  IndexedMesh<N, V> surfaceAnisotropicIndexed(const sph::SphParams<T, N, V> &config, const AnisoSurface &cfg,
                                              const sph::Scene<T, N, V> &scene = {}) {
    IndexedMesh<N, V> mesh;
    IndexedCopy(*this, config, scene, mesh, &cfg).join();
    return mesh;
  }

private:
  // pbf_surface_indexed + the hand-over, shaped like MeshCopy below: one DMA into the page-locked staging, four range
  // assignments on threads of their own once the mesh is large enough to pay for them
  struct IndexedCopy {
    IndexedMesh<N, V> &mesh;
    const V<3> *v3 = nullptr, *n3 = nullptr;
    const V<4> *c4 = nullptr;
    const uint32_t *t3 = nullptr;
    size_t nv = 0, ni = 0;
    std::thread th[4];
    IndexedCopy(Solver &s, const sph::SphParams<T, N, V> &config, const sph::Scene<T, N, V> &scene, IndexedMesh<N, V> &out,
                const AnisoSurface *aniso = nullptr)
        : mesh(out) {
      const pbf_params p = s.params(config, scene);
      uint64_t vertices = 0, triangles = 0;
      if (aniso) {
        s.check(pbf_surface_anisotropic(s.ctx_, &p, aniso, 1, &vertices, &triangles), "pbf_surface_anisotropic");
      } else {
        const pbf_mc_params mc{double(config.surface->resolution), double(config.surface->isolevel),
                               double(config.surface->particleSize), double(config.surface->particleInfluence)};
        s.check(pbf_surface_indexed(s.ctx_, &p, &mc, &vertices, &triangles), "pbf_surface_indexed");
      }
      const void *pv = nullptr, *pn = nullptr, *pc = nullptr;
      s.check(pbf_map_mesh_indexed(s.ctx_, &pv, &pn, &pc, &t3), "pbf_map_mesh_indexed");
      nv = size_t(vertices), ni = size_t(triangles) * 3;
      v3 = static_cast<const V<3> *>(pv), n3 = static_cast<const V<3> *>(pn), c4 = static_cast<const V<4> *>(pc);
      if (ni == 0) nv = 0;
      if (ni >= (size_t(1) << 16)) {
        th[0] = std::thread([this] { mesh.vs.assign(v3, v3 + nv); });
        th[1] = std::thread([this] { mesh.ns.assign(n3, n3 + nv); });
        th[2] = std::thread([this] { mesh.cs.assign(c4, c4 + nv); });
        th[3] = std::thread([this] { mesh.tris.assign(t3, t3 + ni); });
      }
    }
    void join() {
      if (th[0].joinable()) {
        for (auto &t : th) t.join();
      } else {
        mesh.vs.assign(v3, v3 + nv), mesh.ns.assign(n3, n3 + nv), mesh.cs.assign(c4, c4 + nv), mesh.tris.assign(t3, t3 + ni);
      }
    }
    ~IndexedCopy() {
      for (auto &t : th)
        if (t.joinable()) t.join();
    }
  };

  // pbf_surface + the mesh hand-over.  ColouredMesh(size) would zero-fill 54 MB (1 M particles) that a pageable
  // device-to-host copy then overwrites at a few GB/s: 11 ms per frame in round 2.  Instead: ONE DMA into the library's
  // page-locked staging (pbf_map_mesh), then the three vectors are range-assigned from it (no fill), each on a thread of its
  // own — so the caller can do something useful (the particle download) until join().
  struct MeshCopy {
    sph::ColouredMesh<N, V> &mesh;
    const V<3> *v3 = nullptr, *n3 = nullptr;
    const V<4> *c4 = nullptr;
    size_t nv = 0;
    std::thread tv, tn, tc;
    MeshCopy(Solver &s, const sph::SphParams<T, N, V> &config, const sph::Scene<T, N, V> &scene, sph::ColouredMesh<N, V> &out,
             const AnisoSurface *aniso = nullptr)
        : mesh(out) {
      const pbf_params p = s.params(config, scene);
      uint64_t triangles = 0;
      if (aniso) {
        s.check(pbf_surface_anisotropic(s.ctx_, &p, aniso, 0, nullptr, &triangles), "pbf_surface_anisotropic");
      } else {
        const pbf_mc_params mc{double(config.surface->resolution), double(config.surface->isolevel),
                               double(config.surface->particleSize), double(config.surface->particleInfluence)};
        s.check(pbf_surface(s.ctx_, &p, &mc, &triangles), "pbf_surface");
      }
      const void *pv = nullptr, *pn = nullptr, *pc = nullptr;
      s.check(pbf_map_mesh(s.ctx_, &pv, &pn, &pc), "pbf_map_mesh");
      nv = size_t(triangles) * 3;
      v3 = static_cast<const V<3> *>(pv), n3 = static_cast<const V<3> *>(pn), c4 = static_cast<const V<4> *>(pc);
      if (nv >= (size_t(1) << 16)) {  // (small meshes — the stock 18 K-particle run: a thread costs more than the copy)
        tv = std::thread([this] { mesh.vs.assign(v3, v3 + nv); });
        tn = std::thread([this] { mesh.ns.assign(n3, n3 + nv); });
        tc = std::thread([this] { mesh.cs.assign(c4, c4 + nv); });
      }
    }
    void join() {
      if (nv == 0) return;
      if (tv.joinable()) {
        tv.join(), tn.join(), tc.join();
      } else {
        mesh.vs.assign(v3, v3 + nv), mesh.ns.assign(n3, n3 + nv), mesh.cs.assign(c4, c4 + nv);
      }
      nv = 0;
    }
    ~MeshCopy() {
      if (tv.joinable()) tv.join();
      if (tn.joinable()) tn.join();
      if (tc.joinable()) tc.join();
    }
  };

public:
  // ids of the fluid particles in the cell that holds each query point (ompsph.hpp:167-186), answered on the device from
  // the keys and table of the last step (pbf_query_cells); the cells are those of the predicted positions, as in the
  // reference.  Single device.
  std::vector<sph::QueryResult<T, N, V>> query(const sph::SphParams<T, N, V> &config, const sph::Scene<T, N, V> &scene) {
    if (multi()) throw std::runtime_error("queries are a single-device feature");
    const size_t nq = scene.queries.size();
    std::vector<sph::QueryResult<T, N, V>> out(nq);
    if (!nq) return out;
    const pbf_params p = params(config, scene);
    std::vector<double> pts(3 * nq);
    for (size_t i = 0; i < nq; ++i)
      pts[3 * i] = scene.queries[i].point.x, pts[3 * i + 1] = scene.queries[i].point.y, pts[3 * i + 2] = scene.queries[i].point.z;
    std::vector<uint32_t> counts(nq);
    size_t cap = 64;  // (a cell of the rest state holds ~8 particles; a fuller one is asked for again with its own count)
    std::vector<uint64_t> ids(nq * cap);
    check(pbf_query_cells(ctx_, &p, nq, pts.data(), counts.data(), ids.data(), cap), "pbf_query_cells");
    const size_t most = *std::max_element(counts.begin(), counts.end());
    if (most > cap) {
      cap = most, ids.resize(nq * cap);
      check(pbf_query_cells(ctx_, &p, nq, pts.data(), counts.data(), ids.data(), cap), "pbf_query_cells");
    }
    for (size_t i = 0; i < nq; ++i) {
      const uint64_t *row = ids.data() + i * cap;
      out[i] = {scene.queries[i].id, scene.queries[i].point, std::vector<T>(row, row + counts[i])};
    }
    return out;
  }

private:
  void pushScene(const sph::Scene<T, N, V> &scene) {
    std::vector<pbf_source> src(scene.sources.size());
    for (size_t k = 0; k < src.size(); ++k) {
      const auto &q = scene.sources[k];
      src[k] = pbf_source{uint64_t(q.tag), {q.centre.x, q.centre.y, q.centre.z}, {q.velocity.x, q.velocity.y, q.velocity.z},
                          {q.colour.x, q.colour.y, q.colour.z, q.colour.w}, double(q.rate)};
    }
    std::vector<pbf_drain> drn(scene.drains.size());
    for (size_t k = 0; k < drn.size(); ++k) {
      const auto &q = scene.drains[k];
      drn[k] = pbf_drain{{q.centre.x, q.centre.y, q.centre.z}, double(q.width)};
    }
    auto same = [](const auto &a, const auto &b) {
      return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0);
    };
    if (!same(src, sources_)) {
      check(pbf_set_sources(ctx_, src.size(), src.data()), "pbf_set_sources");
      sources_.swap(src);
    }
    if (!same(drn, drains_)) {
      check(pbf_set_drains(ctx_, drn.size(), drn.data()), "pbf_set_drains");
      drains_.swap(drn);
    }
  }

  // advance()'s own query: downloads keys, ids and types and bisects them on the host
  std::vector<sph::QueryResult<T, N, V>> queryHost(const sph::SphParams<T, N, V> &config,
                                                   const sph::Scene<T, N, V> &scene) {
    const size_t n = pbf_count(ctx_);
    std::vector<uint32_t> keys(n);
    std::vector<uint64_t> ids(n);
    std::vector<uint8_t> types(n);
    check(pbf_read_buffer(ctx_, PBF_BUF_KEYS, keys.data(), n * 4), "pbf_read_buffer(keys)");
    check(pbf_download(ctx_, ids.data(), types.data(), nullptr, nullptr, nullptr, nullptr), "pbf_download(ids)");
    uint64_t extent[3];
    double minExtent[3];
    check(pbf_grid_extent(ctx_, extent, minExtent), "pbf_grid_extent");
    const size_t tableN = pbf_table_size(ctx_);
    auto spread = [](uint64_t v) {
      uint32_t x = uint32_t(v);
      x = (x | (x << 16)) & 0x030000FFu, x = (x | (x << 8)) & 0x0300F00Fu;
      x = (x | (x << 4)) & 0x030C30C3u, x = (x | (x << 2)) & 0x09249249u;
      return x;
    };
    std::vector<sph::QueryResult<T, N, V>> out(scene.queries.size());
    for (size_t i = 0; i < scene.queries.size(); ++i) {
      const auto &q = scene.queries[i];
      const N sx = q.point.x / config.scale - N(minExtent[0]), sy = q.point.y / config.scale - N(minExtent[1]),
              sz = q.point.z / config.scale - N(minExtent[2]);
      const uint32_t code = spread(uint64_t(int64_t(sx / h_))) | (spread(uint64_t(int64_t(sy / h_))) << 1) |
                            (spread(uint64_t(int64_t(sz / h_))) << 2);
      std::vector<T> found;
      if (size_t(code) + 1 < tableN) {
        auto lo = std::lower_bound(keys.begin(), keys.end(), code), hi = std::upper_bound(lo, keys.end(), code);
        for (auto it = lo; it != hi; ++it) {
          const size_t a = size_t(it - keys.begin());
          if (types[a] == uint8_t(sph::Type::Fluid)) found.push_back(T(ids[a]));
        }
      }
      out[i] = {q.id, q.point, found};
    }
    return out;
  }
};

}  // namespace sph::hip_impl
