// benchmark.cpp — drop-in benchmark driver for the MI355X backend.
//
// Observable behaviour follows the reference's src/benchmark.cpp: `warmup` untimed advance() calls,
// then `iter` timed ones, each with applyMotionSinXCosZ(param, frame) and an empty Scene
// (benchmark.cpp:22-58); then the summary block of benchmark.cpp:91-101 and "Results flushed.".
// Stock defaults: 20000 nominal particles (2 x 21^3 = 18522), 6 solver iterations, scale 500, h = 0.1
// (benchmark.cpp:23-25,160-163), marching-cubes surface on (benchmark.cpp:29; --no-surface turns it off).
// Differences, all visible in the output: the only backend is `hip`; extra lines report particle-steps/s;
// --resident times the device-resident loop; the surface's case tables are our own, so the vertex
// count need not equal the reference's triangle for triangle.
#include <hip/hip_runtime_api.h>
#include <malloc.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <filesystem>
#include <fstream>
#include <iomanip>
#include <numeric>

#include "args.hpp"
#include "hipsph.hpp"
#include "obj_mesh.hpp"

using duration_millis = std::chrono::duration<double, std::milli>;
using hrc = std::chrono::high_resolution_clock;

namespace {

struct Stats {
  double min, max, mean, stdDev;
};
Stats summaryStats(const std::vector<double> &xs) {
  const double sum = std::accumulate(xs.begin(), xs.end(), 0.0);
  const double mean = sum / double(xs.size());
  double var = 0;
  for (double x : xs) var += (x - mean) * (x - mean);
  var /= double(xs.size());
  const auto [mn, mx] = std::minmax_element(xs.begin(), xs.end());
  return {*mn, *mx, mean, std::sqrt(var)};
}

std::vector<std::pair<int, std::string>> listDevices() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  std::vector<std::pair<int, std::string>> out;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, i) == hipSuccess) out.emplace_back(i, std::string(p.name) + " (" + p.gcnArchName + ")");
  }
  return out;
}

// devices matching any needle: an index or a substring of the name (src/utils.hpp:87-105,128-159).  The reference
// takes the FIRST match; --all-devices takes every match (one x-slab each), --slabs K repeats the first K times.
std::vector<int> findDevices(const sph::driver::Args &args) {
  const auto devices = listDevices();
  std::vector<int> out;
  if (args.list) {
    for (const auto &[i, name] : devices) std::cout << "[" << i << "] " << name << std::endl;
    return out;
  }
  for (const auto &[i, name] : devices)
    for (const auto &needle : args.devices) {
      bool match = false;
      try {
        size_t pos = 0;
        const int idx = std::stoi(needle, &pos);
        match = pos == needle.size() ? idx == i : name.find(needle) != std::string::npos;
      } catch (...) {
        match = name.find(needle) != std::string::npos;
      }
      if (match && (out.empty() || (args.allDevices && out.back() != i))) {
        std::cout << "Using device: " << name << std::endl;
        out.push_back(i);
      }
    }
  if (out.empty()) std::cerr << "No device matches the --devices list" << std::endl;
  if (!out.empty() && args.slabs > 1) out.assign(args.slabs, out.front());
  return out;
}

template <typename N> int run(sph::driver::Args args, const std::vector<int> &devices) {
  using T = size_t;
  using Particle = sph::Particle<T, N, sph::vec>;
  const auto output = args.renderedOutputName();
  std::cout << "Using " << output << " for output" << std::endl;

  sph::SphParams<T, N, sph::vec> param;
  std::vector<Particle> particles;
  sph::McParams<N> mc{};
  const bool moving = args.scene == "cubes";
  if (moving) {
    std::tie(mc, param, particles) = sph::simpleConfigWith2Cubes<T, N, sph::vec>(args.particles, args.solverIter, N(500));
  } else {
    std::tie(param, particles) = sph::damBreakConfig<T, N, sph::vec>(args.particles, args.solverIter, N(500));
  }
  // the stock driver runs with the surface on: param.surface = initialMcParam (benchmark.cpp:29)
  if (!moving) mc = sph::McParams<N>{N(2.0f), N(100), N(25), N(0.5)};  // the same McParams for the dam-break scene
  if (args.surface) param.surface = mc;

  uint32_t flags = (args.fastMath ? PBF_FLAG_FAST_MATH : 0u) | (args.verbose ? PBF_FLAG_STAGE_TIMING : 0u);
  const bool slabbed = devices.size() > 1;
  if (slabbed) {  // x-slabs: device-resident stepping (the surface: every slab its own node planes, concatenated)
    if (!args.resident) std::cout << "Slab mode (" << devices.size() << " slabs): --resident implied" << std::endl;
    else std::cout << "Slab mode (" << devices.size() << " slabs)" << std::endl;
    args.resident = true;
  }
  const bool surfaceTension = args.cohesion > 0 || args.adhesion > 0;
  if (surfaceTension && (slabbed || args.allDevices || args.slabs > 0)) {
    std::cerr << "--surface-tension is a single-device feature: it cannot be combined with --slabs / --all-devices" << std::endl;
    return 1;
  }
  const bool collider = !args.solid.shape.empty();
  if (collider && (slabbed || args.allDevices || args.slabs > 0)) {
    std::cerr << "--collider is a single-device feature: it cannot be combined with --slabs / --all-devices" << std::endl;
    return 1;
  }
  if (collider && !args.resident) std::cout << "--collider takes effect with --resident: ignored" << std::endl;
  const bool scenery = !args.scenery.shape.empty();
  if (scenery && (slabbed || args.allDevices || args.slabs > 0)) {
    std::cerr << "--scenery is a single-device feature: it cannot be combined with --slabs / --all-devices" << std::endl;
    return 1;
  }
  if (scenery && !args.resident) std::cout << "--scenery takes effect with --resident: ignored" << std::endl;
  if ((args.colliderMoves || args.colliderReaction) && (slabbed || args.allDevices || args.slabs > 0)) {
    std::cerr << "--collider-motion / --collider-reaction are single-device features: they cannot be combined with --slabs / --all-devices"
              << std::endl;
    return 1;
  }
  if ((args.colliderMoves || args.colliderReaction) && !(collider && args.resident))
    std::cout << "--collider-motion / --collider-reaction take effect with --resident and --collider: ignored" << std::endl;
  const bool colliderMoves = args.colliderMoves && collider && args.resident;
  if ((args.colliderBody || args.colliderBodyReport) && (slabbed || args.allDevices || args.slabs > 0)) {
    std::cerr << "--collider-body / --collider-body-report are single-device features: they cannot be combined with --slabs / --all-devices"
              << std::endl;
    return 1;
  }
  if (args.colliderBody && args.colliderMoves) {
    std::cerr << "--collider-body and --collider-motion both own the collider's pose: give one of them" << std::endl;
    return 1;
  }
  if (args.colliderBody && collider && args.solid.shape == "mesh") {
    std::cerr << "--collider-body needs --collider=sphere, bowl or plane (the lattice is built about the body's centre)" << std::endl;
    return 1;
  }
  if (args.colliderBody && collider && args.solid.shape == "plane" && !(args.colliderBodyCfg[1] > 0)) {
    std::cerr << "--collider-body with a plane needs its moments: mass,Ixx,Iyy,Izz" << std::endl;
    return 1;
  }
  if ((args.colliderBody || args.colliderBodyReport) && !(collider && args.resident))
    std::cout << "--collider-body / --collider-body-report take effect with --resident and --collider: ignored" << std::endl;
  const bool colliderBody = args.colliderBody && collider && args.resident;
  const size_t colliderBodyReport = colliderBody ? args.colliderBodyReport : 0;
  if (args.colliderBodyContact && !(colliderBody && scenery)) {
    std::cerr << "--collider-body-contact needs --collider-body and --scenery (with --resident and --collider): the body collides with the scenery"
              << std::endl;
    return 1;
  }
  const bool colliderBodyContact = args.colliderBodyContact;
  const size_t colliderReaction = collider && args.resident ? args.colliderReaction : 0;
  if ((args.colliderFriction > 0 || args.colliderFrictionReport) && (slabbed || args.allDevices || args.slabs > 0)) {
    std::cerr << "--collider-friction / --collider-friction-report are single-device features: they cannot be combined with --slabs / --all-devices"
              << std::endl;
    return 1;
  }
  if ((args.colliderFriction > 0 || args.colliderFrictionReport) && !(collider && args.resident))
    std::cout << "--collider-friction / --collider-friction-report take effect with --resident and --collider: ignored" << std::endl;
  const bool colliderFriction = args.colliderFriction > 0 && collider && args.resident;
  const size_t colliderFrictionReport = colliderFriction ? args.colliderFrictionReport : 0;
  if (args.diagnostics && (slabbed || args.allDevices || args.slabs > 0)) {
    std::cerr << "--diagnostics is a single-device feature: it cannot be combined with --slabs / --all-devices" << std::endl;
    return 1;
  }
  if (args.diagnostics && !args.resident) std::cout << "--diagnostics takes effect with --resident: ignored" << std::endl;
  if (!args.probes.empty() && (slabbed || args.allDevices || args.slabs > 0)) {
    std::cerr << "--probe is a single-device feature: it cannot be combined with --slabs / --all-devices" << std::endl;
    return 1;
  }
  if (!args.probes.empty() && !args.resident) std::cout << "--probe takes effect with --resident: ignored" << std::endl;
  const bool whitewater = args.wwCapacity != 0;
  if (whitewater && (slabbed || args.allDevices || args.slabs > 0)) {
    std::cerr << "--whitewater is a single-device feature: it cannot be combined with --slabs / --all-devices" << std::endl;
    return 1;
  }
  if (whitewater && !args.resident) std::cout << "--whitewater takes effect with --resident: ignored" << std::endl;
  if (args.wwSolids && !whitewater) {
    std::cerr << "--whitewater-solids needs --whitewater: it is the diffuse particles that collide with the solids" << std::endl;
    return 1;
  }
  if (args.anisotropy && (slabbed || args.allDevices || args.slabs > 0)) {
    std::cerr << "--anisotropy is a single-device feature: it cannot be combined with --slabs / --all-devices" << std::endl;
    return 1;
  }
  if (args.anisotropy && !args.resident) std::cout << "--anisotropy takes effect with --resident: ignored" << std::endl;
  if (args.anisoSurface && (slabbed || args.allDevices || args.slabs > 0)) {
    std::cerr << "--anisotropic-surface is a single-device feature: it cannot be combined with --slabs / --all-devices" << std::endl;
    return 1;
  }
  if (args.anisoSurface && !args.resident) std::cout << "--anisotropic-surface takes effect with --resident: ignored" << std::endl;
  // --anisotropic-surface --resident: the frames' surface from pbf_surface_anisotropic, at the stock resolution
  const sph::hip_impl::AnisoSurface anisoSurface{double(mc.resolution), args.anisoSurfaceIso,
                                                 {args.anisoSurfaceCfg[0], args.anisoSurfaceCfg[1], args.anisoSurfaceCfg[2],
                                                  args.anisoSurfaceCfg[3], args.anisoSurfaceMinNeighbours}};
  if (args.indexedMesh && (slabbed || args.allDevices || args.slabs > 0)) {
    std::cerr << "--indexed-mesh is a single-device feature: it cannot be combined with --slabs / --all-devices" << std::endl;
    return 1;
  }
  // + inlets and outlets (sph::Scene::sources / drains): with --resident they go to the device (hip_impl::Solver::step),
  // without it into the Scene advance() gets
  sph::Scene<T, N, sph::vec> scene;
  size_t emittedPerFrame = 0;
  for (const auto &a : args.sources) {
    const auto &f = a.v;
    scene.sources.push_back({T(a.tag), {N(f[0]), N(f[1]), N(f[2])}, {N(f[3]), N(f[4]), N(f[5])}, {N(0.2), N(0.6), N(1), N(1)}, N(f[6])});
    const N size = std::sqrt(N(f[6]));  // ompsph.hpp:95-97
    emittedPerFrame += size_t(std::floor(size)) * size_t(std::ceil(size));
  }
  for (const auto &f : args.drains) scene.drains.push_back({T(0), {N(f[0]), N(f[1]), N(f[2])}, N(f[3]), N(0)});
  const bool dynamic = !scene.sources.empty() || !scene.drains.empty();
  if (dynamic && (slabbed || args.allDevices || args.slabs > 0)) {
    std::cerr << "--source / --drain are single-device features: they cannot be combined with --slabs / --all-devices" << std::endl;
    return 1;
  }
  sph::hip_impl::Solver<T, N> solver(N(0.1), devices, flags);
  std::array<double, 3> bodyCentre{0, 0, 0}, bodyMin{0, 0, 0}, bodyMax{0, 0, 0};
  if (surfaceTension) solver.surfaceTension(N(args.cohesion), N(args.adhesion));
  // --collider / --scenery: one builder for both solids (`asScenery`: installed in the world frame through setScenery /
  // setSceneryMesh, never about a body's centre).  false: the mesh was refused and the message printed.
  auto installSolid = [&](const sph::driver::Args::Solid &solid, bool asScenery) -> bool {
    const char *label = asScenery ? "Scenery              : " : "Collider             : ";
    // the analytic distance on a lattice over the box plus one spacing (float64, rounded to N at the end)
    const double spacing = solid.spacing > 0 ? solid.spacing : 0.1 * double(param.scale) / 2;
    const double lo[3] = {double(param.minBound.x), double(param.minBound.y), double(param.minBound.z)};
    const double hi[3] = {double(param.maxBound.x), double(param.maxBound.y), double(param.maxBound.z)};
    std::array<uint32_t, 3> dims;
    std::array<double, 3> origin;
    for (int a = 0; a < 3; ++a) {
      origin[size_t(a)] = lo[a] - spacing;
      dims[size_t(a)] = uint32_t(std::ceil((hi[a] - lo[a]) / spacing)) + 3u;
    }
    // --collider-body: the lattice is the body's own frame, whose origin is the centre of mass — the sphere's centre, for a
    // plane the box's; the start pose puts it back where the static collider would stand
    if (colliderBody && !asScenery)
      for (int a = 0; a < 3; ++a) {
        bodyCentre[size_t(a)] = solid.shape == "plane" ? 0.5 * (lo[a] + hi[a]) : solid.cfg[a];
        origin[size_t(a)] -= bodyCentre[size_t(a)];
        bodyMin[size_t(a)] = lo[a], bodyMax[size_t(a)] = hi[a];
      }
    if (solid.shape == "mesh") {
      const objmesh::Mesh mesh = objmesh::read(solid.mesh);
      pbf_mesh view{mesh.vertices.size() / 3, mesh.triangles.size() / 3, mesh.vertices.data(), mesh.triangles.data()};
      pbf_mesh_info info{};
      // the pre-check: a closed 2-manifold, or with `winding` a soup the kernels can survive
      if ((solid.winding ? pbf_mesh_soup_records(&view, 0, nullptr, &info) : pbf_mesh_records(&view, 0, nullptr, &info)) != PBF_OK) {
        std::cerr << solid.mesh << ": " << pbf_last_error(nullptr) << " (edges " << info.n_edges << ", boundary " << info.boundary_edges
                  << ", non-manifold " << info.nonmanifold_edges << ", misoriented " << info.misoriented_edges << ", degenerate triangles "
                  << info.degenerate_triangles << ")" << std::endl;
        return false;
      }
      pbf_mesh_sdf_stats stats{};
      if (asScenery) solver.setSceneryMesh(mesh.vertices, mesh.triangles, dims, origin, spacing, solid.margin, solid.negate, &stats, solid.winding);
      else solver.setColliderMesh(mesh.vertices, mesh.triangles, dims, origin, spacing, solid.margin, solid.negate, &stats, solid.winding);
      std::cout << label << "mesh " << solid.mesh << (solid.negate ? " (negated)" : "")
                << (solid.winding ? " (winding sign)" : "") << ", " << view.n_triangles << " triangles, volume " << info.volume
                << ", lattice " << dims[0] << " x " << dims[1] << " x " << dims[2] << ", spacing " << spacing << ", margin "
                << solid.margin << ", pairs tested " << stats.pairs_tested << " / " << stats.pairs_total;
      if (solid.winding)
        std::cout << ", boundary " << info.boundary_edges << ", non-manifold " << info.nonmanifold_edges << ", misoriented "
                  << info.misoriented_edges;
      std::cout << std::endl;
    } else {
    const double *g = solid.cfg;
    const std::array<double, 3> centre = asScenery ? std::array<double, 3>{0, 0, 0} : bodyCentre;
    const double nl = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    std::vector<N> phi(size_t(dims[0]) * dims[1] * dims[2]);
    for (uint32_t i = 0; i < dims[0]; ++i)
      for (uint32_t j = 0; j < dims[1]; ++j)
        for (uint32_t k = 0; k < dims[2]; ++k) {
          const double x = (origin[0] + i * spacing) + centre[0], y = (origin[1] + j * spacing) + centre[1],
                       z = (origin[2] + k * spacing) + centre[2];
          double d;
          if (solid.shape == "plane") d = (g[0] * x + g[1] * y + g[2] * z) / nl - g[3];
          else d = std::sqrt((x - g[0]) * (x - g[0]) + (y - g[1]) * (y - g[1]) + (z - g[2]) * (z - g[2])) - g[3];
          phi[(size_t(i) * dims[1] + j) * dims[2] + k] = N(solid.shape == "bowl" ? -d : d);
        }
    if (asScenery) solver.setScenery(dims, origin, spacing, solid.margin, phi.data());
    else solver.setCollider(dims, origin, spacing, solid.margin, phi.data());
    std::cout << label << solid.shape << ", lattice " << dims[0] << " x " << dims[1] << " x " << dims[2]
              << ", spacing " << spacing << ", margin " << solid.margin << std::endl;
    }
    return true;
  };
  if (collider && args.resident && !installSolid(args.solid, false)) return 1;
  if (scenery && args.resident && !installSolid(args.scenery, true)) return 1;
  if (colliderReaction) solver.enableColliderReaction();
  if (colliderBody) {
    // at rest at the collider's centre under the fluid's own acceleration in world units (a unit mass gains constant_force *
    // scale per time: predict works in solver units), its centre kept inside the box
    pbf_collider_body body{};
    const double *c = args.colliderBodyCfg, r = args.solid.cfg[3];
    body.mass = c[0], body.gain = c[4];
    const double force[3] = {double(param.constantForce.x), double(param.constantForce.y), double(param.constantForce.z)};
    for (int a = 0; a < 3; ++a) {
      body.inertia[a] = c[1] > 0 ? c[1 + a] : 0.4 * c[0] * r * r;
      body.accel[a] = force[a] * double(param.scale);
      body.linear_factor[a] = body.angular_factor[a] = 1.0;
      body.centre_min[a] = bodyMin[size_t(a)], body.centre_max[a] = bodyMax[size_t(a)];
      body.pose.rot[4 * a] = 1.0, body.pose.trans[a] = bodyCentre[size_t(a)];
    }
    solver.setColliderBody(body);
    std::cout << "Collider body        : mass " << body.mass << ", moments " << body.inertia[0] << " " << body.inertia[1] << " " << body.inertia[2]
              << ", gain " << body.gain << ", centre " << bodyCentre[0] << " " << bodyCentre[1] << " " << bodyCentre[2] << std::endl;
  }
  if (colliderBodyContact) {  // the collider's zero level, every crossed cell; four fifths of the depth taken back per pass
    pbf_body_contact contact{};
    contact.level = 0, contact.stride = 1, contact.skin = 0, contact.correction = 0.8, contact.slop = 0;
    contact.restitution = args.colliderBodyContactCfg[0], contact.friction = args.colliderBodyContactCfg[1];
    contact.iterations = uint32_t(args.colliderBodyContactCfg[2]);
    solver.setColliderBodyContact(contact);
    std::cout << "Collider body contact: " << solver.colliderBodyContact().points << " surface points, restitution " << contact.restitution
              << ", mu " << contact.friction << ", " << contact.iterations << " pass(es) per step" << std::endl;
  }
  if (colliderFriction) {  // (against a solid at rest; --collider-motion rewrites the velocities every frame, a body supplies its own)
    solver.setColliderFriction(args.colliderFriction);
    std::cout << "Collider friction    : mu " << args.colliderFriction << std::endl;
  }
  // --collider-motion: the pose of the frame numbered f (warm-up frames included), at time f * dt — a rotation by |w| f dt about
  // the axis w through the pivot p (Rodrigues), then the translation v f dt: w = R (b - p) + p + v f dt
  size_t poseFrame = 0;
  auto colliderPoseOf = [&](size_t f, std::array<double, 9> &rot, std::array<double, 3> &trans) {
    const double *m = args.colliderMotion, tau = double(f) * double(param.dt);
    const double wl = std::sqrt((m[3] * m[3] + m[4] * m[4]) + m[5] * m[5]), angle = wl * tau;
    const double k[3] = {wl > 0 ? m[3] / wl : 0.0, wl > 0 ? m[4] / wl : 0.0, wl > 0 ? m[5] / wl : 0.0};
    const double K[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0}, s = std::sin(angle), c1 = 1.0 - std::cos(angle);
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        const double kk = (K[3 * a] * K[b] + K[3 * a + 1] * K[3 + b]) + K[3 * a + 2] * K[6 + b];
        rot[size_t(3 * a + b)] = ((a == b ? 1.0 : 0.0) + s * K[3 * a + b]) + c1 * kk;
      }
    for (int a = 0; a < 3; ++a) {
      const double rp = (rot[size_t(3 * a)] * m[6] + rot[size_t(3 * a + 1)] * m[7]) + rot[size_t(3 * a + 2)] * m[8];
      trans[size_t(a)] = (m[6 + a] - rp) + m[a] * tau;
    }
  };
  if (args.indexedMesh) solver.indexedMesh(true);
  sph::hip_impl::IndexedMesh<N, sph::vec> indexed;  // --indexed-mesh --resident: the last frame's mesh
  // the resident arrays grow by what the inlets emit: room for every frame of the run
  if (args.resident && emittedPerFrame) solver.reserve(particles.size() + (args.warmup + args.iterations) * emittedPerFrame);
  sph::Result<T, N, sph::vec> result;
  auto frameParam = [&](size_t frame) { return moving ? sph::applyMotionSinXCosZ(param, frame) : param; };

  std::vector<double> frameTime;
  hrc::time_point start, end;
  if (args.resident) solver.upload(particles, &param);
  // --whitewater --resident: the first frame probes the potentials with rates 0 and takes the tau ranges from their
  // quantiles; every frame after its fluid step runs one whitewater step
  pbf_whitewater ww{};
  bool wwConfigured = false;
  size_t wwSteps = 0;  // whitewater steps run: the solids' counts exist only after one
  if (whitewater && args.resident) {
    ww.capacity = args.wwCapacity, ww.seed = 1;
    ww.tau_ta[1] = ww.tau_wc[1] = ww.tau_k[1] = 1.0;
    ww.lifetime[0] = 2.0, ww.lifetime[1] = 5.0, ww.k_b = 2.0, ww.k_d = 0.8, ww.spray_below = 6, ww.bubble_from = 20;
    solver.whitewater(ww);
    if (args.wwSolids) {
      pbf_whitewater_solids ws{};
      ws.restitution = args.wwSolidsCfg[0], ws.friction = args.wwSolidsCfg[1], ws.absorb = args.wwSolidsCfg[2] != 0 ? 1u : 0u;
      solver.setWhitewaterSolids(&ws);
    }
  }
  auto one = [&](size_t frame) {
    if (args.resident) {
      if (colliderMoves) {  // the pose of this frame, before it is stepped
        std::array<double, 9> rot;
        std::array<double, 3> trans;
        const double tau = double(poseFrame) * double(param.dt);
        colliderPoseOf(poseFrame++, rot, trans);
        solver.setColliderPose(rot, trans);
        if (colliderFriction) {  // the velocity of the solid's point at the pose's t: v + w x (t - (p + v tau)); the spin is w itself
          const double *m = args.colliderMotion;
          const double d[3] = {trans[0] - (m[6] + m[0] * tau), trans[1] - (m[7] + m[1] * tau), trans[2] - (m[8] + m[2] * tau)};
          solver.setColliderFriction(args.colliderFriction,
                                     {m[0] + (m[4] * d[2] - m[5] * d[1]), m[1] + (m[5] * d[0] - m[3] * d[2]), m[2] + (m[3] * d[1] - m[4] * d[0])},
                                     {m[3], m[4], m[5]});
        }
      }
      solver.step(frameParam(frame), scene);
      if (whitewater && solver.count()) {
        solver.whitewaterStep(frameParam(frame));
        ++wwSteps;
        if (!wwConfigured) {
          solver.whitewaterQuantileTaus(ww);
          ww.k_ta = args.wwTa, ww.k_wc = args.wwWc;
          solver.whitewater(ww);
          wwConfigured = true;
        }
      }
      if (param.surface && solver.count() && args.anisoSurface) {
        if (args.indexedMesh) indexed = solver.surfaceAnisotropicIndexed(frameParam(frame), anisoSurface, scene);
        else result.mesh = solver.surfaceAnisotropic(frameParam(frame), anisoSurface, scene);
      } else if (param.surface && solver.count() && args.indexedMesh) indexed = solver.surfaceIndexed(frameParam(frame));
      else if (param.surface && solver.count()) result.mesh = solver.surface(frameParam(frame));
      solver.sync();  // per-frame time like the reference's blocking advance()
    } else {
      result = solver.advance(frameParam(frame), scene, particles);
    }
  };
  for (size_t frame = 0; frame < args.warmup; ++frame) {
    try {
      one(frame);
    } catch (std::exception const &e) {
      std::cout << "Caught asynchronous exception at warmup frame" << frame << ":\n" << e.what() << "\n";
      throw;
    }
  }
  // --diagnostics: one JSON line per `every` timed frames; its time is kept out of the frame times and of the runtime
  double diagMillis = 0;
  auto report = [&](size_t frame) {
    const auto d0 = hrc::now();
    const auto d = solver.diagnostics(frameParam(frame), /*density=*/solver.count() != 0);
    auto num = [](double x) {  // (JSON has no NaN / Infinity)
      char buf[40];
      std::snprintf(buf, sizeof buf, "%.17g", x);
      return std::isfinite(x) ? std::string(buf) : std::string("null");
    };
    auto vec3 = [&](const double *v) { return "[" + num(v[0]) + "," + num(v[1]) + "," + num(v[2]) + "]"; };
    std::cout << "{\"frame\":" << frame << ",\"diag\":{\"n_fluid\":" << d.fluid << ",\"n_obstacle\":" << d.obstacles
              << ",\"n_nonfinite\":" << d.nonFinite << ",\"mass\":" << num(d.mass) << ",\"moment\":" << vec3(d.moment)
              << ",\"momentum\":" << vec3(d.momentum) << ",\"kinetic\":" << num(d.kinetic) << ",\"max_speed\":" << num(d.maxSpeed)
              << ",\"aabb_min\":" << vec3(d.aabbMin) << ",\"aabb_max\":" << vec3(d.aabbMax) << ",\"n_density\":" << d.densityParticles
              << ",\"nbr_max\":" << d.nbrMax << ",\"rho_min\":" << num(d.rhoMin) << ",\"rho_max\":" << num(d.rhoMax)
              << ",\"rho_mean\":" << num(d.rhoMean) << ",\"err_mean\":" << num(d.errMean) << ",\"err_max\":" << num(d.errMax)
              << ",\"compression_mean\":" << num(d.compressionMean) << ",\"nbr_mean\":" << num(d.nbrMean) << "}}" << std::endl;
    diagMillis += duration_millis(hrc::now() - d0).count();
  };
  // --probe: one JSON line per report with the sums at every probe; its time is kept out like the diagnostics'
  auto probe = [&](size_t frame) {
    const auto d0 = hrc::now();
    std::vector<sph::vec<3, N>> pts;
    for (const auto &q : args.probes) pts.emplace_back(q[0], q[1], q[2]);
    const auto s = solver.sample(frameParam(frame), pts, PBF_SAMPLE_VELOCITY | PBF_SAMPLE_COLOUR);
    auto num = [](double x) {
      char buf[40];
      std::snprintf(buf, sizeof buf, "%.17g", x);
      return std::isfinite(x) ? std::string(buf) : std::string("null");
    };
    std::cout << "{\"frame\":" << frame << ",\"probes\":[";
    for (size_t i = 0; i < pts.size(); ++i) {
      const auto &q = args.probes[i];
      std::cout << (i ? "," : "") << "{\"at\":[" << num(q[0]) << "," << num(q[1]) << "," << num(q[2]) << "],\"rho\":" << num(s.rho[i])
                << ",\"weight\":" << num(s.weight[i]) << ",\"velocity\":[" << num(s.velocity[3 * i]) << "," << num(s.velocity[3 * i + 1])
                << "," << num(s.velocity[3 * i + 2]) << "],\"colour\":[" << num(s.colour[4 * i]) << "," << num(s.colour[4 * i + 1]) << ","
                << num(s.colour[4 * i + 2]) << "," << num(s.colour[4 * i + 3]) << "],\"count\":[" << s.count[2 * i] << ","
                << s.count[2 * i + 1] << "],\"outside\":" << int(s.outside[i]) << "}";
    }
    std::cout << "]}" << std::endl;
    diagMillis += duration_millis(hrc::now() - d0).count();
  };
  // --collider-reaction: one JSON line per report; its time is kept out like the diagnostics'
  auto wrench = [&](size_t frame) {
    const auto d0 = hrc::now();
    const pbf_collider_wrench w = solver.colliderReaction();
    auto num = [](double x) {
      char buf[40];
      std::snprintf(buf, sizeof buf, "%.17g", x);
      return std::isfinite(x) ? std::string(buf) : std::string("null");
    };
    auto vec3 = [&](const double *v) { return "[" + num(v[0]) + "," + num(v[1]) + "," + num(v[2]) + "]"; };
    std::cout << "{\"frame\":" << frame << ",\"wrench\":{\"impulse\":" << vec3(w.impulse) << ",\"angular\":" << vec3(w.angular)
              << ",\"abs_impulse\":" << vec3(w.abs_impulse) << ",\"abs_angular\":" << vec3(w.abs_angular) << ",\"hits\":" << w.hits
              << ",\"particles\":" << w.particles << ",\"step\":" << w.step << "}}" << std::endl;
    diagMillis += duration_millis(hrc::now() - d0).count();
  };
  // --collider-friction-report: the friction pass's sums in the wrench's layout (hits = particles that slid, particles = in contact)
  auto frictionReport = [&](size_t frame) {
    const auto d0 = hrc::now();
    const pbf_collider_wrench w = solver.colliderFrictionReaction();
    auto num = [](double x) {
      char buf[40];
      std::snprintf(buf, sizeof buf, "%.17g", x);
      return std::isfinite(x) ? std::string(buf) : std::string("null");
    };
    auto vec3 = [&](const double *v) { return "[" + num(v[0]) + "," + num(v[1]) + "," + num(v[2]) + "]"; };
    std::cout << "{\"frame\":" << frame << ",\"friction\":{\"impulse\":" << vec3(w.impulse) << ",\"angular\":" << vec3(w.angular)
              << ",\"abs_impulse\":" << vec3(w.abs_impulse) << ",\"abs_angular\":" << vec3(w.abs_angular) << ",\"hits\":" << w.hits
              << ",\"particles\":" << w.particles << ",\"step\":" << w.step << "}}" << std::endl;
    diagMillis += duration_millis(hrc::now() - d0).count();
  };
  // --collider-body-report: one JSON line per report, kept out of the timed frames like the wrench's
  auto bodyReport = [&](size_t frame) {
    const auto d0 = hrc::now();
    const struct pbf_collider_body_state st = solver.colliderBody();
    auto num = [](double x) {
      char buf[40];
      std::snprintf(buf, sizeof buf, "%.17g", x);
      return std::isfinite(x) ? std::string(buf) : std::string("null");
    };
    auto vecn = [&](const double *v, int n) {
      std::string out = "[";
      for (int k = 0; k < n; ++k) out += (k ? "," : "") + num(v[k]);
      return out + "]";
    };
    std::cout << "{\"frame\":" << frame << ",\"body\":{\"rot\":" << vecn(st.pose.rot, 9) << ",\"centre\":" << vecn(st.pose.trans, 3)
              << ",\"quat\":" << vecn(st.quat, 4) << ",\"velocity\":" << vecn(st.velocity, 3) << ",\"angular_velocity\":"
              << vecn(st.angular_velocity, 3) << ",\"impulse\":" << vecn(st.impulse, 3) << ",\"angular\":" << vecn(st.angular, 3)
              << ",\"hits\":" << st.hits << ",\"steps\":" << st.steps << ",\"rejected\":" << st.rejected;
    if (colliderBodyContact) {  // (only with --collider-body-contact: without it the line is what it always was)
      const struct pbf_body_contact_state cs = solver.colliderBodyContact();
      std::cout << ",\"contact_points\":" << cs.points << ",\"contact_depth\":" << num(cs.depth_max) << ",\"contacts\":" << cs.contacts;
    }
    std::cout << "}}" << std::endl;
    diagMillis += duration_millis(hrc::now() - d0).count();
  };
  const bool probing = args.resident && !args.probes.empty();
  start = hrc::now();
  for (size_t frame = 0; frame < args.iterations; ++frame) {
    const auto f0 = hrc::now();
    try {
      one(frame);
    } catch (std::exception const &e) {
      std::cout << "Caught asynchronous exception at benchmark frame" << frame << ":\n" << e.what() << "\n";
      throw;
    }
    frameTime.push_back(duration_millis(hrc::now() - f0).count());
    if (args.resident && args.diagnostics && (frame + 1) % args.diagnostics == 0) report(frame);
    if (colliderReaction && solver.count() && (frame + 1) % colliderReaction == 0) wrench(frame);
    if (colliderBodyReport && (frame + 1) % colliderBodyReport == 0) bodyReport(frame);
    if (colliderFrictionReport && solver.count() && (frame + 1) % colliderFrictionReport == 0) frictionReport(frame);
    if (probing && (args.probeEvery ? (frame + 1) % args.probeEvery == 0 : frame + 1 == args.iterations)) probe(frame);
  }
  end = hrc::now();
  // --anisotropy --resident: the final state's ellipsoids, in the order the download below returns
  sph::hip_impl::Anisotropy<N> ellipsoids;
  const bool anisotropy = args.anisotropy && args.resident && args.warmup + args.iterations > 0;
  if (anisotropy) {
    const pbf_anisotropy cfg{args.anisoCfg[0], args.anisoCfg[1], args.anisoCfg[2], args.anisoCfg[3], args.anisoMinNeighbours};
    ellipsoids = solver.anisotropy(frameParam(args.iterations ? args.iterations - 1 : args.warmup - 1), scene, cfg);
  }
  if (args.resident) solver.download(particles);

  const double seconds = (duration_millis(end - start).count() - diagMillis) / 1000.0;
  const size_t frames = args.iterations;
  const Stats st = frameTime.empty() ? Stats{0, 0, 0, 0} : summaryStats(frameTime);
  std::cout << "Benchmark completed after " << frames << " frames:\n"
            << std::setprecision(4)  //
            << "Runtime              : " << seconds << " s\n"
            << "Framerate            : " << double(frames) / seconds << " fps\n"
            << "Frame-time min       : " << st.min << " ms\n"
            << "Frame-time max       : " << st.max << " ms\n"
            << "Frame-time mean       : " << st.mean << " ms\n"
            << "Frame-time stdDev     : " << st.stdDev << " ms\n"
            << "Final Vertex count   : " << result.mesh.vs.size() << "\n"
            << "Final Particle count : " << particles.size() << " \n"
            << std::endl;
  const double psps = double(particles.size()) * double(frames) / seconds;
  std::cout << std::setprecision(6) << "Particle-steps/s     : " << psps << " (" << (args.resident ? "device-resident" : "advance(): upload+step+download per frame")
            << ", K=" << args.solverIter << ", " << (args.fp64 ? "fp64" : "fp32") << ")\n";
  const auto &imesh = args.resident ? indexed : solver.lastIndexedMesh();
  sph::hip_impl::WhitewaterParticles<N, sph::vec> diffuse;
  if (whitewater && args.resident) {
    const auto &w = solver.whitewaterStats();
    diffuse = solver.whitewaterParticles();
    std::cout << "Whitewater           : " << w.alive << " alive (" << w.kind[0] << " spray, " << w.kind[1] << " foam, " << w.kind[2]
              << " bubble), last frame: " << w.emitted << " emitted, " << w.dropped << " dropped, " << w.died << " died\n";
    if (args.wwSolids && wwSteps) {
      const auto s = solver.whitewaterSolidsStats();
      std::cout << "Whitewater solids    : last frame: " << s.hit_collider << " hit the collider, " << s.hit_scenery << " hit the scenery, "
                << s.absorbed << " absorbed, " << s.born_inside << " born inside (" << s.step << " steps)\n";
    }
  }
  if (args.indexedMesh)
    std::cout << "Indexed mesh         : " << imesh.vs.size() << " vertices, " << imesh.tris.size() / 3 << " triangles\n";
  if (args.verbose) {
    const char *names[16];
    double ms[16];
    uint64_t calls[16];
    const int k = pbf_stage_times(solver.context(), names, ms, calls, 16);
    std::cout << "Stopwatch[ advance]:\n";
    for (int i = 0; i < k; ++i)
      std::cout << "    ->`" << names[i] << "` : " << ms[i] << "ms x " << double(calls[i]) / double(args.warmup + frames) << "/frame\n";
  }
  if (args.json)
    std::cout << "{\"impl\":\"hip\",\"scene\":\"" << args.scene << "\",\"particles\":" << particles.size()
              << ",\"solver_iter\":" << args.solverIter << ",\"fp64\":" << (args.fp64 ? "true" : "false")
              << ",\"resident\":" << (args.resident ? "true" : "false") << ",\"slabs\":" << devices.size() << ",\"frames\":" << frames
              << ",\"seconds\":" << seconds << ",\"particle_steps_per_s\":" << psps << ",\"frame_ms_mean\":" << st.mean
              << "}" << std::endl;
  sph::save(result, particles, output);
  if (whitewater && args.resident && !output.empty()) {  // whitewater.ply: position + kind (0 spray, 1 foam, 2 bubble)
    std::ofstream ply(std::filesystem::path(output) / "whitewater.ply");
    ply << "ply\nformat ascii 1.0\nelement vertex " << diffuse.positions.size()
        << "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar kind\nend_header\n";
    ply.precision(std::numeric_limits<N>::max_digits10);
    for (size_t i = 0; i < diffuse.positions.size(); ++i)
      ply << diffuse.positions[i].x << ' ' << diffuse.positions[i].y << ' ' << diffuse.positions[i].z << ' ' << int(diffuse.kind[i]) << '\n';
  }
  if (anisotropy && !output.empty()) {  // ellipsoids.ply: one vertex per FLUID particle, semi-axes h * scale * radius_k along axis k
    const size_t n = ellipsoids.neighbours.size();
    size_t fluid = 0;
    for (size_t i = 0; i < n && i < particles.size(); ++i) fluid += particles[i].type == sph::Type::Fluid ? 1 : 0;
    std::ofstream ply(std::filesystem::path(output) / "ellipsoids.ply");
    ply << "ply\nformat ascii 1.0\nelement vertex " << fluid << "\nproperty float x\nproperty float y\nproperty float z\n";
    for (const char *name : {"r1", "r2", "r3", "a1x", "a1y", "a1z", "a2x", "a2y", "a2z", "a3x", "a3y", "a3z"})
      ply << "property float " << name << "\n";
    ply << "property uint neighbours\nend_header\n";
    ply.precision(std::numeric_limits<N>::max_digits10);
    for (size_t i = 0; i < n && i < particles.size(); ++i) {
      if (particles[i].type != sph::Type::Fluid) continue;
      for (size_t k = 0; k < 3; ++k) ply << ellipsoids.centre[k * n + i] << ' ';
      for (size_t k = 0; k < 3; ++k) ply << ellipsoids.radii[k * n + i] << ' ';
      for (size_t k = 0; k < 9; ++k) ply << ellipsoids.axes[k * n + i] << ' ';
      ply << ellipsoids.neighbours[i] << '\n';
    }
  }
  if (args.indexedMesh && !output.empty()) {  // mesh.obj as an indexed OBJ: V `v`, V `vn`, T `f a//a b//b c//c`
    std::ofstream obj(std::filesystem::path(output) / "mesh.obj");
    for (const auto &v : imesh.vs) obj << "v " << v.x << ' ' << v.y << ' ' << v.z << '\n';
    for (const auto &n : imesh.ns) obj << "vn " << n.x << ' ' << n.y << ' ' << n.z << '\n';
    for (size_t t = 0; t + 2 < imesh.tris.size(); t += 3) {
      obj << 'f';
      for (size_t k = 0; k < 3; ++k) obj << ' ' << imesh.tris[t + k] + 1 << "//" << imesh.tris[t + k] + 1;
      obj << '\n';
    }
  }
  std::cout << "Results flushed." << std::endl;
  return 0;
}

}  // namespace

int main(int argc, char *argv[]) {
  // advance() returns the mesh by value (src/sph.hpp:114-125): three freshly allocated vectors per frame — 54 MB at 1 M
  // particles — which `result = solver.advance(...)` (benchmark.cpp:33,47) frees again one frame later.  Left alone, glibc
  // hands the freed top of the heap back to the system every frame (the trim threshold follows the mmap threshold) and
  // the next frame's vectors fault every page in again: ~2 ms per frame of page faults.  Keep the memory instead.
  mallopt(M_MMAP_THRESHOLD, 32 << 20);
  mallopt(M_TRIM_THRESHOLD, 1 << 30);
  mallopt(M_TOP_PAD, 128 << 20);
  sph::driver::Args args(200, "./out_{impl}_{type}_{iter}");
  if (!args.parse(argc, argv)) return EXIT_SUCCESS;  // the reference exits 0 after help / parse errors too
  if (args.impl != "hip") {
    std::cerr << "Implementation `" << args.impl << "` is not part of this build: this driver ships the `hip` backend only "
              << "(omp/ocl/sycl live in the reference)" << std::endl;
    return EXIT_FAILURE;
  }
  const std::vector<int> devices = findDevices(args);
  if (devices.empty()) return args.list ? EXIT_SUCCESS : EXIT_FAILURE;
  try {
    return args.fp64 ? run<double>(args, devices) : run<float>(args, devices);
  } catch (const std::exception &e) {
    std::cerr << "benchmark failed: " << e.what() << std::endl;
    return EXIT_FAILURE;
  }
}
