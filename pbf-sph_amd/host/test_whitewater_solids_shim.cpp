// test_whitewater_solids_shim.cpp — sph::hip_impl::Solver::setWhitewaterSolids() / whitewaterSolidsStats() against the C ABI
// they wrap, in both precisions.  The two-cube scene with whitewater on and a floor plane a quarter of the box up as scenery:
// the shim hands the library's pool and counts through bit for bit, no diffuse particle is left under the plane, the setting
// changes the pool and not the fluid, NULL turns it off, and the stats refuse while it is off.  Prints "ok <name>" /
// "FAIL <name>" lines and "ALL OK"; tests/test_whitewater_solids_gpu.py runs it on a GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "hipsph.hpp"
#include "shim_check.hpp"

using T = size_t;

using shim::check;
using shim::same_bytes;
template <typename W> static bool same_pool(const W &a, const W &b) {
  return same_bytes(a.positions, b.positions) && same_bytes(a.velocities, b.velocities) && same_bytes(a.life, b.life) &&
         same_bytes(a.kind, b.kind) && same_bytes(a.parentId, b.parentId);
}

template <typename N> static void run(const std::string &tag) {
  using P = sph::Particle<T, N, sph::vec>;
  auto [mc, config, particles] = sph::simpleConfigWith2Cubes<T, N, sph::vec>(2048, 2, N(500));
  (void)mc;
  config.surface.reset();

  pbf_whitewater ww{};
  ww.capacity = 4096, ww.seed = 3, ww.k_ta = 300, ww.k_wc = 300;
  ww.tau_ta[0] = 0, ww.tau_ta[1] = 1, ww.tau_wc[0] = 0, ww.tau_wc[1] = 1, ww.tau_k[0] = 0, ww.tau_k[1] = 0.05;
  ww.lifetime[0] = 2, ww.lifetime[1] = 5, ww.k_b = 2, ww.k_d = 0.8, ww.spray_below = 6, ww.bubble_from = 20;
  pbf_whitewater_solids ws{};
  ws.restitution = 0.25, ws.friction = 0.5;

  // the floor plane as a lattice over the box plus one spacing
  const double lo[3] = {double(config.minBound.x), double(config.minBound.y), double(config.minBound.z)};
  const double hi[3] = {double(config.maxBound.x), double(config.maxBound.y), double(config.maxBound.z)};
  const double spacing = (hi[0] - lo[0]) / 15.0, margin = 0.1 * spacing;
  std::array<uint32_t, 3> dims;
  std::array<double, 3> origin;
  for (int a = 0; a < 3; ++a) {
    origin[size_t(a)] = lo[a] - spacing;
    dims[size_t(a)] = uint32_t(std::ceil((hi[a] - lo[a]) / spacing)) + 3u;
  }
  const double floorY = lo[1] + 0.25 * (hi[1] - lo[1]);
  std::vector<N> plane(size_t(dims[0]) * dims[1] * dims[2]);
  for (uint32_t i = 0; i < dims[0]; ++i)
    for (uint32_t j = 0; j < dims[1]; ++j)
      for (uint32_t k = 0; k < dims[2]; ++k) plane[(size_t(i) * dims[1] + j) * dims[2] + k] = N(origin[1] + j * spacing - floorY);

  // a: the shim;  b: the C ABI;  off: whitewater without the setting.  The fluid runs WITHOUT the scenery until the last frames,
  // so that fluid, and with it children, are under the plane when it arrives.
  sph::hip_impl::Solver<T, N> a(N(0.1)), b(N(0.1)), off(N(0.1));
  a.upload(particles), b.upload(particles), off.upload(particles);
  a.whitewater(ww), b.whitewater(ww), off.whitewater(ww);
  bool refused = false;
  try {
    (void)a.whitewaterSolidsStats();
  } catch (const std::exception &e) {
    refused = std::strstr(e.what(), "pbf_whitewater_solids_stats") != nullptr;
  }
  check(tag + "whitewater_solids_shim_stats_need_the_setting", refused);
  a.setWhitewaterSolids(&ws);
  check(tag + "whitewater_solids_shim_capi_set", pbf_set_whitewater_solids(b.context(), &ws) == PBF_OK);
  pbf_whitewater_solids bad = ws;
  bad.restitution = 1.5;
  refused = false;
  try {
    a.setWhitewaterSolids(&bad);
  } catch (const std::exception &e) {
    refused = std::strstr(e.what(), "pbf_set_whitewater_solids") != nullptr;
  }
  check(tag + "whitewater_solids_shim_refuses_a_bad_setting", refused);

  pbf_params p{};
  p.dt = double(config.dt), p.scale = double(config.scale), p.iteration = config.iteration;
  p.constant_force[0] = config.constantForce.x, p.constant_force[1] = config.constantForce.y, p.constant_force[2] = config.constantForce.z;
  p.min_bound[0] = config.minBound.x, p.min_bound[1] = config.minBound.y, p.min_bound[2] = config.minBound.z;
  p.max_bound[0] = config.maxBound.x, p.max_bound[1] = config.maxBound.y, p.max_bound[2] = config.maxBound.z;
  bool countsSame = true, capiOk = true;
  unsigned long long born = 0, hits = 0;
  for (int f = 0; f < 6; ++f) {
    if (f == 3) {
      a.setScenery(dims, origin, spacing, margin, plane.data()), off.setScenery(dims, origin, spacing, margin, plane.data());
      pbf_collider_sdf sdf{};
      for (int k = 0; k < 3; ++k) sdf.dims[k] = dims[size_t(k)], sdf.origin[k] = origin[size_t(k)];
      sdf.spacing = spacing, sdf.margin = margin, sdf.phi = plane.data();
      capiOk = capiOk && pbf_set_scenery(b.context(), &sdf) == PBF_OK;
    }
    a.step(config), b.step(config), off.step(config);
    (void)a.whitewaterStep(config), (void)off.whitewaterStep(config);
    capiOk = capiOk && pbf_whitewater_step(b.context(), &p, nullptr) == PBF_OK;
    const auto sa = a.whitewaterSolidsStats();
    struct pbf_whitewater_solids_stats sb {};
    capiOk = capiOk && pbf_whitewater_solids_stats(b.context(), &sb) == PBF_OK;
    countsSame = countsSame && !std::memcmp(&sa, &sb, sizeof(sa)) && sa.step == uint64_t(f + 1);
    if (f < 3) countsSame = countsSame && sa.hit_scenery == 0 && sa.born_inside == 0;  // (no lattice yet: nothing ran)
    born += sa.born_inside, hits += sa.hit_scenery;
  }
  check(tag + "whitewater_solids_shim_capi_ok", capiOk);
  check(tag + "whitewater_solids_shim_counts", countsSame && born + hits > 0, "born %llu hits %llu", born, hits);
  const auto pa = a.whitewaterParticles();
  const size_t n = pbf_whitewater_count(b.context());
  sph::hip_impl::WhitewaterParticles<N, sph::vec> pb;
  pb.positions.resize(n), pb.velocities.resize(n), pb.life.resize(n), pb.kind.resize(n), pb.parentId.resize(n);
  check(tag + "whitewater_solids_shim_capi_download",
        pbf_whitewater_download(b.context(), pb.positions.data(), pb.velocities.data(), pb.life.data(), pb.kind.data(), pb.parentId.data()) == PBF_OK);
  check(tag + "whitewater_solids_shim_pool_bits", !pa.positions.empty() && same_pool(pa, pb));
  // the plane is exact in the lattice (phi is linear in y): the projection lands on floorY + margin within a few roundings of
  // the box's size; 1e-4 of a spacing is far above them and far below the margin
  double lowest = 1e300;
  for (const auto &x : pa.positions) lowest = std::fmin(lowest, double(x.y));
  check(tag + "whitewater_solids_shim_nobody_under_the_plane", lowest >= floorY + margin - 1e-4 * spacing, "lowest %g, plane %g", lowest,
        floorY + margin);
  check(tag + "whitewater_solids_shim_changes_the_pool", !same_pool(pa, off.whitewaterParticles()));

  // off again: the stats refuse, and the next whitewater step of a and of a solver that was never set agree on a fresh pool
  a.setWhitewaterSolids(nullptr);
  refused = false;
  try {
    (void)a.whitewaterSolidsStats();
  } catch (const std::exception &e) {
    refused = std::strstr(e.what(), "pbf_whitewater_solids_stats") != nullptr;
  }
  check(tag + "whitewater_solids_shim_off_refuses_stats", refused);
  std::vector<P> ya, yb;
  a.download(ya), b.download(yb);
  check(tag + "whitewater_solids_shim_fluid_same", shim::same_particles(ya, yb));
}

int main() {
  run<float>("fp32_");
  run<double>("fp64_");
  return shim::finish();
}
