// test_aniso_shim.cpp — sph::hip_impl::Solver::anisotropy() against the C ABI it wraps: the shim hands the library's arrays
// through bit for bit, in both precisions, refuses before a step, and a call between two steps leaves the next step's result
// alone.  Prints "ok <name>" / "FAIL <name>" lines and "ALL OK"; tests/test_anisotropy_gpu.py runs it on a GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "hipsph.hpp"
#include "shim_check.hpp"

using T = size_t;

using shim::check;
using shim::same_bytes;

template <typename N> static void run(const std::string &tag) {
  using P = sph::Particle<T, N, sph::vec>;
  auto [mc, config, particles] = sph::simpleConfigWith2Cubes<T, N, sph::vec>(2048, 2, N(500));
  (void)mc;
  for (size_t i = 0; i < particles.size(); i += 9) particles[i].type = sph::Type::Obstacle;
  const sph::Scene<T, N, sph::vec> scene{};
  const pbf_anisotropy cfg{0.9, 4.0, 20.0 / 3.0, 0.5, 8u};

  sph::hip_impl::Solver<T, N> a(N(0.1)), b(N(0.1));
  a.upload(particles), b.upload(particles);
  bool refused = false;
  try {
    (void)a.anisotropy(config, scene, cfg);
  } catch (const std::exception &e) {
    refused = std::strstr(e.what(), "pbf_anisotropy_compute") != nullptr;
  }
  check(tag + "aniso_shim_needs_a_step", refused);

  a.step(config), b.step(config);
  const auto s = a.anisotropy(config, scene, cfg);

  // the same call through the C ABI
  const size_t n = pbf_count(a.context());
  pbf_params p{};
  p.dt = double(config.dt), p.scale = double(config.scale), p.iteration = config.iteration;
  p.constant_force[0] = config.constantForce.x, p.constant_force[1] = config.constantForce.y, p.constant_force[2] = config.constantForce.z;
  p.min_bound[0] = config.minBound.x, p.min_bound[1] = config.minBound.y, p.min_bound[2] = config.minBound.z;
  p.max_bound[0] = config.maxBound.x, p.max_bound[1] = config.maxBound.y, p.max_bound[2] = config.maxBound.z;
  std::vector<N> centre(3 * n), G(6 * n), axes(9 * n), radii(3 * n);
  std::vector<uint32_t> nbr(n);
  const pbf_anisotropy_out out{centre.data(), G.data(), axes.data(), radii.data(), nbr.data()};
  check(tag + "aniso_shim_capi_ok", n == particles.size() && pbf_anisotropy_compute(a.context(), &p, &cfg, &out) == PBF_OK);
  check(tag + "aniso_shim_bits", same_bytes(s.centre, centre) && same_bytes(s.G, G) && same_bytes(s.axes, axes) &&
                                     same_bytes(s.radii, radii) && same_bytes(s.neighbours, nbr));
  // an obstacle's record is its position and zeros, a fluid particle's radii are ordered
  std::vector<P> now;
  a.download(now);
  size_t aniso = 0, iso = 0;
  bool obstaclesZero = true, ordered = true;
  for (size_t i = 0; i < n; ++i) {
    if (now[i].type == sph::Type::Obstacle) {
      obstaclesZero = obstaclesZero && radii[i] == N(0) && G[i] == N(0) && axes[i] == N(0) && nbr[i] == 0u &&
                      centre[i] == now[i].position.x && centre[n + i] == now[i].position.y && centre[2 * n + i] == now[i].position.z;
      continue;
    }
    (nbr[i] > cfg.min_neighbours ? aniso : iso) += 1;
    ordered = ordered && radii[i] >= radii[n + i] && radii[n + i] >= radii[2 * n + i] && radii[2 * n + i] > N(0);
  }
  check(tag + "aniso_shim_anisotropic_branch", aniso > 0);
  // the other branch: no particle has more than 100000 neighbours, so every fluid particle gets radii = k_n and axes = I
  pbf_anisotropy few = cfg;
  few.min_neighbours = 100000u;
  const auto f = a.anisotropy(config, scene, few);
  bool isotropic = f.radii.size() == 3 * n;
  for (size_t i = 0; i < n && isotropic; ++i)
    if (now[i].type != sph::Type::Obstacle)
      isotropic = f.radii[i] == N(0.5) && f.radii[2 * n + i] == N(0.5) && f.axes[i] == N(1) && f.axes[n + i] == N(0) &&
                  f.axes[4 * n + i] == N(1) && f.axes[8 * n + i] == N(1);
  check(tag + "aniso_shim_isotropic_branch", isotropic && aniso + iso > 0);
  check(tag + "aniso_shim_obstacles", obstaclesZero);
  check(tag + "aniso_shim_radii_ordered", ordered);

  // the observer changes nothing: one more step on both, the one that was asked in between included
  a.step(config), b.step(config);
  std::vector<P> ya, yb;
  a.download(ya), b.download(yb);
  check(tag + "aniso_shim_observer", shim::same_particles(ya, yb));
}

int main() {
  run<float>("fp32_");
  run<double>("fp64_");
  return shim::finish();
}
