// test_whitewater_shim.cpp — sph::hip_impl::Solver::whitewater() / whitewaterStep() / whitewaterParticles() against the C ABI
// they wrap, in both precisions: the shim hands the library's pool through bit for bit, advance() runs one whitewater step
// after each fluid step once configured, the fluid never notices, and an unconfigured solver refuses.  Prints "ok <name>" /
// "FAIL <name>" lines and "ALL OK"; tests/test_whitewater_gpu.py runs it on a GPU.
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
  for (size_t i = 0; i < particles.size(); i += 9) particles[i].type = sph::Type::Obstacle;

  pbf_whitewater ww{};
  ww.capacity = 4096, ww.seed = 3, ww.k_ta = 300, ww.k_wc = 300;
  ww.tau_ta[0] = 0, ww.tau_ta[1] = 1, ww.tau_wc[0] = 0, ww.tau_wc[1] = 1, ww.tau_k[0] = 0, ww.tau_k[1] = 0.05;
  ww.lifetime[0] = 2, ww.lifetime[1] = 5, ww.k_b = 2, ww.k_d = 0.8, ww.spray_below = 6, ww.bubble_from = 20;

  // resident path: shim calls on a, the C ABI on b
  sph::hip_impl::Solver<T, N> a(N(0.1)), b(N(0.1)), plain(N(0.1));
  a.upload(particles), b.upload(particles), plain.upload(particles);
  bool refused = false;
  try {
    (void)a.whitewaterStep(config);
  } catch (const std::exception &e) {
    refused = std::strstr(e.what(), "pbf_whitewater_step") != nullptr;
  }
  check(tag + "whitewater_shim_needs_configure", refused);
  a.whitewater(ww);
  check(tag + "whitewater_shim_capi_configure", pbf_whitewater_configure(b.context(), &ww) == PBF_OK);
  pbf_params p{};
  p.dt = double(config.dt), p.scale = double(config.scale), p.iteration = config.iteration;
  p.constant_force[0] = config.constantForce.x, p.constant_force[1] = config.constantForce.y, p.constant_force[2] = config.constantForce.z;
  p.min_bound[0] = config.minBound.x, p.min_bound[1] = config.minBound.y, p.min_bound[2] = config.minBound.z;
  p.max_bound[0] = config.maxBound.x, p.max_bound[1] = config.maxBound.y, p.max_bound[2] = config.maxBound.z;
  bool statsSame = true, capiOk = true;
  pbf_whitewater_stats sa{}, sb{};
  for (int f = 0; f < 4; ++f) {
    a.step(config), b.step(config), plain.step(config);
    sa = a.whitewaterStep(config);
    capiOk = capiOk && pbf_whitewater_step(b.context(), &p, &sb) == PBF_OK;
    statsSame = statsSame && !std::memcmp(&sa, &sb, sizeof(sa));
  }
  check(tag + "whitewater_shim_capi_ok", capiOk);
  check(tag + "whitewater_shim_stats", statsSame && sa.alive > 0 && !std::memcmp(&sa, &a.whitewaterStats(), sizeof(sa)));
  const auto pa = a.whitewaterParticles();
  const size_t n = pbf_whitewater_count(b.context());
  sph::hip_impl::WhitewaterParticles<N, sph::vec> pb;
  pb.positions.resize(n), pb.velocities.resize(n), pb.life.resize(n), pb.kind.resize(n), pb.parentId.resize(n);
  check(tag + "whitewater_shim_capi_download",
        pbf_whitewater_download(b.context(), pb.positions.data(), pb.velocities.data(), pb.life.data(), pb.kind.data(), pb.parentId.data()) == PBF_OK);
  check(tag + "whitewater_shim_pool_bits", pa.positions.size() == sa.alive && same_pool(pa, pb));
  std::vector<P> ya, yp;
  a.download(ya), plain.download(yp);
  check(tag + "whitewater_shim_observer", shim::same_particles(ya, yp));

  // advance(): configured, one whitewater step after each fluid step — the same frames by hand on d
  sph::hip_impl::Solver<T, N> c(N(0.1)), d(N(0.1));
  c.whitewater(ww), d.whitewater(ww);
  std::vector<P> xc = particles, xd = particles;
  const sph::Scene<T, N, sph::vec> scene{};
  bool frames = true;
  for (int f = 0; f < 3; ++f) {
    (void)c.advance(config, scene, xc);
    d.upload(xd);
    d.step(config);
    const auto sd = d.whitewaterStep(config);
    d.download(xd);
    frames = frames && !std::memcmp(&sd, &c.whitewaterStats(), sizeof(sd));
  }
  check(tag + "whitewater_shim_advance_steps", frames && c.whitewaterStats().alive > 0);
  check(tag + "whitewater_shim_advance_pool", same_pool(c.whitewaterParticles(), d.whitewaterParticles()));
  check(tag + "whitewater_shim_advance_fluid", shim::same_particles(xc, xd));
  ww.capacity = 0;
  c.whitewater(ww);
  (void)c.advance(config, scene, xc);
  check(tag + "whitewater_shim_off", c.whitewaterParticles().positions.empty() && pbf_whitewater_count(c.context()) == 0);
}

int main() {
  run<float>("fp32_");
  run<double>("fp64_");
  return shim::finish();
}
