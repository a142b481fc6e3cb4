// test_sample_shim.cpp — sph::hip_impl::Solver::sample() / sampleLattice() against the C ABI they wrap: the shim hands the
// library's sums through bit for bit, in both precisions, divides where it says it does, refuses before a step, and a call
// between two steps leaves the next step's result alone.  Prints "ok <name>" / "FAIL <name>" lines and "ALL OK";
// tests/test_sample_gpu.py runs it on a GPU.
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
  using V3 = sph::vec<3, N>;
  auto [mc, config, particles] = sph::simpleConfigWith2Cubes<T, N, sph::vec>(2048, 2, N(500));
  (void)mc;
  for (size_t i = 0; i < particles.size(); i += 9) particles[i].type = sph::Type::Obstacle;

  sph::hip_impl::Solver<T, N> a(N(0.1)), b(N(0.1));
  a.upload(particles), b.upload(particles);
  std::vector<V3> pts;
  for (size_t i = 0; i < particles.size(); i += 13) pts.push_back(particles[i].position + V3(3, -2, 1) * N(1));
  pts.push_back(V3(-500, 0, 0));  // outside the grid
  bool refused = false;
  try {
    (void)a.sample(config, pts);
  } catch (const std::exception &e) {
    refused = std::strstr(e.what(), "pbf_sample_points") != nullptr;
  }
  check(tag + "sample_shim_needs_a_step", refused);

  a.step(config), b.step(config);
  const uint32_t what = PBF_SAMPLE_VELOCITY | PBF_SAMPLE_COLOUR;
  const auto s = a.sample(config, pts, what);

  // the same call through the C ABI
  const size_t n = pts.size();
  pbf_params p{};
  p.dt = double(config.dt), p.scale = double(config.scale), p.iteration = config.iteration;
  p.constant_force[0] = config.constantForce.x, p.constant_force[1] = config.constantForce.y, p.constant_force[2] = config.constantForce.z;
  p.min_bound[0] = config.minBound.x, p.min_bound[1] = config.minBound.y, p.min_bound[2] = config.minBound.z;
  p.max_bound[0] = config.maxBound.x, p.max_bound[1] = config.maxBound.y, p.max_bound[2] = config.maxBound.z;
  std::vector<double> flat(3 * n);
  for (size_t i = 0; i < n; ++i) flat[3 * i] = pts[i].x, flat[3 * i + 1] = pts[i].y, flat[3 * i + 2] = pts[i].z;
  std::vector<N> rho(n), weight(n), mv(3 * n), mcol(4 * n);
  std::vector<uint32_t> count(2 * n);
  std::vector<uint8_t> outside(n);
  const pbf_sample_out out{rho.data(), weight.data(), mv.data(), mcol.data(), count.data(), outside.data()};
  const int rc = pbf_sample_points(a.context(), &p, n, flat.data(), what, &out);
  check(tag + "sample_shim_capi_ok", rc == PBF_OK);
  check(tag + "sample_shim_points_bits", same_bytes(s.rho, rho) && same_bytes(s.weight, weight) && same_bytes(s.mv, mv) &&
                                             same_bytes(s.mc, mcol) && same_bytes(s.count, count) && same_bytes(s.outside, outside));
  bool hit = false, divided = s.velocity.size() == 3 * n && s.colour.size() == 4 * n;
  for (size_t i = 0; i < n && divided; ++i) {
    hit = hit || weight[i] > N(0);
    for (size_t k = 0; k < 3; ++k) divided = divided && s.velocity[3 * i + k] == (weight[i] == N(0) ? N(0) : mv[3 * i + k] / weight[i]);
    for (size_t k = 0; k < 4; ++k) divided = divided && s.colour[4 * i + k] == (weight[i] == N(0) ? N(0) : mcol[4 * i + k] / weight[i]);
  }
  check(tag + "sample_shim_division", divided && hit);
  check(tag + "sample_shim_outside", outside[n - 1] == 1 && rho[n - 1] == N(0) && outside[0] == 0);

  // the lattice, with fewer outputs
  const std::array<uint64_t, 3> dims{5, 7, 9};
  const V3 origin = particles[0].position - V3(40, 40, 40) * N(1), spacing(N(17), N(23), N(11));
  const auto l = a.sampleLattice(config, origin, spacing, dims, PBF_SAMPLE_VELOCITY);
  const size_t m = 5 * 7 * 9;
  std::vector<N> lrho(m), lweight(m), lmv(3 * m);
  std::vector<uint32_t> lcount(2 * m);
  std::vector<uint8_t> loutside(m);
  const pbf_sample_out lout{lrho.data(), lweight.data(), lmv.data(), nullptr, lcount.data(), loutside.data()};
  const double o3[3] = {double(origin.x), double(origin.y), double(origin.z)}, s3[3] = {17, 23, 11};
  check(tag + "sample_shim_lattice_capi_ok", pbf_sample_lattice(a.context(), &p, o3, s3, dims.data(), PBF_SAMPLE_VELOCITY, &lout) == PBF_OK);
  check(tag + "sample_shim_lattice_bits", same_bytes(l.rho, lrho) && same_bytes(l.weight, lweight) && same_bytes(l.mv, lmv) &&
                                              l.mc.empty() && l.colour.empty() && same_bytes(l.count, lcount) &&
                                              same_bytes(l.outside, loutside));

  // the observer changes nothing: one more step on both, the one that was asked in between included
  a.step(config), b.step(config);
  std::vector<P> ya, yb;
  a.download(ya), b.download(yb);
  check(tag + "sample_shim_observer", shim::same_particles(ya, yb));
}

int main() {
  run<float>("fp32_");
  run<double>("fp64_");
  return shim::finish();
}
