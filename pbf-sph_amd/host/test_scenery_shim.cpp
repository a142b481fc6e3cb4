// test_scenery_shim.cpp — sph::hip_impl::Solver::setScenery() / clearScenery() / sampleScenery() through advance().
//   test_scenery_shim <frames>
// The two-cube scene over a floor plane a quarter of the box up, as a lattice over the box plus one spacing.  Checked here:
// the scenery changes the run; scenery alone is the static collider with the same lattice, bit for bit; clearScenery() gives
// the run that never had one; a collider (a ball in the middle) beside the scenery runs, differs from the scenery alone and
// leaves the collider's reaction readable; sampleScenery() finds a point under the plane and lifts it.  Prints "ok <name>" /
// "FAIL <name>" lines and "ALL OK".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hipsph.hpp"
#include "shim_check.hpp"

using T = size_t;
using N = float;
using P = sph::Particle<T, N, sph::vec>;

using shim::check;

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: test_scenery_shim <frames>\n");
    return 2;
  }
  const int frames = std::atoi(argv[1]);

  auto [mc, config, particles] = sph::simpleConfigWith2Cubes<T, N, sph::vec>(2048, 4, N(500));
  (void)mc;
  const sph::Scene<T, N, sph::vec> scene{};
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
  const double c[3] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])}, r = 0.2 * (hi[0] - lo[0]);
  std::vector<N> plane(size_t(dims[0]) * dims[1] * dims[2]), ball(plane.size());
  for (uint32_t i = 0; i < dims[0]; ++i)
    for (uint32_t j = 0; j < dims[1]; ++j)
      for (uint32_t k = 0; k < dims[2]; ++k) {
        const double x = origin[0] + i * spacing, y = origin[1] + j * spacing, z = origin[2] + k * spacing;
        const size_t at = (size_t(i) * dims[1] + j) * dims[2] + k;
        plane[at] = N(y - floorY);
        ball[at] = N(std::sqrt((x - c[0]) * (x - c[0]) + (y - c[1]) * (y - c[1]) + (z - c[2]) * (z - c[2])) - r);
      }

  std::vector<P> with = particles, without = particles, cleared = particles, asCollider = particles, both = particles;
  sph::hip_impl::Solver<T, N> a(N(0.1)), b(N(0.1)), d(N(0.1)), e(N(0.1)), f(N(0.1));
  a.setScenery(dims, origin, spacing, margin, plane.data());
  d.setScenery(dims, origin, spacing, margin, plane.data()).clearScenery();
  e.setCollider(dims, origin, spacing, margin, plane.data());
  f.setCollider(dims, origin, spacing, margin, ball.data()).setScenery(dims, origin, spacing, margin, plane.data());
  for (int k = 0; k < frames; ++k) {
    (void)a.advance(config, scene, with);
    (void)b.advance(config, scene, without);
    (void)d.advance(config, scene, cleared);
    (void)e.advance(config, scene, asCollider);
    (void)f.advance(config, scene, both);
  }
  check("scenery_shim_changes_the_run", with.size() == without.size() && !shim::same_particles(with, without));
  check("scenery_shim_alone_is_the_static_collider", shim::same_particles(with, asCollider));
  check("scenery_shim_clear_is_off", shim::same_particles(cleared, without));
  check("scenery_shim_beside_a_collider", both.size() == with.size() && !shim::same_particles(both, with));
  const pbf_collider_wrench w = f.colliderReaction();  // (the pair turned the records on)
  check("scenery_shim_reaction_is_on", w.step == uint64_t(frames), "step %llu", static_cast<unsigned long long>(w.step));

  // one point under the plane, one far above it
  const std::vector<double> points = {c[0], floorY - 0.5 * spacing, c[2], c[0], floorY + 3.0 * spacing, c[2]};
  std::vector<N> phi, moved;
  std::vector<uint8_t> hit;
  a.sampleScenery(config, points, phi, moved, hit);
  check("scenery_shim_sample", hit.size() == 2 && hit[0] == 1 && hit[1] == 0 && phi[0] < N(0) && phi[1] > N(0) &&
                                   double(moved[1]) * double(config.scale) > floorY, "hit %d %d phi %g %g", int(hit[0]), int(hit[1]),
        double(phi[0]), double(phi[1]));
  return shim::finish();
}
