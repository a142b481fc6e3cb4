// test_diag_shim.cpp — sph::hip_impl::Solver::diagnostics() against sums formed on the host from download(): the shim
// hands the library's record through unchanged, refuses the density part before a step, and a call between two steps
// leaves the next step's result alone.  Prints "ok <name>" / "FAIL <name>" lines and "ALL OK";
// tests/test_diagnostics_gpu.py runs it on a GPU.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "hipsph.hpp"
#include "shim_check.hpp"

using T = size_t;
using N = float;
using P = sph::Particle<T, N, sph::vec>;

using shim::check;
static bool close(double a, double b, double scale) { return std::fabs(a - b) <= 1e-12 * scale; }

int main() {
  auto [mc, config, particles] = sph::simpleConfigWith2Cubes<T, N, sph::vec>(2048, 2, N(500));
  (void)mc;
  particles[7].type = sph::Type::Obstacle;

  sph::hip_impl::Solver<T, N> a(N(0.1)), b(N(0.1));
  a.upload(particles), b.upload(particles);
  bool refused = false;
  try {
    (void)a.diagnostics(config, true);
  } catch (const std::exception &e) {
    refused = std::strstr(e.what(), "pbf_diagnostics") != nullptr;
  }
  check("diag_shim_density_needs_a_step", refused);

  a.step(config), b.step(config);
  const auto d = a.diagnostics(config, true);
  std::vector<P> xs;
  a.download(xs);
  double mass = 0, abs = 0, mom[3] = {0, 0, 0}, kin = 0, top = 0;
  uint64_t fluid = 0, obstacles = 0;
  for (const P &x : xs) {
    if (x.type == sph::Type::Obstacle) {
      ++obstacles;
      continue;
    }
    const double m = x.mass, vx = x.velocity.x, vy = x.velocity.y, vz = x.velocity.z, v2 = vx * vx + vy * vy + vz * vz;
    ++fluid, mass += m, kin += 0.5 * m * v2, top = std::fmax(top, v2);
    mom[0] += m * vx, mom[1] += m * vy, mom[2] += m * vz;
    abs += m * (std::fabs(vx) + std::fabs(vy) + std::fabs(vz));
  }
  check("diag_shim_counts", d.fluid == fluid && d.obstacles == obstacles && d.nonFinite == 0 && d.densityParticles == fluid);
  check("diag_shim_sums", close(d.mass, mass, mass) && close(d.kinetic, kin, kin) && close(d.momentum[0], mom[0], abs) &&
                              close(d.momentum[1], mom[1], abs) && close(d.momentum[2], mom[2], abs));
  check("diag_shim_max_speed", close(d.maxSpeed, std::sqrt(top), std::sqrt(top)));
  check("diag_shim_density", d.rhoMin > 0 && d.rhoMin <= d.rhoMean && d.rhoMean <= d.rhoMax && d.nbrMax >= 1 &&
                                 d.nbrMean > 0 && d.errMax >= d.errMean && d.errMean >= d.compressionMean);

  // the observer changes nothing: one more step on both, the one that was asked in between included
  a.step(config), b.step(config);
  std::vector<P> ya, yb;
  a.download(ya), b.download(yb);
  check("diag_shim_observer", shim::same_particles(ya, yb));

  return shim::finish();
}
