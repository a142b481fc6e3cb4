// test_scene_shim.cpp — the whole sph::Scene on the device-resident path of sph::hip_impl::Solver: upload() once, then
// step(config, scene, n) + download() and the public query() must equal n x advance() on the same scene (sources, a
// drain, an obstacle, queries; reference behaviour: src/omp/ompsph.hpp:91-126,167-186) — the same particles in the
// same order with the same bytes, the same query answers.  Prints "ok <name>" / "FAIL <name>" lines and "ALL OK";
// tests/test_scene_resident_gpu.py runs it on a GPU.
#include "hipsph.hpp"
#include "shim_check.hpp"

using T = size_t;
using N = float;
using P = sph::Particle<T, N, sph::vec>;
using V3 = sph::vec<3, N>;
using V4 = sph::vec<4, N>;

using shim::check;

int main() {
  auto [mc, config, particles] = sph::simpleConfigWith2Cubes<T, N, sph::vec>(2048, 4, N(500));
  (void)mc;
  particles[7].type = sph::Type::Obstacle;
  sph::Scene<T, N, sph::vec> scene;
  scene.sources.push_back({T(100777), V3(500, 300, 500), V3(0, 1, 0), V4(1, 0, 0, 1), N(16)});
  scene.sources.push_back({T(100888), V3(200, 700, 800), V3(3, 0, -2), V4(0, 1, 0, 1), N(10)});
  scene.drains.push_back({T(1), particles[7].position, N(60), N(0)});
  scene.queries.push_back({T(5), particles[100].position});
  scene.queries.push_back({T(6), V3(990, 990, 990)});
  scene.queries.push_back({T(7), V3(510, 310, 510)});
  const uint32_t frames = 4;

  sph::hip_impl::Solver<T, N> host(N(0.1));
  auto xs = particles;
  sph::Result<T, N, sph::vec> last;
  for (uint32_t f = 0; f < frames; ++f) last = host.advance(config, scene, xs);

  sph::hip_impl::Solver<T, N> resident(N(0.1));
  resident.reserve(particles.size() + frames * 28);
  resident.upload(particles);
  resident.step(config, scene, frames);
  const auto answers = resident.query(config, scene);
  std::vector<P> ys;
  resident.download(ys);
  check("scene_resident_count", resident.count() == xs.size());
  check("scene_resident_equals_advance", shim::same_particles(xs, ys));
  bool q = answers.size() == last.queries.size();
  for (size_t i = 0; q && i < answers.size(); ++i)
    q = answers[i].id == last.queries[i].id && answers[i].neighbours == last.queries[i].neighbours;
  check("scene_resident_queries", q);

  // one step at a time, the scene unchanged in between: nothing is pushed twice, the result is the same
  sph::hip_impl::Solver<T, N> single(N(0.1));
  single.reserve(particles.size() + frames * 28);
  single.upload(particles);
  for (uint32_t f = 0; f < frames; ++f) single.step(config, scene);
  std::vector<P> zs;
  single.download(zs);
  check("scene_resident_stepwise", shim::same_particles(xs, zs));
  // an empty scene clears both settings again
  single.step(config);
  check("scene_resident_cleared", single.count() == zs.size());

  return shim::finish();
}
