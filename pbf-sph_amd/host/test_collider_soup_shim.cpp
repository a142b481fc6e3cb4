// test_collider_soup_shim.cpp — sph::hip_impl::Solver::setColliderMesh(..., winding = true) and meshWinding() through advance().
//   test_collider_soup_shim <mesh file> <dump file> <frames>
// reads the mesh file of test_collider_mesh_shim {uint32 dims[3], double origin[3], double spacing, double margin, uint32
// negate, uint32 nv, uint32 nt, double vertices[3 nv], uint32 triangles[3 nt]} — an OPEN mesh here —, runs the two-cube scene
// through advance() for <frames> frames with the collider built from it under the winding-number sign and writes {uint64 n;
// the scene as built and the state after the last frame — id, type, mass, position, velocity, colour —; uint64 nodes; float
// w[nodes], meshWinding()'s field}.  tests/test_mesh_winding_gpu.py writes the mesh, runs this on a GPU and holds the dump to
// the same calls over the C ABI, bit for bit.  Also checked here: without the flag the open mesh is refused and the
// collider stays, the pair counts are reported, the collider changes the result, and w has both sides of 1 / 2.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hipsph.hpp"
#include "shim_check.hpp"

using T = size_t;
using N = float;
using P = sph::Particle<T, N, sph::vec>;

using shim::check;

static void write_particles(std::FILE *f, const std::vector<P> &xs) {
  for (const P &p : xs) {
    const uint64_t id = p.id;
    std::fwrite(&id, 8, 1, f);
  }
  for (const P &p : xs) {
    const uint8_t ty = uint8_t(p.type);
    std::fwrite(&ty, 1, 1, f);
  }
  for (const P &p : xs) std::fwrite(&p.mass, sizeof(N), 1, f);
  for (const P &p : xs) std::fwrite(&p.position, sizeof(N), 3, f);
  for (const P &p : xs) std::fwrite(&p.velocity, sizeof(N), 3, f);
  for (const P &p : xs) std::fwrite(&p.colour, sizeof(N), 4, f);
}

int main(int argc, char **argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: test_collider_soup_shim <mesh file> <dump file> <frames>\n");
    return 2;
  }
  std::array<uint32_t, 3> dims{};
  std::array<double, 3> origin{};
  double spacing = 0, margin = 0;
  uint32_t negate = 0, nv = 0, nt = 0;
  std::vector<double> vertices;
  std::vector<uint32_t> triangles;
  {
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
      std::fprintf(stderr, "cannot open %s\n", argv[1]);
      return 2;
    }
    bool ok = std::fread(dims.data(), 4, 3, f) == 3 && std::fread(origin.data(), 8, 3, f) == 3 && std::fread(&spacing, 8, 1, f) == 1 &&
              std::fread(&margin, 8, 1, f) == 1 && std::fread(&negate, 4, 1, f) == 1 && std::fread(&nv, 4, 1, f) == 1 &&
              std::fread(&nt, 4, 1, f) == 1;
    ok = ok && nv > 0 && nt > 0 && nv < (1u << 24) && nt < (1u << 24);
    if (ok) {
      vertices.resize(3 * size_t(nv)), triangles.resize(3 * size_t(nt));
      ok = std::fread(vertices.data(), 8, vertices.size(), f) == vertices.size() &&
           std::fread(triangles.data(), 4, triangles.size(), f) == triangles.size();
    }
    std::fclose(f);
    if (!ok) {
      std::fprintf(stderr, "malformed mesh file %s\n", argv[1]);
      return 2;
    }
  }
  const int frames = std::atoi(argv[3]);

  auto [mc, config, particles] = sph::simpleConfigWith2Cubes<T, N, sph::vec>(2048, 4, N(500));
  (void)mc;
  const sph::Scene<T, N, sph::vec> scene{};
  std::vector<P> with = particles, without = particles;

  sph::hip_impl::Solver<T, N> a(N(0.1)), b(N(0.1));
  pbf_mesh_sdf_stats stats{};
  a.setColliderMesh(vertices, triangles, dims, origin, spacing, margin, negate != 0, &stats, /*winding=*/true);
  check("collider_soup_shim_pairs", stats.pairs_total == uint64_t(dims[0]) * dims[1] * dims[2] * nt && stats.pairs_tested > 0 &&
                                        stats.pairs_tested <= stats.pairs_total);
  bool refused = false;
  try {  // without the flag the open mesh is refused and the collider stays
    a.setColliderMesh(vertices, triangles, dims, origin, spacing, margin, negate != 0);
  } catch (const std::runtime_error &) {
    refused = true;
  }
  check("collider_soup_shim_refused_without_the_flag", refused);
  const std::vector<N> w = a.meshWinding(vertices, triangles, dims, origin, spacing);
  size_t in = 0, out = 0;
  for (N x : w) in += x > N(0.5), out += x < N(0.5);
  check("collider_soup_shim_winding_field", w.size() == size_t(dims[0]) * dims[1] * dims[2] && in > 0 && out > 0 && in + out == w.size());
  for (int k = 0; k < frames; ++k) {
    (void)a.advance(config, scene, with);
    (void)b.advance(config, scene, without);
  }
  check("collider_soup_shim_changes_the_run", with.size() == without.size() && !shim::same_particles(with, without));

  std::FILE *f = std::fopen(argv[2], "wb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[2]);
    return 2;
  }
  const uint64_t n = particles.size(), nodes = w.size();
  check("collider_soup_shim_count", with.size() == n);
  std::fwrite(&n, 8, 1, f);
  write_particles(f, particles);
  write_particles(f, with);
  std::fwrite(&nodes, 8, 1, f);
  std::fwrite(w.data(), sizeof(N), w.size(), f);
  std::fclose(f);
  return shim::finish();
}
