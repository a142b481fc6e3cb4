// test_collider_mesh_shim.cpp — sph::hip_impl::Solver::setColliderMesh() through advance().
//   test_collider_mesh_shim <mesh file> <dump file> <frames>
// reads {uint32 dims[3], double origin[3], double spacing, double margin, uint32 negate, uint32 nv, uint32 nt, double
// vertices[3 nv], uint32 triangles[3 nt]}, runs the two-cube scene through advance() for <frames> frames with the collider
// built from that mesh and writes the dump of test_collider_shim: {uint64 n; then twice — the scene as built, the state after
// the last frame — id, type, mass, position, velocity, colour}.  tests/test_mesh_sdf_gpu.py writes the mesh, runs this on a GPU
// and holds the dump to the same frames over the C ABI, bit for bit.  Also checked here: the collider changes the result, the
// pair counts are reported, and clearCollider() gives the run that never had one.
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
    std::fprintf(stderr, "usage: test_collider_mesh_shim <mesh file> <dump file> <frames>\n");
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
  std::vector<P> with = particles, without = particles, cleared = particles;

  sph::hip_impl::Solver<T, N> a(N(0.1)), b(N(0.1)), c(N(0.1));
  pbf_mesh_sdf_stats stats{};
  a.setColliderMesh(vertices, triangles, dims, origin, spacing, margin, negate != 0, &stats);
  c.setColliderMesh(vertices, triangles, dims, origin, spacing, margin, negate != 0).clearCollider();
  check("collider_mesh_shim_pairs", stats.pairs_total == uint64_t(dims[0]) * dims[1] * dims[2] * nt && stats.pairs_tested > 0 &&
                                        stats.pairs_tested <= stats.pairs_total);
  bool refused = false;
  try {  // an open mesh is refused and the collider stays
    std::vector<uint32_t> open(triangles.begin(), triangles.end() - 3);
    a.setColliderMesh(vertices, open, dims, origin, spacing, margin, negate != 0);
  } catch (const std::runtime_error &) {
    refused = true;
  }
  check("collider_mesh_shim_refuses_an_open_mesh", refused);
  for (int k = 0; k < frames; ++k) {
    (void)a.advance(config, scene, with);
    (void)b.advance(config, scene, without);
    (void)c.advance(config, scene, cleared);
  }
  check("collider_mesh_shim_changes_the_run", with.size() == without.size() && !shim::same_particles(with, without));
  check("collider_mesh_shim_clear_is_off", shim::same_particles(cleared, without));

  std::FILE *f = std::fopen(argv[2], "wb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[2]);
    return 2;
  }
  const uint64_t n = particles.size();
  check("collider_mesh_shim_count", with.size() == n);
  std::fwrite(&n, 8, 1, f);
  write_particles(f, particles);
  write_particles(f, with);
  std::fclose(f);
  return shim::finish();
}
