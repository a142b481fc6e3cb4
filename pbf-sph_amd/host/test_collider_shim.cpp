// test_collider_shim.cpp — sph::hip_impl::Solver::setCollider() / clearCollider() through advance().
//   test_collider_shim <lattice file> <dump file> <frames>
// reads a lattice {uint32 dims[3], double origin[3], double spacing, double margin, float phi[dims product]}, runs the
// two-cube scene through advance() for <frames> frames with that collider and writes {uint64 n; then twice — the scene as
// built, the state after the last frame — id u64[n], type u8[n], mass f32[n], position f32[3n], velocity f32[3n], colour
// f32[4n]}.  tests/test_collider_gpu.py makes the lattice, runs this on a GPU and holds the dump to the same frames over the
// C ABI, bit for bit.  Also checked here: the collider changes the result, and clearCollider() gives the run that never
// had one.  Prints "ok <name>" / "FAIL <name>" lines and "ALL OK".
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
    std::fprintf(stderr, "usage: test_collider_shim <lattice file> <dump file> <frames>\n");
    return 2;
  }
  std::array<uint32_t, 3> dims{};
  std::array<double, 3> origin{};
  double spacing = 0, margin = 0;
  std::vector<N> phi;
  {
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
      std::fprintf(stderr, "cannot open %s\n", argv[1]);
      return 2;
    }
    bool ok = std::fread(dims.data(), 4, 3, f) == 3 && std::fread(origin.data(), 8, 3, f) == 3 && std::fread(&spacing, 8, 1, f) == 1 &&
              std::fread(&margin, 8, 1, f) == 1;
    const size_t nodes = ok ? size_t(dims[0]) * dims[1] * dims[2] : 0;
    ok = ok && nodes > 0 && nodes < (size_t(1) << 24);
    if (ok) {
      phi.resize(nodes);
      ok = std::fread(phi.data(), sizeof(N), nodes, f) == nodes;
    }
    std::fclose(f);
    if (!ok) {
      std::fprintf(stderr, "malformed lattice file %s\n", argv[1]);
      return 2;
    }
  }
  const int frames = std::atoi(argv[3]);

  auto [mc, config, particles] = sph::simpleConfigWith2Cubes<T, N, sph::vec>(2048, 4, N(500));
  (void)mc;
  const sph::Scene<T, N, sph::vec> scene{};
  std::vector<P> with = particles, without = particles, cleared = particles;

  sph::hip_impl::Solver<T, N> a(N(0.1)), b(N(0.1)), c(N(0.1));
  a.setCollider(dims, origin, spacing, margin, phi.data());
  c.setCollider(dims, origin, spacing, margin, phi.data()).clearCollider();
  for (int k = 0; k < frames; ++k) {
    (void)a.advance(config, scene, with);
    (void)b.advance(config, scene, without);
    (void)c.advance(config, scene, cleared);
  }
  check("collider_shim_changes_the_run", with.size() == without.size() && !shim::same_particles(with, without));
  check("collider_shim_clear_is_off", shim::same_particles(cleared, without));

  std::FILE *f = std::fopen(argv[2], "wb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[2]);
    return 2;
  }
  const uint64_t n = particles.size();
  check("collider_shim_count", with.size() == n);
  std::fwrite(&n, 8, 1, f);
  write_particles(f, particles);
  write_particles(f, with);
  std::fclose(f);
  return shim::finish();
}
