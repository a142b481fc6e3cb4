// test_collider_friction_shim.cpp — sph::hip_impl::Solver::setColliderFriction() / clearColliderFriction() /
// colliderFrictionReaction() through advance().
//   test_collider_friction_shim <lattice file> <dump file> <frames>
// reads a lattice {uint32 dims[3], double origin[3], double spacing, double margin, float phi[dims product]} in the frame of
// the pose (identity, (500, 500, 500)), runs the two-cube scene through advance() for <frames> frames with that collider and
// friction mu = 0.5 against a solid that moves with velocity (60, 0, -25) and angular velocity (0.1, -0.2, 0.4), and writes
// {uint64 n; then twice — the scene as built, the state after the last frame — id u64[n], type u8[n], mass f32[n], position
// f32[3n], velocity f32[3n], colour f32[4n]; then per frame the pbf_collider_wrench of the friction pass}.
// tests/test_collider_friction_cli_gpu.py makes the lattice, runs this on a GPU and holds the dump to the same frames over the
// C ABI, bit for bit.  Also checked here: particles slid, clearColliderFriction() gives the frames of a solver that never had
// it, and the refused calls throw.  Prints "ok <name>" / "FAIL <name>" lines and "ALL OK".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

template <typename F> static bool throws(F &&f) {
  try {
    f();
  } catch (const std::exception &) {
    return true;
  }
  return false;
}

int main(int argc, char **argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: test_collider_friction_shim <lattice file> <dump file> <frames>\n");
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
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const std::array<double, 9> eye{1, 0, 0, 0, 1, 0, 0, 0, 1};
  const std::array<double, 3> centre{500, 500, 500}, V{60, 0, -25}, W{0.1, -0.2, 0.4};

  auto [mc, config, particles] = sph::simpleConfigWith2Cubes<T, N, sph::vec>(2048, 4, N(500));
  (void)mc;
  const sph::Scene<T, N, sph::vec> scene{};
  std::vector<P> rubbed = particles;

  sph::hip_impl::Solver<T, N> a(N(0.1)), b(N(0.1));
  check("collider_friction_shim_refused_without_a_collider", throws([&] { a.setColliderFriction(0.5); }));
  a.setCollider(dims, origin, spacing, margin, phi.data()).setColliderPose(eye, centre);
  b.setCollider(dims, origin, spacing, margin, phi.data()).setColliderPose(eye, centre).enableColliderReaction();
  check("collider_friction_shim_reaction_refused_while_off", throws([&] { (void)a.colliderFrictionReaction(); }));
  check("collider_friction_shim_zero_mu_refused", throws([&] { a.setColliderFriction(0.0); }));
  check("collider_friction_shim_nan_mu_refused", throws([&] { a.setColliderFriction(nan); }));
  check("collider_friction_shim_infinite_velocity_refused", throws([&] { a.setColliderFriction(0.5, {inf, 0, 0}); }));
  a.setColliderFriction(inf);  // (no-slip is accepted; the next call rewrites the record)
  a.setColliderFriction(0.5, V, W);
  check("collider_friction_shim_reaction_refused_before_a_step", throws([&] { (void)a.colliderFrictionReaction(); }));

  std::vector<pbf_collider_wrench> sums;
  uint64_t slid = 0;
  for (int k = 0; k < frames; ++k) {
    (void)a.advance(config, scene, rubbed);
    sums.push_back(a.colliderFrictionReaction());
    slid += sums.back().hits;
  }
  check("collider_friction_shim_slid", slid > 0);
  check("collider_friction_shim_passes", !sums.empty() && sums.back().step == uint64_t(frames) && sums.back().hits <= sums.back().particles);

  // clearColliderFriction(): the frames of a solver that only ever had the reaction
  {
    std::vector<P> cleared = rubbed, never = rubbed;
    a.clearColliderFriction();
    (void)a.advance(config, scene, cleared);
    (void)b.advance(config, scene, never);
    check("collider_friction_shim_clear_equals_never_set", shim::same_particles(cleared, never));
    check("collider_friction_shim_reaction_refused_after_clear", throws([&] { (void)a.colliderFrictionReaction(); }));
  }

  std::FILE *f = std::fopen(argv[2], "wb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[2]);
    return 2;
  }
  const uint64_t n = particles.size();
  check("collider_friction_shim_count", rubbed.size() == n);
  std::fwrite(&n, 8, 1, f);
  write_particles(f, particles);
  write_particles(f, rubbed);
  for (const auto &w : sums) std::fwrite(&w, sizeof w, 1, f);
  std::fclose(f);
  return shim::finish();
}
