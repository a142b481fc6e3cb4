// test_collider_body_shim.cpp — sph::hip_impl::Solver::setColliderBody() / clearColliderBody() / colliderBody() through advance().
//   test_collider_body_shim <lattice file> <dump file> <frames>
// reads a lattice {uint32 dims[3], double origin[3], double spacing, double margin, float phi[dims product]} in the body's
// frame, runs the two-cube scene through advance() for <frames> frames with that collider as a body — mass 300, moments
// (3e6, 4e6, 5e6), gain 0.49, accel (0, 200, 0), dampings 0.1 and 0.3, started at the identity at (500, 500, 500) with velocity
// (10, -20, 5) and angular velocity (0.2, 0.1, -0.3) — and writes {uint64 n; then twice — the scene as built, the state after the
// last frame — id u64[n], type u8[n], mass f32[n], position f32[3n], velocity f32[3n], colour f32[4n]; then per frame the
// pbf_collider_body_state}.  tests/test_collider_body_cli_gpu.py makes the lattice, runs this on a GPU and holds the dump to the
// same frames over the C ABI, bit for bit.  Also checked here: the body is touched and moves, clearColliderBody() leaves the
// solid where it is, and the refused calls throw.  Prints "ok <name>" / "FAIL <name>" lines and "ALL OK".
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

static pbf_collider_body the_body() {
  const double inf = std::numeric_limits<double>::infinity();
  pbf_collider_body b{};
  b.mass = 300, b.inertia[0] = 3e6, b.inertia[1] = 4e6, b.inertia[2] = 5e6, b.gain = 0.49;
  b.linear_damping = 0.1, b.angular_damping = 0.3, b.accel[1] = 200;
  for (int a = 0; a < 3; ++a)
    b.linear_factor[a] = b.angular_factor[a] = 1, b.centre_min[a] = -inf, b.centre_max[a] = inf, b.pose.rot[4 * a] = 1, b.pose.trans[a] = 500;
  b.velocity[0] = 10, b.velocity[1] = -20, b.velocity[2] = 5;
  b.angular_velocity[0] = 0.2, b.angular_velocity[1] = 0.1, b.angular_velocity[2] = -0.3;
  return b;
}

int main(int argc, char **argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: test_collider_body_shim <lattice file> <dump file> <frames>\n");
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
  std::vector<P> floating = particles;

  sph::hip_impl::Solver<T, N> a(N(0.1)), b(N(0.1));
  bool threw = false;
  try {
    a.setColliderBody(the_body());  // (no collider yet)
  } catch (const std::exception &) {
    threw = true;
  }
  check("collider_body_shim_refused_without_a_collider", threw);
  a.setCollider(dims, origin, spacing, margin, phi.data());
  b.setCollider(dims, origin, spacing, margin, phi.data());
  threw = false;
  try {
    (void)a.colliderBody();  // (no body yet)
  } catch (const std::exception &) {
    threw = true;
  }
  check("collider_body_shim_state_refused_without_a_body", threw);
  threw = false;
  try {
    pbf_collider_body bad = the_body();
    bad.mass = 0;
    a.setColliderBody(bad);
  } catch (const std::exception &) {
    threw = true;
  }
  check("collider_body_shim_zero_mass_refused", threw);
  a.setColliderBody(the_body());
  threw = false;
  try {
    a.setColliderPose({1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0});  // (the body owns the pose)
  } catch (const std::exception &) {
    threw = true;
  }
  check("collider_body_shim_pose_refused_while_on", threw);

  std::vector<struct pbf_collider_body_state> states;
  uint64_t hits = 0;
  for (int k = 0; k < frames; ++k) {
    (void)a.advance(config, scene, floating);
    states.push_back(a.colliderBody());
    hits += states.back().hits;
  }
  check("collider_body_shim_touched", hits > 0);
  check("collider_body_shim_steps", !states.empty() && states.back().steps == uint64_t(frames) && states.back().rejected == 0);
  check("collider_body_shim_moved", !states.empty() && states.back().pose.trans[1] != 500.0 && states.back().quat[0] != 1.0);

  // clearColliderBody(): the solid stays where the body left it — the same frames as a pose set by hand
  if (!states.empty()) {
    std::array<double, 9> rot;
    std::array<double, 3> trans;
    for (size_t k = 0; k < 9; ++k) rot[k] = states.back().pose.rot[k];
    for (size_t k = 0; k < 3; ++k) trans[k] = states.back().pose.trans[k];
    std::vector<P> left = floating, posed = floating;
    a.clearColliderBody();
    b.setColliderPose(rot, trans).enableColliderReaction();
    (void)a.advance(config, scene, left);
    (void)b.advance(config, scene, posed);
    check("collider_body_shim_clear_leaves_the_pose", shim::same_particles(left, posed));
  }

  std::FILE *f = std::fopen(argv[2], "wb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[2]);
    return 2;
  }
  const uint64_t n = particles.size();
  check("collider_body_shim_count", floating.size() == n);
  std::fwrite(&n, 8, 1, f);
  write_particles(f, particles);
  write_particles(f, floating);
  for (const auto &st : states) std::fwrite(&st, sizeof st, 1, f);
  std::fclose(f);
  return shim::finish();
}
