// test_collider_pose_shim.cpp — sph::hip_impl::Solver::setColliderPose() / clearColliderPose() / enableColliderReaction() /
// colliderReaction() through advance().
//   test_collider_pose_shim <lattice file> <dump file> <frames>
// reads a lattice {uint32 dims[3], double origin[3], double spacing, double margin, float phi[dims product]}, runs the
// two-cube scene through advance() for <frames> frames with that collider under a pose that changes every frame — a turn
// about z by 0.04 rad per frame about the box's centre, carried along (3, -2, 1) per frame — and the reaction on, and writes
// {uint64 n; then twice — the scene as built, the state after the last frame — id u64[n], type u8[n], mass f32[n],
// position f32[3n], velocity f32[3n], colour f32[4n]; then per frame double rot[9], trans[3] and the pbf_collider_wrench}.
// tests/test_collider_pose_gpu.py makes the lattice, runs this on a GPU and holds the dump to the same frames with the same
// poses over the C ABI, bit for bit.  Also checked here: the pose changes the result, the collider pushes (hits > 0 in some
// frame), clearColliderPose() gives the static collider's run, and the refused calls throw.  Prints "ok <name>" /
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

static void pose_of(int frame, std::array<double, 9> &rot, std::array<double, 3> &trans) {
  const double a = 0.04 * frame, c = std::cos(a), s = std::sin(a), p[3] = {500, 500, 500};
  rot = {c, -s, 0, s, c, 0, 0, 0, 1};
  const double v[3] = {3.0 * frame, -2.0 * frame, 1.0 * frame};
  for (size_t k = 0; k < 3; ++k) trans[k] = (p[k] - ((rot[3 * k] * p[0] + rot[3 * k + 1] * p[1]) + rot[3 * k + 2] * p[2])) + v[k];
}

int main(int argc, char **argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: test_collider_pose_shim <lattice file> <dump file> <frames>\n");
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
  std::vector<P> posed = particles, fixed = particles, cleared = particles;

  sph::hip_impl::Solver<T, N> a(N(0.1)), b(N(0.1)), c(N(0.1));
  bool threw = false;
  try {
    std::array<double, 9> rot;
    std::array<double, 3> trans;
    pose_of(1, rot, trans);
    a.setColliderPose(rot, trans);  // (no collider yet)
  } catch (const std::exception &) {
    threw = true;
  }
  check("collider_pose_shim_refused_without_a_collider", threw);
  a.setCollider(dims, origin, spacing, margin, phi.data()).enableColliderReaction();
  b.setCollider(dims, origin, spacing, margin, phi.data());
  c.setCollider(dims, origin, spacing, margin, phi.data());
  threw = false;
  try {
    (void)b.colliderReaction();  // (not enabled)
  } catch (const std::exception &) {
    threw = true;
  }
  check("collider_pose_shim_reaction_refused_when_off", threw);
  threw = false;
  try {
    a.setColliderPose({1, 0, 0, 0, 1, 0, 0, 0, -1}, {0, 0, 0});  // (a reflection)
  } catch (const std::exception &) {
    threw = true;
  }
  check("collider_pose_shim_reflection_refused", threw);

  std::vector<std::array<double, 9>> rots;
  std::vector<std::array<double, 3>> transs;
  std::vector<pbf_collider_wrench> wrenches;
  uint64_t hits = 0;
  for (int k = 0; k < frames; ++k) {
    std::array<double, 9> rot;
    std::array<double, 3> trans;
    pose_of(k, rot, trans);
    a.setColliderPose(rot, trans);
    (void)a.advance(config, scene, posed);
    const pbf_collider_wrench w = a.colliderReaction();
    rots.push_back(rot), transs.push_back(trans), wrenches.push_back(w);
    hits += w.hits;
    (void)b.advance(config, scene, fixed);
    c.setColliderPose(rot, trans).clearColliderPose();
    (void)c.advance(config, scene, cleared);
  }
  check("collider_pose_shim_changes_the_run", posed.size() == fixed.size() && !shim::same_particles(posed, fixed));
  check("collider_pose_shim_clear_is_static", shim::same_particles(cleared, fixed));
  check("collider_pose_shim_pushes", hits > 0);
  check("collider_pose_shim_serial", !wrenches.empty() && wrenches.back().step == uint64_t(frames));

  std::FILE *f = std::fopen(argv[2], "wb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[2]);
    return 2;
  }
  const uint64_t n = particles.size();
  check("collider_pose_shim_count", posed.size() == n);
  std::fwrite(&n, 8, 1, f);
  write_particles(f, particles);
  write_particles(f, posed);
  for (size_t k = 0; k < wrenches.size(); ++k) {
    std::fwrite(rots[k].data(), 8, 9, f);
    std::fwrite(transs[k].data(), 8, 3, f);
    std::fwrite(&wrenches[k], sizeof(pbf_collider_wrench), 1, f);
  }
  std::fclose(f);
  return shim::finish();
}
