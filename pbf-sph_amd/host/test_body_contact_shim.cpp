// test_body_contact_shim.cpp — sph::hip_impl::Solver::setColliderBodyContact() / clearColliderBodyContact() /
// colliderBodyContact() / colliderBodyContactPoints() through advance().
//   test_body_contact_shim <collider lattice file> <scenery lattice file> <dump file> <frames>
// reads two lattices {uint32 dims[3], double origin[3], double spacing, double margin, float phi[dims product]} — the collider's
// in the body's frame, the scenery's in the world's —, runs the two-cube scene through advance() for <frames> frames with the
// collider as a body — mass 46, moments 66 240, gain 0.49, accel (0, 4900, 0), started at the identity at (500, 728, 500) with
// velocity (200, 300, -50) and angular velocity (0.5, -0.3, 0.2) — in contact with the scenery — level 0, stride 1, skin 6,
// restitution 0.3, friction 0.4, correction 0.3, slop 0.5, 2 passes per step — and writes {uint64 n, uint64 points; then twice —
// the scene as built, the state after the last frame — id u64[n], type u8[n], mass f32[n], position f32[3n], velocity f32[3n],
// colour f32[4n]; the points f32[3 points]; then per frame the pbf_collider_body_state and the pbf_body_contact_state}.
// tests/test_body_contact_gpu.py makes the lattices, runs this on a GPU and holds the dump to the same frames over the C ABI,
// bit for bit.  Also checked here: the refused calls throw, the body touches the scenery, and clearColliderBodyContact()
// turns the observer off.  Prints "ok <name>" / "FAIL <name>" lines and "ALL OK".
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

struct Lattice {
  std::array<uint32_t, 3> dims{};
  std::array<double, 3> origin{};
  double spacing = 0, margin = 0;
  std::vector<N> phi;
};

static bool read_lattice(const char *path, Lattice &l) {
  std::FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  bool ok = std::fread(l.dims.data(), 4, 3, f) == 3 && std::fread(l.origin.data(), 8, 3, f) == 3 && std::fread(&l.spacing, 8, 1, f) == 1 &&
            std::fread(&l.margin, 8, 1, f) == 1;
  const size_t nodes = ok ? size_t(l.dims[0]) * l.dims[1] * l.dims[2] : 0;
  ok = ok && nodes > 0 && nodes < (size_t(1) << 24);
  if (ok) {
    l.phi.resize(nodes);
    ok = std::fread(l.phi.data(), sizeof(N), nodes, f) == nodes;
  }
  std::fclose(f);
  return ok;
}

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
  b.mass = 46, b.inertia[0] = b.inertia[1] = b.inertia[2] = 66240, b.gain = 0.49, b.accel[1] = 4900;
  for (int a = 0; a < 3; ++a) b.linear_factor[a] = b.angular_factor[a] = 1, b.centre_min[a] = -inf, b.centre_max[a] = inf, b.pose.rot[4 * a] = 1;
  b.pose.trans[0] = 500, b.pose.trans[1] = 728, b.pose.trans[2] = 500;
  b.velocity[0] = 200, b.velocity[1] = 300, b.velocity[2] = -50;
  b.angular_velocity[0] = 0.5, b.angular_velocity[1] = -0.3, b.angular_velocity[2] = 0.2;
  return b;
}

static pbf_body_contact the_contact() {
  pbf_body_contact c{};
  c.level = 0, c.stride = 1, c.skin = 6, c.restitution = 0.3, c.friction = 0.4, c.correction = 0.3, c.slop = 0.5, c.iterations = 2;
  return c;
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
  if (argc != 5) {
    std::fprintf(stderr, "usage: test_body_contact_shim <collider lattice file> <scenery lattice file> <dump file> <frames>\n");
    return 2;
  }
  Lattice body, scenery;
  if (!read_lattice(argv[1], body) || !read_lattice(argv[2], scenery)) {
    std::fprintf(stderr, "cannot read the lattice files\n");
    return 2;
  }
  const int frames = std::atoi(argv[4]);

  auto [mc, config, particles] = sph::simpleConfigWith2Cubes<T, N, sph::vec>(2048, 4, N(500));
  (void)mc;
  const sph::Scene<T, N, sph::vec> scene{};
  std::vector<P> state = particles;

  sph::hip_impl::Solver<T, N> a(N(0.1));
  a.setCollider(body.dims, body.origin, body.spacing, body.margin, body.phi.data());
  check("body_contact_shim_refused_without_a_body", throws([&] { a.setColliderBodyContact(the_contact()); }));
  a.setColliderBody(the_body());
  check("body_contact_shim_refused_without_scenery", throws([&] { a.setColliderBodyContact(the_contact()); }));
  a.setScenery(scenery.dims, scenery.origin, scenery.spacing, scenery.margin, scenery.phi.data());
  check("body_contact_shim_state_refused_while_off", throws([&] { (void)a.colliderBodyContact(); }));
  check("body_contact_shim_bad_restitution_refused", throws([&] {
          pbf_body_contact bad = the_contact();
          bad.restitution = 1.5;
          a.setColliderBodyContact(bad);
        }));
  a.setColliderBodyContact(the_contact());
  const std::vector<N> points = a.colliderBodyContactPoints();
  check("body_contact_shim_points", !points.empty() && points.size() % 3 == 0 && a.colliderBodyContact().points == points.size() / 3);

  std::vector<struct pbf_collider_body_state> bodies;
  std::vector<struct pbf_body_contact_state> contacts;
  for (int k = 0; k < frames; ++k) {
    (void)a.advance(config, scene, state);
    bodies.push_back(a.colliderBody());
    contacts.push_back(a.colliderBodyContact());
  }
  check("body_contact_shim_passes", !contacts.empty() && contacts.back().passes == 2 * uint64_t(frames) && contacts.back().rejected == 0);
  check("body_contact_shim_touched", !contacts.empty() && contacts.back().contacts > 0);
  check("body_contact_shim_held", !bodies.empty() && bodies.back().pose.trans[1] < 800.0);

  std::FILE *f = std::fopen(argv[3], "wb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[3]);
    return 2;
  }
  const uint64_t n = particles.size(), np = points.size() / 3;
  check("body_contact_shim_count", state.size() == n);
  std::fwrite(&n, 8, 1, f);
  std::fwrite(&np, 8, 1, f);
  write_particles(f, particles);
  write_particles(f, state);
  std::fwrite(points.data(), sizeof(N), points.size(), f);
  for (size_t k = 0; k < bodies.size(); ++k) {
    std::fwrite(&bodies[k], sizeof bodies[k], 1, f);
    std::fwrite(&contacts[k], sizeof contacts[k], 1, f);
  }
  std::fclose(f);

  a.clearColliderBodyContact();
  check("body_contact_shim_cleared", throws([&] { (void)a.colliderBodyContact(); }));
  return shim::finish();
}
