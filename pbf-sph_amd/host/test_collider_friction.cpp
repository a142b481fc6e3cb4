// test_collider_friction — the host-side text of the collider friction: the argument check of pbf_set_collider_friction
// (csrc/pbf_collider_friction.hpp) and colliderbody::kick() (csrc/pbf_collider_body.hpp) in front of the very advance()
// k_body_kick_advance runs.  No HIP, not linked against the library.
//
// The check: "refuse <name>: <reason>" per refused argument and "ok / FAIL <name>" lines.
//
// The sequences: every input and output is printed as the 64-bit words of the doubles, so that
// tests/test_collider_friction_cpu.py can run tests/collider_friction_ref.py on the same inputs and compare bit for bit:
//   case <name> <dt> <the 40 words of the pbf_collider_body>
//   kick <P.xyz L.xyz>                          the friction sums handed to one kick (absent in a step without pending sums)
//   sums <P.xyz L.xyz> <hits>                   the reaction sums handed to the advance that follows
//   state <the 31 words of the pbf_collider_body_state after it>
// The cases: a kick before every advance under a generic pose, a kick in every other step (the pending word), frozen axes,
// a pure linear and a pure angular impulse, and friction sums that hold a NaN or an infinity.  Prints "ALL OK"; exit status 0
// iff all ok.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "pbf_collider_friction.hpp"
#include "shim_check.hpp"

using shim::check;

namespace {

const double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();

pbf_collider_pose rodrigues(double x, double y, double z, double angle) {
  const double n = std::sqrt(x * x + y * y + z * z);
  const double k[3] = {x / n, y / n, z / n}, c = std::cos(angle), s = std::sin(angle);
  const double K[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
  pbf_collider_pose p{};
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double kk = 0;
      for (int m = 0; m < 3; ++m) kk += K[3 * a + m] * K[3 * m + b];
      p.rot[3 * a + b] = (a == b ? 1.0 : 0.0) + s * K[3 * a + b] + (1 - c) * kk;
    }
  return p;
}

pbf_collider_body stock() {
  pbf_collider_body b{};
  b.mass = 3.5, b.inertia[0] = 900, b.inertia[1] = 1400, b.inertia[2] = 2100, b.gain = 0.49;
  for (int a = 0; a < 3; ++a) b.linear_factor[a] = b.angular_factor[a] = 1.0, b.centre_min[a] = -kInf, b.centre_max[a] = kInf;
  b.pose = rodrigues(0.3, -0.5, 0.8, 0.7);
  b.pose.trans[0] = 420, b.pose.trans[1] = 310, b.pose.trans[2] = 555;
  b.accel[1] = 9800, b.linear_damping = 0.3, b.angular_damping = 1.1;
  b.velocity[0] = 30, b.velocity[2] = -12, b.angular_velocity[0] = 0.4, b.angular_velocity[1] = -0.9, b.angular_velocity[2] = 0.2;
  return b;
}

void words(const void *p, size_t bytes) {
  for (size_t k = 0; k < bytes / 8; ++k) {
    uint64_t w;
    std::memcpy(&w, static_cast<const char *>(p) + 8 * k, 8);
    std::printf(" %016" PRIx64, w);
  }
}

uint64_t lcg = 0x9E3779B97F4A7C15ull;
double uniform() {  // in [-1, 1)
  lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
  return double(int64_t(lcg >> 11) - (int64_t(1) << 52)) / double(int64_t(1) << 52);
}

// `steps` kick + advance pairs.  kicks: 1 = a kick before every advance, 2 = before every other one, 3 = as 1 with a NaN in
// step 2 and an infinity in step 4, 4 = a pure linear impulse, 5 = a pure angular impulse; the reaction sums are pseudo-random
void run(const char *name, const pbf_collider_body &b, double dt, int steps, int kicks) {
  std::printf("case %s", name);
  words(&dt, 8);
  words(&b, sizeof b);
  std::printf("\n");
  colliderbody::Record r = colliderbody::record_of(b);
  for (int k = 0; k < steps; ++k) {
    double f[6], s[6];
    for (int a = 0; a < 3; ++a) f[a] = 40.0 * uniform(), f[3 + a] = 9000.0 * uniform();
    for (int a = 0; a < 3; ++a) s[a] = 0.02 * uniform(), s[3 + a] = 4.0 * uniform();
    if (kicks == 3 && k == 2) f[1] = kNaN;
    if (kicks == 3 && k == 4) f[5] = -kInf;
    if (kicks == 4) f[3] = f[4] = f[5] = 0.0;
    if (kicks == 5) f[0] = f[1] = f[2] = 0.0;
    if (kicks != 2 || k % 2 == 0) {
      colliderbody::kick(r.par, r.st, f, f + 3);
      std::printf("kick");
      words(f, sizeof f);
      std::printf("\n");
    }
    const uint64_t hits = 17 + uint64_t(k);
    colliderbody::advance(r.par, r.st, dt, s, s + 3, hits);
    std::printf("sums");
    words(s, sizeof s);
    std::printf(" %" PRIu64 "\n", hits);
    std::printf("state");
    words(&r.st, sizeof r.st);
    std::printf("\n");
  }
}

pbf_collider_friction friction(double mu) {
  pbf_collider_friction f{};
  f.mu = mu, f.velocity[0] = 30, f.velocity[1] = -5, f.angular_velocity[2] = 1.5;
  return f;
}

void refused(const char *name, const pbf_collider_friction &f, const char *reason) {
  const char *why = nullptr;
  const int rc = colliderfriction::check(&f, &why);
  std::printf("refuse %s: %s\n", name, why ? why : "(accepted)");
  check(std::string("refused ") + name,
        rc == PBF_ERR_INVALID && why && std::strstr(why, reason) && colliderfriction::check(&f, nullptr) == PBF_ERR_INVALID);
}

}  // namespace

int main() {
  static_assert(sizeof(pbf_collider_friction) == 7 * 8, "seven doubles");
  const double dt = double(0.0083f);
  // ---- the check ----
  {
    const char *why = nullptr;
    pbf_collider_friction f = friction(0.4);
    check("accepted stock", colliderfriction::check(&f, &why) == PBF_OK && why == nullptr);
    f = friction(kInf);
    check("accepted mu = inf", colliderfriction::check(&f, &why) == PBF_OK && why == nullptr);
    f = friction(5e-324);
    check("accepted a denormal mu", colliderfriction::check(&f, &why) == PBF_OK && why == nullptr);
  }
  {
    pbf_collider_friction f = friction(0.0);
    refused("zero mu", f, "mu <= 0 or NaN");
    f = friction(-0.3);
    refused("negative mu", f, "mu <= 0 or NaN");
    f = friction(kNaN);
    refused("NaN mu", f, "mu <= 0 or NaN");
    f = friction(-kInf);
    refused("mu = -inf", f, "mu <= 0 or NaN");
    f = friction(0.4), f.velocity[1] = kInf;
    refused("infinite velocity", f, "non-finite velocity");
    f = friction(0.4), f.velocity[2] = kNaN;
    refused("NaN velocity", f, "non-finite velocity");
    f = friction(0.4), f.angular_velocity[0] = -kInf;
    refused("infinite angular velocity", f, "non-finite velocity");
    f = friction(0.4), f.angular_velocity[2] = kNaN;
    refused("NaN angular velocity", f, "non-finite velocity");
  }
  // ---- the sequences ----
  const pbf_collider_body b = stock();
  run("kick-every-step", b, dt, 24, 1);
  run("kick-every-other-step", b, dt, 12, 2);
  pbf_collider_body f = b;
  f.linear_factor[0] = f.linear_factor[2] = 0, f.angular_factor[1] = 0;
  run("frozen-axes", f, dt, 12, 1);
  run("rejected-kicks", b, dt, 8, 3);
  run("linear-only", b, dt, 6, 4);
  run("angular-only", b, dt, 6, 5);
  return shim::finish();
}
