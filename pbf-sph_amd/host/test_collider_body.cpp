// test_collider_body — csrc/pbf_collider_body.hpp on the host: the parameter check of pbf_set_collider_body and the very
// advance() k_body_advance runs.  No HIP, not linked against the library.
//
// The check: "refuse <name>: <reason>" per refused body and "ok / FAIL <name>" lines (a refused body must come with its
// reason, an accepted one with none).
//
// The advance: sequences whose every input and output is printed as the 64-bit words of the doubles, so that
// tests/test_collider_body_cpu.py can run tests/collider_body_ref.py on the same inputs and compare bit for bit:
//   case <name> <dt> <the 40 words of the pbf_collider_body>
//   sums <P.xyz L.xyz> <hits>                   the sums handed to one advance
//   state <the 31 words of the pbf_collider_body_state after it>
// The cases: free fall, a spin about a principal axis, a generic tumble under pseudo-random sums (dampings, a tilted start
// pose from each branch of the matrix -> quaternion conversion), frozen axes, centre bounds that clamp, and sums that hold a
// NaN or overflow the impulse.  Prints "ALL OK"; exit status 0 iff all ok.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "pbf_collider_body.hpp"
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

// `steps` advances; sums: 0 = zeros, 1 = pseudo-random, 2 = pseudo-random with a NaN in step 3 and an overflow in step 5
void run(const char *name, const pbf_collider_body &b, double dt, int steps, int sums) {
  std::printf("case %s", name);
  words(&dt, 8);
  words(&b, sizeof b);
  std::printf("\n");
  colliderbody::Record r = colliderbody::record_of(b);
  for (int k = 0; k < steps; ++k) {
    double s[6] = {0, 0, 0, 0, 0, 0};
    uint64_t hits = 0;
    if (sums) {
      for (int a = 0; a < 3; ++a) s[a] = 0.02 * uniform(), s[3 + a] = 4.0 * uniform();
      hits = 17 + uint64_t(k);
      if (sums == 2 && k == 3) s[4] = kNaN;
      if (sums == 2 && k == 5) s[0] = 1e308;
    }
    colliderbody::advance(r.par, r.st, dt, s, s + 3, hits);
    std::printf("sums");
    words(s, sizeof s);
    std::printf(" %" PRIu64 "\n", hits);
    std::printf("state");
    words(&r.st, sizeof r.st);
    std::printf("\n");
  }
}

void refused(const char *name, const pbf_collider_body &b, const char *reason) {
  const char *why = nullptr;
  const int rc = colliderbody::check(&b, &why);
  std::printf("refuse %s: %s\n", name, why ? why : "(accepted)");
  check(std::string("refused ") + name,
        rc == PBF_ERR_INVALID && why && std::strstr(why, reason) && colliderbody::check(&b, nullptr) == PBF_ERR_INVALID);
}

}  // namespace

int main() {
  static_assert(sizeof(pbf_collider_body) == 40 * 8 && sizeof(struct pbf_collider_body_state) == 31 * 8, "doubles and 64-bit counters");
  const double dt = double(0.0083f);
  // ---- the check ----
  {
    const char *why = nullptr;
    pbf_collider_body b = stock();
    check("accepted stock", colliderbody::check(&b, &why) == PBF_OK && why == nullptr);
    b.centre_min[1] = 100, b.centre_max[1] = 100, b.linear_factor[0] = 0, b.angular_factor[2] = 0, b.gain = 0, b.linear_damping = 0;
    check("accepted equal bounds, zero factors, zero gain", colliderbody::check(&b, &why) == PBF_OK && why == nullptr);
  }
  const double bad[3] = {kNaN, kInf, -kInf};
  bool all = true;
  for (double v : bad)
    for (int k = 0; k < 16; ++k) {  // every parameter before the centre bounds
      pbf_collider_body b = stock();
      (&b.mass)[k] = v;
      const char *why = nullptr;
      all = all && colliderbody::check(&b, &why) == PBF_ERR_INVALID && why && std::strstr(why, "non-finite parameter");
    }
  check("refused a non-finite parameter anywhere", all);
  {
    pbf_collider_body b = stock();
    b.mass = kNaN;
    refused("non-finite mass", b, "non-finite parameter");
    b = stock(), b.centre_max[2] = kNaN;
    refused("NaN centre bound", b, "non-finite parameter");
    b = stock(), b.angular_velocity[1] = kInf;
    refused("non-finite start velocity", b, "non-finite start velocity");
    b = stock(), b.mass = 0;
    refused("zero mass", b, "mass <= 0");
    b = stock(), b.mass = -1;
    refused("negative mass", b, "mass <= 0");
    b = stock(), b.inertia[1] = 0;
    refused("zero inertia", b, "inertia <= 0");
    b = stock(), b.gain = -0.1;
    refused("negative gain", b, "gain < 0");
    b = stock(), b.linear_damping = -1e-9;
    refused("negative linear damping", b, "damping < 0");
    b = stock(), b.angular_damping = -2;
    refused("negative angular damping", b, "damping < 0");
    b = stock(), b.linear_factor[2] = 0.5;
    refused("linear factor 0.5", b, "factor other than 0 or 1");
    b = stock(), b.angular_factor[0] = -1;
    refused("angular factor -1", b, "factor other than 0 or 1");
    b = stock(), b.centre_min[0] = 5, b.centre_max[0] = 4;
    refused("centre_min > centre_max", b, "centre_min > centre_max");
    b = stock(), b.pose.rot[8] = -b.pose.rot[8], b.pose.rot[6] = -b.pose.rot[6], b.pose.rot[7] = -b.pose.rot[7];
    refused("reflected start pose", b, "det rot < 0");
    b = stock(), b.pose.rot[1] += 1e-4;
    refused("sheared start pose", b, "not a rotation");
    b = stock(), b.pose.trans[0] = kInf;
    refused("non-finite start centre", b, "non-finite entry in trans");
  }
  {
    pbf_collider_body b = stock();
    b.centre_min[0] = -kInf, b.centre_max[0] = kInf;
    const char *why = nullptr;
    check("accepted infinite centre bounds", colliderbody::check(&b, &why) == PBF_OK);
  }
  // ---- the conversion: R(q(R)) = R within a few eps on every branch ----
  {
    const double turns[4][4] = {{0.3, -0.5, 0.8, 0.7}, {1, 0.1, -0.05, 3.0}, {0.1, 1, 0.07, 3.1}, {-0.06, 0.1, 1, 2.9}};
    bool ok = true;
    for (const auto &t : turns) {
      const pbf_collider_pose p = rodrigues(t[0], t[1], t[2], t[3]);
      double q[4], r[9];
      colliderbody::quaternion_of(p.rot, q), colliderbody::rotation_of(q, r);
      for (int k = 0; k < 9; ++k) ok = ok && std::fabs(r[k] - p.rot[k]) < 1e-14;
    }
    check("quaternion_of inverts rotation_of on every branch", ok);
  }
  // ---- the sequences ----
  pbf_collider_body b = stock();
  b.accel[1] = 9800;
  run("free-fall", b, dt, 40, 0);
  b = stock();
  for (int k = 0; k < 9; ++k) b.pose.rot[k] = (k % 4 == 0) ? 1.0 : 0.0;
  b.angular_velocity[2] = 1.7;
  run("spin-z", b, dt, 40, 0);
  b = stock();
  b.accel[1] = 9800, b.linear_damping = 0.3, b.angular_damping = 1.1;
  b.velocity[0] = 30, b.velocity[2] = -12, b.angular_velocity[0] = 0.4, b.angular_velocity[1] = -0.9, b.angular_velocity[2] = 0.2;
  run("tumble", b, dt, 24, 1);
  const double turns[3][4] = {{1, 0.1, -0.05, 3.0}, {0.1, 1, 0.07, 3.1}, {-0.06, 0.1, 1, 2.9}};
  for (int k = 0; k < 3; ++k) {
    pbf_collider_body c = b;
    const pbf_collider_pose p = rodrigues(turns[k][0], turns[k][1], turns[k][2], turns[k][3]);
    for (int m = 0; m < 9; ++m) c.pose.rot[m] = p.rot[m];
    run(("tumble-branch" + std::to_string(k + 1)).c_str(), c, dt, 6, 1);
  }
  pbf_collider_body f = b;
  f.linear_factor[0] = f.linear_factor[2] = 0, f.angular_factor[1] = 0;
  run("frozen-axes", f, dt, 12, 1);
  pbf_collider_body c = b;
  c.centre_max[1] = 316, c.centre_min[0] = 418.5;
  c.velocity[0] = -60;
  run("clamped", c, dt, 16, 1);
  run("rejected-sums", b, dt, 8, 2);
  return shim::finish();
}
