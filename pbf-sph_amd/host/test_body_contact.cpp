// test_body_contact — csrc/pbf_body_contact.hpp on the host: the parameter check of pbf_set_collider_body_contact, a walk of
// the mode owner's events, and the very resolve() k_contact_resolve runs.  No HIP, not linked against the library.
//
// The check: "refuse <name>: <reason>" per refused configuration and "ok / FAIL <name>" lines.
// The walk: "ok / FAIL mode ..." lines.
// The response: sequences whose every input and output is printed as the 64-bit words of the doubles, so that
// tests/test_body_contact_cpu.py can run tests/body_contact_ref.py on the same inputs and compare bit for bit:
//   case <name> <the 40 words of the pbf_collider_body> <skin restitution friction correction slop>
//   sums <S M.xyz A.xyz D> <count>              the sums handed to one resolve
//   state <the 31 words of the pbf_collider_body_state after it> <the 18 words of the pbf_body_contact_state>
// The cases: no points; a separating contact (a shift, no impulse); friction that slides and friction that sticks; locked
// linear and angular axes; a centre bound the shift reaches; M = 0; a non-finite sum.  Prints "ALL OK"; exit status 0 iff all ok.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "pbf_body_contact.hpp"
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

// a body on its way down (gravity is +y) and sideways, spinning
pbf_collider_body stock_body() {
  pbf_collider_body b{};
  b.mass = 3.5, b.inertia[0] = 900, b.inertia[1] = 1400, b.inertia[2] = 2100, b.gain = 0.49;
  for (int a = 0; a < 3; ++a) b.linear_factor[a] = b.angular_factor[a] = 1.0, b.centre_min[a] = -kInf, b.centre_max[a] = kInf;
  b.pose = rodrigues(0.3, -0.5, 0.8, 0.7);
  b.pose.trans[0] = 420, b.pose.trans[1] = 310, b.pose.trans[2] = 555;
  b.velocity[0] = 30, b.velocity[1] = 140, b.velocity[2] = -12;
  b.angular_velocity[0] = 0.4, b.angular_velocity[1] = -0.9, b.angular_velocity[2] = 0.2;
  return b;
}
pbf_body_contact stock_contact() {
  pbf_body_contact c{};
  c.level = 0, c.stride = 1, c.skin = 2, c.restitution = 0.5, c.friction = 0, c.correction = 0.8, c.slop = 0.5, c.iterations = 1;
  return c;
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

// a floor below the body (its push is towards -y, slightly tilted), `count` points about `depth` deep around the arm (12, 60, -7)
bodycontact::Sums floor_sums(uint64_t count, double depth) {
  bodycontact::Sums s{};
  s.count = count;
  if (!count) return s;
  s.S = double(count) * depth * (1.0 + 0.05 * uniform());
  s.M[0] = 0.04 * s.S * uniform(), s.M[1] = -s.S * (0.98 + 0.01 * uniform()), s.M[2] = 0.04 * s.S * uniform();
  s.A[0] = s.S * (12.0 + uniform()), s.A[1] = s.S * (60.0 + uniform()), s.A[2] = s.S * (-7.0 + uniform());
  s.D = depth * (1.3 + 0.1 * uniform());
  return s;
}

struct Case {
  colliderbody::Record body;
  bodycontact::Record contact;
};
Case begin(const char *name, const pbf_collider_body &b, const pbf_body_contact &c) {
  Case k{colliderbody::record_of(b), bodycontact::record_of(c, 1234)};
  std::printf("case %s", name);
  words(&b, sizeof b);
  words(&k.contact.par, sizeof k.contact.par);
  std::printf("\n");
  return k;
}
void pass(Case &k, const bodycontact::Sums &s) {
  bodycontact::resolve(k.body.par, k.body.st, k.contact.par, s, k.contact.st);
  std::printf("sums");
  words(&s, 8 * sizeof(double));
  std::printf(" %" PRIu64 "\n", s.count);
  std::printf("state");
  words(&k.body.st, sizeof k.body.st);
  words(&k.contact.st, sizeof k.contact.st);
  std::printf("\n");
}

void refused(const char *name, const pbf_body_contact &c, const char *reason) {
  const char *why = nullptr;
  const int rc = bodycontact::check(&c, &why);
  std::printf("refuse %s: %s\n", name, why ? why : "(accepted)");
  check(std::string("refused ") + name, rc == PBF_ERR_INVALID && why && std::strstr(why, reason) && bodycontact::check(&c, nullptr) == PBF_ERR_INVALID);
}

}  // namespace

int main() {
  static_assert(sizeof(struct pbf_body_contact_state) == 18 * 8 && sizeof(bodycontact::Record) == 23 * 8 &&
                    offsetof(bodycontact::Sums, count) == 8 * sizeof(double),
                "doubles and 64-bit counters");
  // ---- the check ----
  {
    const char *why = nullptr;
    pbf_body_contact c = stock_contact();
    check("accepted stock", bodycontact::check(&c, &why) == PBF_OK && why == nullptr);
    c.skin = 0, c.restitution = 1, c.friction = 0, c.correction = 0, c.slop = 0, c.iterations = 8, c.level = -3;
    check("accepted the ends of every range", bodycontact::check(&c, &why) == PBF_OK && why == nullptr);
    c = stock_contact(), c.level = kNaN;
    refused("non-finite level", c, "non-finite parameter");
    c = stock_contact(), c.friction = kInf;
    refused("infinite friction", c, "non-finite parameter");
    c = stock_contact(), c.stride = 0;
    refused("zero stride", c, "stride < 1");
    c = stock_contact(), c.skin = -1e-9;
    refused("negative skin", c, "skin < 0");
    c = stock_contact(), c.restitution = 1.5;
    refused("restitution 1.5", c, "restitution outside");
    c = stock_contact(), c.restitution = -0.1;
    refused("negative restitution", c, "restitution outside");
    c = stock_contact(), c.friction = -1;
    refused("negative friction", c, "friction < 0");
    c = stock_contact(), c.correction = 1.01;
    refused("correction 1.01", c, "correction outside");
    c = stock_contact(), c.slop = -2;
    refused("negative slop", c, "slop < 0");
    c = stock_contact(), c.iterations = 0;
    refused("zero iterations", c, "iterations outside");
    c = stock_contact(), c.iterations = 9;
    refused("nine iterations", c, "iterations outside");
  }
  // ---- the mode owner: every event from every state it can be in ----
  {
    bodycontact::Mode m;
    check("mode starts off", !m.on && m.points == 0 && m.iterations == 0 && m.gen == 0 && m.launches_per_step() == 0);
    check("mode cleared while off changes nothing", !m.cleared() && m.gen == 0);
    check("mode rewritten while off changes nothing", !m.rewritten(3) && !m.on && m.gen == 0);
    check("mode configured with no point is refused", !m.configured(0, 2, 0.0, 1) && !m.on && m.gen == 0);
    check("mode configured with no pass is refused", !m.configured(10, 0, 0.0, 1) && !m.on && m.gen == 0);
    check("mode off -> on bumps", m.configured(65, 2, 1.5, 2) && m.on && m.points == 65 && m.iterations == 2 && m.gen == 1 &&
                                      m.launches_per_step() == 4);
    check("mode same points asks level and stride", m.same_points(1.5, 2) && !m.same_points(1.5, 1) && !m.same_points(1.0, 2));
    check("mode a rewrite with the same passes keeps the key", !m.rewritten(2) && m.gen == 1 && m.iterations == 2);
    check("mode a rewrite with other passes bumps", m.rewritten(4) && m.gen == 2 && m.iterations == 4 && m.launches_per_step() == 8 &&
                                                        m.points == 65);
    check("mode a rewrite to no pass is refused", !m.rewritten(0) && m.iterations == 4 && m.gen == 2);
    check("mode other points while on bumps", m.configured(1025, 1, 0.0, 1) && m.points == 1025 && m.iterations == 1 && m.gen == 3);
    check("mode on -> off bumps", m.cleared() && !m.on && m.points == 0 && m.iterations == 0 && m.gen == 4 && !m.same_points(0.0, 1));
    check("mode cleared twice bumps once", !m.cleared() && m.gen == 4);
    check("mode on again", m.configured(1, 8, -2.0, 3) && m.on && m.gen == 5 && m.launches_per_step() == 16);
  }
  // ---- the sequences ----
  pbf_collider_body b = stock_body();
  pbf_body_contact c = stock_contact();
  {
    Case k = begin("no-points", b, c);
    for (int p = 0; p < 3; ++p) pass(k, floor_sums(0, 0));
    check("no points: passes alone count", k.contact.st.passes == 3 && k.contact.st.contacts == 0 && k.contact.st.rejected == 0);
  }
  {
    Case k = begin("approaching", b, c);
    for (int p = 0; p < 6; ++p) pass(k, floor_sums(40 + 7 * uint64_t(p), 1.5 + 0.2 * p));
    check("approaching: every pass responded", k.contact.st.contacts == 6);
  }
  {
    pbf_collider_body up = b;
    up.velocity[1] = -140;  // (leaving the floor: un >= 0)
    up.angular_velocity[0] = up.angular_velocity[1] = up.angular_velocity[2] = 0;
    Case k = begin("separating", up, c);
    for (int p = 0; p < 4; ++p) pass(k, floor_sums(30, 1.5));
    bool shifted = true;
    for (int a = 0; a < 3; ++a) shifted = shifted && k.contact.st.impulse[a] == 0.0;
    check("separating: a shift and no impulse", shifted && k.contact.st.shift[1] < 0 && k.body.st.velocity[1] == -140);
  }
  {
    pbf_body_contact f = c;
    f.friction = 0.05;
    Case k = begin("friction-slides", b, f);
    for (int p = 0; p < 4; ++p) pass(k, floor_sums(50, 1.2));
    f.friction = 50;
    Case s = begin("friction-sticks", b, f);
    for (int p = 0; p < 4; ++p) pass(s, floor_sums(50, 1.2));
  }
  {
    pbf_collider_body l = b;
    l.linear_factor[0] = 0, l.linear_factor[2] = 0, l.angular_factor[1] = 0;
    pbf_body_contact f = c;
    f.friction = 0.4;
    Case k = begin("locked-axes", l, f);
    for (int p = 0; p < 5; ++p) pass(k, floor_sums(64, 2.0));
    check("locked axes stay where they are", k.body.st.pose.trans[0] == 420 && k.body.st.pose.trans[2] == 555 &&
                                                 k.body.st.velocity[0] == 30 && k.body.st.angular_velocity[1] == -0.9);
  }
  {
    pbf_collider_body m = b;
    m.centre_min[1] = 309.5;  // (the floor pushes towards -y: the first shift reaches the bound)
    Case k = begin("centre-bound", m, c);
    for (int p = 0; p < 3; ++p) pass(k, floor_sums(20, 3.0));
    check("centre bound: clamped and stopped", k.body.st.pose.trans[1] == 309.5 && k.body.st.velocity[1] == 0.0);
  }
  {
    Case k = begin("cancelling", b, c);
    bodycontact::Sums s = floor_sums(10, 1.0);
    s.M[0] = s.M[1] = s.M[2] = 0.0;
    pass(k, s);
    pass(k, floor_sums(10, 1.0));
    check("M = 0 is rejected, the next pass responds", k.contact.st.rejected == 1 && k.contact.st.contacts == 1 && k.contact.st.passes == 2);
  }
  {
    Case k = begin("non-finite", b, c);
    bodycontact::Sums s = floor_sums(10, 1.0);
    s.A[2] = kNaN;
    pass(k, s);
    s = floor_sums(10, 1.0), s.S = kInf;
    pass(k, s);
    s = floor_sums(10, 1.0), s.M[1] = -1e200, s.M[0] = 1e200;  // (ln overflows)
    pass(k, s);
    pass(k, floor_sums(10, 1.0));
    check("non-finite sums are rejected and leave the body finite", k.contact.st.rejected == 3 && k.contact.st.contacts == 1 &&
                                                                        colliderbody::finite(k.body.st.velocity[1]));
  }
  return shim::finish();
}
