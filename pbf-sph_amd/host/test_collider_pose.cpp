// test_collider_pose — the pose check of csrc/pbf_collider_pose.hpp (pbf_set_collider_pose's refusals) on poses whose verdict
// can be written down by hand.  No HIP, not linked against the library.
//   accepted: the identity, a quarter turn about z, a rotation by 0.7 rad about (0.3, -0.5, 0.8) (Rodrigues, in double), the
//     same rounded to float and a product of three elementary rotations formed in float, a uniform scaling by 1.000004
//     (R^T R - I = 8e-6 on the diagonal).
//   refused: a NaN or an infinity in any of the twelve entries; a scaling by 1.00001 (2e-5); a shear of 1e-4; the zero matrix;
//     entries of 1e200 (R^T R overflows); diag(1, 1, -1) and R diag(-1, 1, 1) (orthogonal, det = -1).
// Prints "ok <name>" / "FAIL <name>" lines and "ALL OK"; exit status 0 iff all ok.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "pbf_collider_pose.hpp"
#include "shim_check.hpp"

using shim::check;

namespace {

pbf_collider_pose identity() {
  pbf_collider_pose p{};
  p.rot[0] = p.rot[4] = p.rot[8] = 1.0;
  return p;
}

pbf_collider_pose rodrigues(double x, double y, double z, double angle) {
  const double n = std::sqrt(x * x + y * y + z * z);
  const double k[3] = {x / n, y / n, z / n}, c = std::cos(angle), s = std::sin(angle);
  const double K[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
  pbf_collider_pose p = identity();
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double kk = 0;
      for (int m = 0; m < 3; ++m) kk += K[3 * a + m] * K[3 * m + b];
      p.rot[3 * a + b] += s * K[3 * a + b] + (1 - c) * kk;
    }
  p.trans[0] = 120, p.trans[1] = -40, p.trans[2] = 65;
  return p;
}

void mul(const float *a, const float *b, float *out) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) out[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}
void elementary(int axis, float angle, float *m) {
  const int i = (axis + 1) % 3, j = (axis + 2) % 3;
  for (int k = 0; k < 9; ++k) m[k] = (k % 4 == 0) ? 1.0f : 0.0f;
  m[3 * i + i] = std::cos(angle), m[3 * i + j] = -std::sin(angle), m[3 * j + i] = std::sin(angle), m[3 * j + j] = std::cos(angle);
}

bool accepted(const pbf_collider_pose &p) {
  const char *why = nullptr;
  return colliderpose::check(&p, &why) == PBF_OK && why == nullptr;
}
bool refused(const pbf_collider_pose &p) {
  const char *why = nullptr;
  return colliderpose::check(&p, &why) == PBF_ERR_INVALID && why != nullptr && colliderpose::check(&p, nullptr) == PBF_ERR_INVALID;
}

}  // namespace

int main() {
  const pbf_collider_pose R = rodrigues(0.3, -0.5, 0.8, 0.7);
  check("identity", accepted(identity()));
  pbf_collider_pose q = identity();
  q.rot[0] = 0, q.rot[1] = -1, q.rot[3] = 1, q.rot[4] = 0;
  check("quarter turn about z", accepted(q) && colliderpose::det(q.rot) == 1.0 && colliderpose::ortho_error(q.rot) == 0.0);
  check("rodrigues", accepted(R) && colliderpose::ortho_error(R.rot) < 1e-15 && std::fabs(colliderpose::det(R.rot) - 1) < 1e-15);
  pbf_collider_pose f = R;
  for (double &v : f.rot) v = double(float(v));
  check("rounded to float", accepted(f) && colliderpose::ortho_error(f.rot) > 0 && colliderpose::ortho_error(f.rot) < 1e-6);
  {
    float a[9], b[9], c[9], ab[9], abc[9];
    elementary(0, 0.4f, a), elementary(1, -1.1f, b), elementary(2, 2.3f, c);
    mul(a, b, ab), mul(ab, c, abc);
    pbf_collider_pose p = identity();
    for (int k = 0; k < 9; ++k) p.rot[k] = abc[k];
    check("composed in float", accepted(p) && colliderpose::ortho_error(p.rot) < 1e-6);
  }
  pbf_collider_pose s = R;
  for (double &v : s.rot) v *= 1.000004;
  check("scaled by 1.000004", accepted(s));
  for (double &v : s.rot) v = v / 1.000004 * 1.00001;
  check("scaled by 1.00001", refused(s));

  const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                         -std::numeric_limits<double>::infinity()};
  bool all = true;
  for (double v : bad)
    for (int k = 0; k < 12; ++k) {
      pbf_collider_pose p = R;
      (k < 9 ? p.rot[k] : p.trans[k - 9]) = v;
      all = all && refused(p);
    }
  check("a non-finite entry anywhere", all);
  pbf_collider_pose sh = R;
  sh.rot[1] += 1e-4;
  check("shear", refused(sh));
  pbf_collider_pose z{};
  check("zero matrix", refused(z));
  pbf_collider_pose big = R;
  for (double &v : big.rot) v = 1e200;
  check("overflowing entries", refused(big));
  pbf_collider_pose m = identity();
  m.rot[8] = -1;
  check("reflection diag(1, 1, -1)", refused(m) && colliderpose::ortho_error(m.rot) == 0.0);
  pbf_collider_pose rm = R;
  for (int a = 0; a < 3; ++a) rm.rot[3 * a] = -rm.rot[3 * a];
  check("reflection R diag(-1, 1, 1)", refused(rm));
  pbf_collider_pose far = R;
  far.trans[0] = 1e300;
  check("a huge finite translation is the caller's business", accepted(far));
  return shim::finish();
}
