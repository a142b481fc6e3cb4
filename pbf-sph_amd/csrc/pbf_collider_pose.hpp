// pbf_collider_pose.hpp — what pbf_set_collider_pose (include/pbf_hip.h) refuses about a pose.  Plain C++: no HIP and no
// library call in it, so host/test_collider_pose.cpp compiles it alone.
//
// Everything is evaluated in double in the order written:
//   every entry of rot and trans is finite
//   (R^T R)_ab = (R[0][a] R[0][b] + R[1][a] R[1][b]) + R[2][a] R[2][b];   max_ab |(R^T R)_ab - I_ab| <= 1e-5
//   det R = (R00 (R11 R22 - R12 R21) - R01 (R10 R22 - R12 R20)) + R02 (R10 R21 - R11 R20) >= 0       (no reflection)
// The bound is a stated condition of the interface, loose enough for a matrix composed in float (whose R^T R is off by a
// few 1e-7); the library does not re-orthonormalise.
#pragma once
#include <cmath>

#include "pbf_hip.h"

namespace colliderpose {

constexpr double kOrthoBound = 1e-5;

// max |R^T R - I| of a row-major 3 x 3 matrix
inline double ortho_error(const double *r) {
  double worst = 0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double v = (r[a] * r[b] + r[3 + a] * r[3 + b]) + r[6 + a] * r[6 + b];
      worst = std::fmax(worst, std::fabs(v - (a == b ? 1.0 : 0.0)));
    }
  return worst;
}
inline double det(const double *r) {
  return (r[0] * (r[4] * r[8] - r[5] * r[7]) - r[1] * (r[3] * r[8] - r[5] * r[6])) + r[2] * (r[3] * r[7] - r[4] * r[6]);
}

// PBF_OK, or PBF_ERR_INVALID with *why (may be NULL) naming the condition
inline int check(const pbf_collider_pose *pose, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(pose->rot[k])) return *why = "pbf_set_collider_pose: a non-finite entry in rot", PBF_ERR_INVALID;
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(pose->trans[k])) return *why = "pbf_set_collider_pose: a non-finite entry in trans", PBF_ERR_INVALID;
  if (!(ortho_error(pose->rot) <= kOrthoBound))
    return *why = "pbf_set_collider_pose: rot is not a rotation (max |R^T R - I| > 1e-5)", PBF_ERR_INVALID;
  if (det(pose->rot) < 0) return *why = "pbf_set_collider_pose: det rot < 0 (a reflection)", PBF_ERR_INVALID;
  return PBF_OK;
}

}  // namespace colliderpose
