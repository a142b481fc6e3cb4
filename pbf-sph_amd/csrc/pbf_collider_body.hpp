// pbf_collider_body.hpp — the rigid body of pbf_set_collider_body (include/pbf_hip.h): what the call refuses about its
// parameters, the record the ctx keeps on the device, the conversion of a rotation matrix to a unit quaternion and the
// advance of one step.  Plain C++: no HIP and no library call in it, so host/test_collider_body.cpp compiles it alone.
// advance() is marked PBF_BODY_FN, __host__ __device__ under hipcc and empty otherwise: k_body_advance (csrc/pbf_kernels.hpp)
// and the host program run the same text.
//
// Everything is evaluated in double whatever the ctx's N, in the order written, not contracted (the library is built with
// -ffp-contract=off and IEEE sqrt and divide); PBF_FLAG_FAST_MATH does not reach it.
//
// The state: x[3] the centre of mass (world units; the pose's t, since the body frame's origin is the centre of mass),
// q[4] a unit quaternion (w, x, y, z), body -> world, v[3] world units per time, w[3] the angular velocity in the world
// frame, rad per time.  The body's principal axes are the lattice's axes.
//
// One advance takes dt and the step's raw sums P, L — exactly pbf_collider_wrench.impulse and .angular, L about the t the
// step's delta-p launches read:
//
//   R      = R(q):  R00 = 1 - 2 (y y + z z)   R01 = 2 (x y - w z)       R02 = 2 (x z + w y)
//                   R10 = 2 (x y + w z)       R11 = 1 - 2 (x x + z z)   R12 = 2 (y z - w x)
//                   R20 = 2 (x z - w y)       R21 = 2 (y z + w x)       R22 = 1 - 2 (x x + y y)
//   J_a    = -(gain * P_a) / dt        H_a = -(gain * L_a) / dt
//            one non-finite J or H: all six count as zero for this step and `rejected` goes up by one
//   v'_a   = ((v_a + dt * accel_a) + J_a / mass) * linear_factor_a / (1 + dt * linear_damping)
//   h_b    = (R[0][b] H_0 + R[1][b] H_1) + R[2][b] H_2                  (R^T H)
//   k_b    = h_b / inertia_b
//   w'_a   = ((w_a + ((R[a][0] k_0 + R[a][1] k_1) + R[a][2] k_2)) * angular_factor_a) / (1 + dt * angular_damping)
//   x'_a   = x_a + dt * v'_a ;  x'_a < centre_min_a or > centre_max_a: x'_a = that bound, v'_a = 0
//   d      = (0, w') (x) q:   d_w = -((w'_x q_x + w'_y q_y) + w'_z q_z)
//                             d_x = (w'_x q_w + w'_y q_z) - w'_z q_y     (y, z cyclic)
//   u      = q + (dt / 2) * d ;   q' = u / sqrt(((u_w u_w + u_x u_x) + u_y u_y) + u_z u_z)
//   pose   = { R(q'), x' }        steps += 1
//
// `gain` is the caller's.  Finalise gives a particle the collider displaced by delta the velocity change VD * delta / dt
// with VD = 0.49 (the reference's damping of the position-derived velocity), so with gain = 0.49 the body receives exactly
// the momentum the fluid was given; gain = 1 is the plain position-based estimate delta / dt.
//
// With friction on as well (pbf_set_collider_friction, csrc/pbf_collider_friction.hpp) the stage first hands the body the
// raw sums P, L of the previous step's friction pass — impulses already, world units x mass / time, L about x — through
// kick(), then advances as above:
//
//   R      = R(q)
//   v_a    = v_a + (-P_a / mass) * linear_factor_a
//   h_b    = (R[0][b] (-L_0) + R[1][b] (-L_1)) + R[2][b] (-L_2)         k_b = h_b / inertia_b
//   w_a    = w_a + ((R[a][0] k_0 + R[a][1] k_1) + R[a][2] k_2) * angular_factor_a
//            one non-finite P or L: no kick, and `rejected` goes up by one
//
// Limitations: there is no gyroscopic term (w x I w): a spinning asymmetric body does not precess.  No contact of the body
// with the box or with obstacles beyond the bounds of its centre (contact with the scenery: csrc/pbf_body_contact.hpp), no
// swept collision, no restitution against the fluid.
#pragma once

#include <cstddef>
#include <cstdint>

#include "pbf_collider_pose.hpp"
#include "pbf_hip.h"

#if defined(__HIP__)
#define PBF_BODY_FN __host__ __device__
#else
#define PBF_BODY_FN
#endif

namespace colliderbody {

// the parameters: the front of pbf_collider_body
struct Params {
  double mass, inertia[3], gain, linear_damping, angular_damping, accel[3], linear_factor[3], angular_factor[3], centre_min[3],
      centre_max[3];
};
static_assert(offsetof(pbf_collider_body, pose) == sizeof(Params), "Params is pbf_collider_body up to its start pose");

// the ctx's device record: written whole by pbf_set_collider_body (k_body_store), advanced by k_body_advance, read by
// pbf_collider_body_state.  st.pose.trans is x, st.quat is q.
struct Record {
  Params par;
  struct pbf_collider_body_state st;
};

// (x - x is 0 for every finite x and NaN otherwise: no library call)
PBF_BODY_FN inline bool finite(double x) { return x - x == 0.0; }

// row-major R(q) of q = (w, x, y, z)
PBF_BODY_FN inline void rotation_of(const double *q, double *r) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  r[0] = 1.0 - 2.0 * (y * y + z * z), r[1] = 2.0 * (x * y - w * z), r[2] = 2.0 * (x * z + w * y);
  r[3] = 2.0 * (x * y + w * z), r[4] = 1.0 - 2.0 * (x * x + z * z), r[5] = 2.0 * (y * z - w * x);
  r[6] = 2.0 * (x * z - w * y), r[7] = 2.0 * (y * z + w * x), r[8] = 1.0 - 2.0 * (x * x + y * y);
}

PBF_BODY_FN inline void normalise(double *q) {
  const double n = __builtin_sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  for (int k = 0; k < 4; ++k) q[k] = q[k] / n;
}

// the unit quaternion of a rotation matrix (row-major, as colliderpose::check accepts it), by the largest of the trace and
// the diagonal entries (Shepperd), then normalised:
//   tr = (R00 + R11) + R22 > 0:   s = 2 sqrt(tr + 1)                  q = (s / 4, (R21 - R12) / s, (R02 - R20) / s, (R10 - R01) / s)
//   else R00 > R11, R00 > R22:    s = 2 sqrt(((1 + R00) - R11) - R22)   q = ((R21 - R12) / s, s / 4, (R01 + R10) / s, (R02 + R20) / s)
//   else R11 > R22:               s = 2 sqrt(((1 + R11) - R00) - R22)   q = ((R02 - R20) / s, (R01 + R10) / s, s / 4, (R12 + R21) / s)
//   else:                         s = 2 sqrt(((1 + R22) - R00) - R11)   q = ((R10 - R01) / s, (R02 + R20) / s, (R12 + R21) / s, s / 4)
PBF_BODY_FN inline void quaternion_of(const double *r, double *q) {
  const double tr = (r[0] + r[4]) + r[8];
  if (tr > 0.0) {
    const double s = 2.0 * __builtin_sqrt(tr + 1.0);
    q[0] = s / 4.0, q[1] = (r[7] - r[5]) / s, q[2] = (r[2] - r[6]) / s, q[3] = (r[3] - r[1]) / s;
  } else if (r[0] > r[4] && r[0] > r[8]) {
    const double s = 2.0 * __builtin_sqrt(((1.0 + r[0]) - r[4]) - r[8]);
    q[0] = (r[7] - r[5]) / s, q[1] = s / 4.0, q[2] = (r[1] + r[3]) / s, q[3] = (r[2] + r[6]) / s;
  } else if (r[4] > r[8]) {
    const double s = 2.0 * __builtin_sqrt(((1.0 + r[4]) - r[0]) - r[8]);
    q[0] = (r[2] - r[6]) / s, q[1] = (r[1] + r[3]) / s, q[2] = s / 4.0, q[3] = (r[5] + r[7]) / s;
  } else {
    const double s = 2.0 * __builtin_sqrt(((1.0 + r[8]) - r[0]) - r[4]);
    q[0] = (r[3] - r[1]) / s, q[1] = (r[2] + r[6]) / s, q[2] = (r[5] + r[7]) / s, q[3] = s / 4.0;
  }
  normalise(q);
}

// one step of the body: the text of this file's head.  P, L, hits: the sums the step's reduction delivered.
PBF_BODY_FN inline void advance(const Params &par, struct pbf_collider_body_state &st, double dt, const double *P, const double *L,
                                uint64_t hits) {
  double *x = st.pose.trans, *q = st.quat, *v = st.velocity, *w = st.angular_velocity;
  double R[9];
  rotation_of(q, R);
  double J[3], H[3];
  bool ok = true;
  for (int a = 0; a < 3; ++a) {
    J[a] = -(par.gain * P[a]) / dt, H[a] = -(par.gain * L[a]) / dt;
    ok = ok && finite(J[a]) && finite(H[a]);
  }
  if (!ok) {
    for (int a = 0; a < 3; ++a) J[a] = 0.0, H[a] = 0.0;
    st.rejected += 1;
  }
  for (int a = 0; a < 3; ++a)
    v[a] = ((v[a] + dt * par.accel[a]) + J[a] / par.mass) * par.linear_factor[a] / (1.0 + dt * par.linear_damping);
  double k[3];
  for (int b = 0; b < 3; ++b) k[b] = ((R[b] * H[0] + R[3 + b] * H[1]) + R[6 + b] * H[2]) / par.inertia[b];
  for (int a = 0; a < 3; ++a)
    w[a] = ((w[a] + ((R[3 * a] * k[0] + R[3 * a + 1] * k[1]) + R[3 * a + 2] * k[2])) * par.angular_factor[a]) /
           (1.0 + dt * par.angular_damping);
  for (int a = 0; a < 3; ++a) {
    x[a] = x[a] + dt * v[a];
    if (x[a] < par.centre_min[a]) x[a] = par.centre_min[a], v[a] = 0.0;
    else if (x[a] > par.centre_max[a]) x[a] = par.centre_max[a], v[a] = 0.0;
  }
  const double s = dt / 2.0;
  const double d[4] = {-((w[0] * q[1] + w[1] * q[2]) + w[2] * q[3]), (w[0] * q[0] + w[1] * q[3]) - w[2] * q[2],
                       (w[1] * q[0] + w[2] * q[1]) - w[0] * q[3], (w[2] * q[0] + w[0] * q[2]) - w[1] * q[1]};
  for (int c = 0; c < 4; ++c) q[c] = q[c] + s * d[c];
  normalise(q);
  rotation_of(q, st.pose.rot);
  for (int a = 0; a < 3; ++a) st.impulse[a] = P[a], st.angular[a] = L[a];
  st.hits = hits;
  st.steps += 1;
}

// the friction pass's sums P, L (about x) as one impulse on the body: the text of this file's head
PBF_BODY_FN inline void kick(const Params &par, struct pbf_collider_body_state &st, const double *P, const double *L) {
  double *v = st.velocity, *w = st.angular_velocity;
  bool ok = true;
  for (int a = 0; a < 3; ++a) ok = ok && finite(P[a]) && finite(L[a]);
  if (!ok) {
    st.rejected += 1;
    return;
  }
  double R[9];
  rotation_of(st.quat, R);
  for (int a = 0; a < 3; ++a) v[a] = v[a] + (-P[a] / par.mass) * par.linear_factor[a];
  double k[3];
  for (int b = 0; b < 3; ++b) k[b] = ((R[b] * (-L[0]) + R[3 + b] * (-L[1])) + R[6 + b] * (-L[2])) / par.inertia[b];
  for (int a = 0; a < 3; ++a) w[a] = w[a] + ((R[3 * a] * k[0] + R[3 * a + 1] * k[1]) + R[3 * a + 2] * k[2]) * par.angular_factor[a];
}

// the record pbf_set_collider_body writes: the parameters, the state at rest in its start pose (which is kept as given:
// the first step's delta-p launches read N(rot), N(trans) as a pbf_set_collider_pose call would have left them)
inline Record record_of(const pbf_collider_body &b) {
  Record r{};
  const double *front = &b.mass;
  double *par = &r.par.mass;
  for (size_t k = 0; k < sizeof(Params) / sizeof(double); ++k) par[k] = front[k];
  r.st.pose = b.pose;
  quaternion_of(b.pose.rot, r.st.quat);
  for (int a = 0; a < 3; ++a) r.st.velocity[a] = b.velocity[a], r.st.angular_velocity[a] = b.angular_velocity[a];
  return r;
}

// PBF_OK, or PBF_ERR_INVALID with *why (may be NULL) naming the condition
inline int check(const pbf_collider_body *b, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  const double *front = &b->mass;
  for (size_t k = 0; k < sizeof(Params) / sizeof(double); ++k) {
    const bool bound = k >= offsetof(Params, centre_min) / sizeof(double);  // (the centre bounds may be +-inf, not NaN)
    if (bound ? front[k] != front[k] : !finite(front[k]))
      return *why = "pbf_set_collider_body: a non-finite parameter", PBF_ERR_INVALID;
  }
  for (int a = 0; a < 3; ++a)
    if (!finite(b->velocity[a]) || !finite(b->angular_velocity[a]))
      return *why = "pbf_set_collider_body: a non-finite start velocity", PBF_ERR_INVALID;
  if (!(b->mass > 0)) return *why = "pbf_set_collider_body: mass <= 0", PBF_ERR_INVALID;
  for (int a = 0; a < 3; ++a)
    if (!(b->inertia[a] > 0)) return *why = "pbf_set_collider_body: an inertia <= 0", PBF_ERR_INVALID;
  if (b->gain < 0) return *why = "pbf_set_collider_body: gain < 0", PBF_ERR_INVALID;
  if (b->linear_damping < 0 || b->angular_damping < 0) return *why = "pbf_set_collider_body: a damping < 0", PBF_ERR_INVALID;
  for (int a = 0; a < 3; ++a)
    if ((b->linear_factor[a] != 0.0 && b->linear_factor[a] != 1.0) || (b->angular_factor[a] != 0.0 && b->angular_factor[a] != 1.0))
      return *why = "pbf_set_collider_body: a factor other than 0 or 1", PBF_ERR_INVALID;
  for (int a = 0; a < 3; ++a)
    if (b->centre_min[a] > b->centre_max[a]) return *why = "pbf_set_collider_body: centre_min > centre_max", PBF_ERR_INVALID;
  return colliderpose::check(&b->pose, why);
}

}  // namespace colliderbody
