// pbf_body_contact.hpp — contact of the rigid body with the scenery (pbf_set_collider_body_contact, include/pbf_hip.h): what
// the call refuses about its parameters, the small owner of its mode (on / off, the point count, the passes per step, the
// generation a captured step's key takes), the record the ctx keeps on the device, and the response of one pass.  Plain
// C++17: no HIP and no library call in it, so host/test_body_contact.cpp compiles it alone.  resolve() is marked PBF_BODY_FN
// like colliderbody::advance: k_contact_resolve (csrc/pbf_body_contact_kernels.hpp) and the host program run the same text.
//
// The body's surface is a fixed set of points b in the body frame, taken once from the collider's lattice (the kernels'
// header says how).  Every step, after the body's advance, `iterations` passes run; each pass is two launches.
//
// The detection of one pass, per point b (N, body frame).  R and x are the body record's pose in double; the order is the
// order written, not contracted; PBF_FLAG_FAST_MATH does not reach it:
//
//   r_a = (R[a][0] b_0 + R[a][1] b_1) + R[a][2] b_2        w_a = r_a + x_a
//   the static contract of csrc/pbf_collider.hpp on the scenery's lattice with margin := N(skin), at (N(w_0), N(w_1), N(w_2))
//        -> inside, hit, k = (margin - phi) / len, g
//   m_a = double(k) * double(g_a)          d = sqrt((m_0 m_0 + m_1 m_1) + m_2 m_2)
//   in contact  =  inside && hit && d > 0 && d finite
//   sums over the points in contact:  S = sum d,  M_a = sum m_a,  A_a = sum d * r_a,  D = max d,  count
//
// The response of that pass (resolve(), everything in double, in the order written, not contracted).  mass, inertia, F =
// linear_factor, G = angular_factor and the centre bounds are the body's; e = restitution, mu = friction, beta = correction
// and slop are the contact's; x, v, w are the body's centre, velocity and angular velocity, R its pose's rotation:
//
//   passes += 1;  the raw sums S, M, A, D go to the state, impulse = shift = 0
//   count == 0: done                                                        (the sums are the zeros)
//   ln = sqrt((M_0 M_0 + M_1 M_1) + M_2 M_2)
//   S, an M_a, an A_a, D or ln non-finite, or !(ln > 0): rejected += 1, done                  (opposite walls cancel)
//   n_a = M_a / ln          r_a = A_a / S          contacts += 1
//   cross(p, q) = (p_1 q_2 - p_2 q_1,  p_2 q_0 - p_0 q_2,  p_0 q_1 - p_1 q_0)
//   dot(p, q)   = (p_0 q_0 + p_1 q_1) + p_2 q_2
//   W(c):  h_b = (R[0][b] c_0 + R[1][b] c_1) + R[2][b] c_2 ;  k_b = h_b / inertia_b
//          W_a = ((R[a][0] k_0 + R[a][1] k_1) + R[a][2] k_2) * G_a
//   Wn = W(cross(r, n))
//   kn = ((F_0 n_0 n_0 + F_1 n_1 n_1) + F_2 n_2 n_2) / mass + dot(n, cross(Wn, r))          (F_a n_a n_a = (F_a * n_a) * n_a)
//   u  = v + cross(w, r)          un = dot(u, n)
//   un < 0 && kn > 0:  j = -((1 + e) * un) / kn ;  v_a = v_a + ((j * n_a) / mass) * F_a ;  w_a = w_a + j * Wn_a
//   else:              j = 0
//   mu > 0 && j > 0:   u' = v + cross(w, r) ;  c = dot(u', n) ;  ut_a = u'_a - c * n_a
//                      lt = sqrt((ut_0 ut_0 + ut_1 ut_1) + ut_2 ut_2)
//                      lt > 0:  t_a = ut_a / lt ;  Wt = W(cross(r, t))
//                               kt = ((F_0 t_0 t_0 + F_1 t_1 t_1) + F_2 t_2 t_2) / mass + dot(t, cross(Wt, r))
//                               kt > 0:  jt = min(mu * j, lt / kt)
//                                        v_a = v_a - ((jt * t_a) / mass) * F_a ;  w_a = w_a - jt * Wt_a
//                      (jt = 0 and t = 0 wherever a condition fails)
//   impulse_a = j * n_a - jt * t_a
//   s = beta * max(D - slop, 0) ;  shift_a = (s * n_a) * F_a ;  x_a = x_a + shift_a
//   x_a < centre_min_a or > centre_max_a: x_a = that bound, v_a = 0           (exactly as advance() applies the bounds)
//   pose.trans = x (rot and q unchanged); the kernel rewrites N(x) in the pose record the delta-p launches read
//
// n is the direction in which the scenery pushes the averaged contact out, r the depth-weighted contact point about the
// centre of mass: ONE impulse per pass at one point, along one normal.  A single pass leaves a share (1 - beta) of the depth
// beyond slop; further passes of the same step detect again from the shifted centre.  The impulse is the classic
// j = -(1 + e) un / (1/m + n . (I^-1 (r x n)) x r) with the factors folded in; friction is Coulomb's, clamped at sticking.
//
// Limitations: no contact with the box walls or with obstacle particles (walls are composed into the scenery's lattice); the
// position correction translates and never rotates the body; one averaged contact per pass, not a per-point manifold; no
// swept contact (a body faster than its own thickness per step can tunnel); one body; not in slab mode; the scenery
// receives no reaction.
#pragma once

#include <cstddef>
#include <cstdint>

#include "pbf_collider_body.hpp"
#include "pbf_hip.h"

namespace bodycontact {

// ---- the mode: read freely, changed through the events ONLY (tests/test_body_contact_cpu.py holds pbf_hip.hip to that) ----
// `gen` is part of a captured step's key (GraphKey::contact).  An event that changes which launches a step runs or their
// arguments — off <-> on, another point set, another number of passes — bumps it and returns true: the caller then drops the
// captured graphs.  A rewrite of the record alone returns false.
struct Mode {
  bool on = false;          // stage_body runs the passes
  uint64_t points = 0;      // points in the buffer (> 0 while on)
  uint32_t iterations = 0;  // passes per step (1..8 while on)
  uint32_t stride = 0;      // the extraction the buffer came from
  double level = 0;
  uint64_t gen = 0;

  // the point buffer of this configuration is the one in place: a configure call may keep it and rewrite the record only
  bool same_points(double lvl, uint32_t str) const { return on && lvl == level && str == stride; }
  uint32_t launches_per_step() const { return on ? 2u * iterations : 0u; }

  // a point set was extracted and the record stored (off -> on, or another level / stride while on)
  bool configured(uint64_t n, uint32_t iters, double lvl, uint32_t str) {
    if (n == 0 || iters == 0) return false;  // (refused by the entry point: nothing changes)
    on = true, points = n, iterations = iters, level = lvl, stride = str;
    return bump();
  }
  // the record was rewritten while on with the same point set; another number of passes is another launch sequence
  bool rewritten(uint32_t iters) {
    if (!on || iters == 0 || iters == iterations) return false;
    iterations = iters;
    return bump();
  }
  // NULL to the call, a cleared body, a replaced or cleared collider, a cleared scenery
  bool cleared() {
    if (!on) return false;
    on = false, points = 0, iterations = 0, stride = 0, level = 0;
    return bump();
  }

 private:
  bool bump() { return ++gen, true; }
};

// ---- the record on the device ----
struct Params {
  double skin, restitution, friction, correction, slop;
};
struct Record {
  Params par;
  struct pbf_body_contact_state st;
};
// what one detection pass delivers
struct Sums {
  double S, M[3], A[3], D;
  uint64_t count;
};

using colliderbody::finite;

// PBF_OK, or PBF_ERR_INVALID with *why (may be NULL) naming the condition
inline int check(const pbf_body_contact *c, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  if (!finite(c->level) || !finite(c->skin) || !finite(c->restitution) || !finite(c->friction) || !finite(c->correction) ||
      !finite(c->slop))
    return *why = "pbf_set_collider_body_contact: a non-finite parameter", PBF_ERR_INVALID;
  if (c->stride < 1) return *why = "pbf_set_collider_body_contact: stride < 1", PBF_ERR_INVALID;
  if (c->skin < 0) return *why = "pbf_set_collider_body_contact: skin < 0", PBF_ERR_INVALID;
  if (c->restitution < 0 || c->restitution > 1) return *why = "pbf_set_collider_body_contact: restitution outside [0, 1]", PBF_ERR_INVALID;
  if (c->friction < 0) return *why = "pbf_set_collider_body_contact: friction < 0", PBF_ERR_INVALID;
  if (c->correction < 0 || c->correction > 1) return *why = "pbf_set_collider_body_contact: correction outside [0, 1]", PBF_ERR_INVALID;
  if (c->slop < 0) return *why = "pbf_set_collider_body_contact: slop < 0", PBF_ERR_INVALID;
  if (c->iterations < 1 || c->iterations > 8) return *why = "pbf_set_collider_body_contact: iterations outside 1..8", PBF_ERR_INVALID;
  return PBF_OK;
}

// the record pbf_set_collider_body_contact writes: the parameters, the counters at zero
inline Record record_of(const pbf_body_contact &c, uint64_t points) {
  Record r{};
  r.par.skin = c.skin, r.par.restitution = c.restitution, r.par.friction = c.friction, r.par.correction = c.correction, r.par.slop = c.slop;
  r.st.points = points;
  return r;
}

PBF_BODY_FN inline void cross(const double *p, const double *q, double *o) {
  o[0] = p[1] * q[2] - p[2] * q[1], o[1] = p[2] * q[0] - p[0] * q[2], o[2] = p[0] * q[1] - p[1] * q[0];
}
PBF_BODY_FN inline double dot(const double *p, const double *q) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }
// W(c) = (R I^-1 R^T c) * G, component by component as the head writes it
PBF_BODY_FN inline void world_inverse_inertia(const colliderbody::Params &par, const double *R, const double *c, double *W) {
  double k[3];
  for (int b = 0; b < 3; ++b) k[b] = ((R[b] * c[0] + R[3 + b] * c[1]) + R[6 + b] * c[2]) / par.inertia[b];
  for (int a = 0; a < 3; ++a) W[a] = ((R[3 * a] * k[0] + R[3 * a + 1] * k[1]) + R[3 * a + 2] * k[2]) * par.angular_factor[a];
}

// one pass's response: the text of this file's head
PBF_BODY_FN inline void resolve(const colliderbody::Params &par, struct pbf_collider_body_state &st, const Params &cp, const Sums &s,
                                struct pbf_body_contact_state &cs) {
  double *x = st.pose.trans, *v = st.velocity, *w = st.angular_velocity;
  const double *R = st.pose.rot, *F = par.linear_factor;
  cs.passes += 1;
  cs.depth_sum = s.S, cs.depth_max = s.D;
  for (int a = 0; a < 3; ++a) cs.push[a] = s.M[a], cs.arm[a] = s.A[a], cs.impulse[a] = 0.0, cs.shift[a] = 0.0;
  if (s.count == 0) return;
  const double ln = __builtin_sqrt((s.M[0] * s.M[0] + s.M[1] * s.M[1]) + s.M[2] * s.M[2]);
  bool ok = finite(s.S) && finite(s.D) && finite(ln);
  for (int a = 0; a < 3; ++a) ok = ok && finite(s.M[a]) && finite(s.A[a]);
  if (!ok || !(ln > 0.0)) {
    cs.rejected += 1;
    return;
  }
  double n[3], r[3];
  for (int a = 0; a < 3; ++a) n[a] = s.M[a] / ln, r[a] = s.A[a] / s.S;
  cs.contacts += 1;
  double c[3], Wn[3], u[3];
  cross(r, n, c);
  world_inverse_inertia(par, R, c, Wn);
  cross(Wn, r, c);
  const double kn = ((F[0] * n[0] * n[0] + F[1] * n[1] * n[1]) + F[2] * n[2] * n[2]) / par.mass + dot(n, c);
  cross(w, r, c);
  for (int a = 0; a < 3; ++a) u[a] = v[a] + c[a];
  const double un = dot(u, n);
  double j = 0.0, jt = 0.0, t[3] = {0.0, 0.0, 0.0};
  if (un < 0.0 && kn > 0.0) {
    j = -((1.0 + cp.restitution) * un) / kn;
    for (int a = 0; a < 3; ++a) v[a] = v[a] + ((j * n[a]) / par.mass) * F[a], w[a] = w[a] + j * Wn[a];
  }
  if (cp.friction > 0.0 && j > 0.0) {
    cross(w, r, c);
    for (int a = 0; a < 3; ++a) u[a] = v[a] + c[a];
    const double cn = dot(u, n);
    double ut[3];
    for (int a = 0; a < 3; ++a) ut[a] = u[a] - cn * n[a];
    const double lt = __builtin_sqrt((ut[0] * ut[0] + ut[1] * ut[1]) + ut[2] * ut[2]);
    if (lt > 0.0) {
      double tt[3], Wt[3];
      for (int a = 0; a < 3; ++a) tt[a] = ut[a] / lt;
      cross(r, tt, c);
      world_inverse_inertia(par, R, c, Wt);
      cross(Wt, r, c);
      const double kt = ((F[0] * tt[0] * tt[0] + F[1] * tt[1] * tt[1]) + F[2] * tt[2] * tt[2]) / par.mass + dot(tt, c);
      if (kt > 0.0) {
        const double stick = lt / kt, slide = cp.friction * j;
        jt = slide < stick ? slide : stick;
        for (int a = 0; a < 3; ++a) t[a] = tt[a], v[a] = v[a] - ((jt * tt[a]) / par.mass) * F[a], w[a] = w[a] - jt * Wt[a];
      }
    }
  }
  for (int a = 0; a < 3; ++a) cs.impulse[a] = j * n[a] - jt * t[a];
  const double over = s.D - cp.slop, sh = cp.correction * (over > 0.0 ? over : 0.0);
  for (int a = 0; a < 3; ++a) {
    cs.shift[a] = (sh * n[a]) * F[a];
    x[a] = x[a] + cs.shift[a];
    if (x[a] < par.centre_min[a]) x[a] = par.centre_min[a], v[a] = 0.0;
    else if (x[a] > par.centre_max[a]) x[a] = par.centre_max[a], v[a] = 0.0;
  }
}

}  // namespace bodycontact
