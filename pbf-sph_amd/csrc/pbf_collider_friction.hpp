// pbf_collider_friction.hpp — Coulomb friction against the collider (pbf_set_collider_friction, include/pbf_hip.h): the
// argument check, the small device records, and k_collider_friction, ONE streaming pass on the finalised velocity.  This is
// Bridson's particle - level-set friction, v_t' = max(0, 1 - mu dv_n / |v_t|) v_t, relative to the solid's contact velocity;
// dv_n is what this solver's finalise really gave the particle from the solid's push, which is why VD appears.
//
// The pass reads the step's reaction records (DeltaOp<.., COLLIDE_REACT>): A, the summed world displacement the solid gave
// the particle over the iterations, is the contact normal and the normal impulse at once, so no lattice is loaded.
//
// The contract (the same text as the header's).  Everything per particle is in N, in the order written, not contracted (the
// library is built with -ffp-contract=off and IEEE sqrt and divide); PBF_FLAG_FAST_MATH does not reach it.  vel4 is in the
// solver frame (world / scale, see finalise_one); A, V, W and t are world.
//
//   V, W   = the friction record's, rounded to N; with a body on: N(st.velocity), N(st.angular_velocity) of the body record
//            as the kernel finds them
//   t      = the ctx's ColliderPose trans as the kernel finds it (no pose ever set: the identity record, 0); mu = N(record's)
//   particle a, its record A = push[2 r], r = rowSlotOf[a] when the delta-p launches ran on the row-major copy, else a
//   (obstacles keep the sort's zero record: they never act)
//     len  = sqrt((A_x A_x + A_y A_y) + A_z A_z)          act = A.w > 0 && len > 0
//     n_a  = A_a / len
//     r_a  = pos4[a]_a - t_a                               (the finalised world position)
//     c_x  = W_y r_z - W_z r_y   (y, z cyclic; each product rounded, one subtraction)
//     vb_a = (V_a + c_a) / scale
//     u_a  = v_a - vb_a          un = (u_x n_x + u_y n_y) + u_z n_z          ut_a = u_a - un * n_a
//     s    = sqrt((ut_x ut_x + ut_y ut_y) + ut_z ut_z)     slide = act && s > 0
//     jn   = (VD * (len / scale)) / dt                     (the speed finalise gave the particle from the solid's push)
//     g    = (mu * jn) / s        f = g < 1 ? g : 1        (a NaN g counts as 1)        dv_a = -(f * ut_a)
//     v'_a = slide ? v_a + dv_a : v_a                      (bits kept otherwise; pos4, pStar, lambda untouched)
//   sums, terms formed in double:  m = pos4[a].w   p_a = m * (double(dv_a) * double(scale))
//     P += p        L_x += double(r_y) p_z - double(r_z) p_y  (y, z cyclic)        + the sums of |term|
//     cnt[0] = particles that slid          cnt[1] = particles with act
//
// A lane whose record has A.w == 0 loads neither pos4 nor vel4 — a wave without a contact streams 16 B per particle (and the
// 4-byte slot) — and contributes the identity; a lane that does not slide stores nothing.
//
// The reduction is k_wrench_partial's: workgroup b owns the particles [DIAG_TILE b, DIAG_TILE (b + 1)) of the Morton order,
// lanes by the butterfly, waves through LDS, no atomics (WrenchPartial, wrench_block_fold, wrench_fold_partials).  The partial
// records stay in a buffer of the pass's own until the next pass overwrites them: pbf_collider_friction_reaction folds them
// for the host (k_friction_final), and with a body on the body stage of the NEXT step folds them and kicks the body
// (k_body_kick_advance).  The host carries them across a grow of the buffer (an upload that grows the capacity), and
// pbf_set_collider_body drops sums that are still pending when it places a body.  Ctl counts on the device: whether the
// last pass's sums are still to be consumed by a body, the number of its partial records, and the passes run.
//
// V, W, mu and t sit at the same address for every lane and arrive through const __restrict__ pointers: the compiler may
// load them on the scalar path, once per wave.
//
// Limitations: one coefficient (no separate static and kinetic friction), no restitution, no friction against the box walls
// or obstacle particles, not in slab mode.
#pragma once

#include <cstddef>
#include <cstdint>

#include "pbf_collider_body.hpp"
#include "pbf_hip.h"

namespace colliderfriction {

// the device's counters: written by the pass (one lane), read and cleared by the body stage, read by the observer
struct Ctl {
  unsigned long long pending;  // 1: the partial records hold sums no body has consumed
  unsigned long long nb;       // partial records of the last pass
  unsigned long long passes;   // passes since friction was turned on
};

// PBF_OK, or PBF_ERR_INVALID with *why (may be NULL) naming the condition
inline int check(const pbf_collider_friction *f, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  if (!(f->mu > 0)) return *why = "pbf_set_collider_friction: mu <= 0 or NaN", PBF_ERR_INVALID;
  for (int a = 0; a < 3; ++a)
    if (!colliderbody::finite(f->velocity[a]) || !colliderbody::finite(f->angular_velocity[a]))
      return *why = "pbf_set_collider_friction: a non-finite velocity", PBF_ERR_INVALID;
  return PBF_OK;
}

}  // namespace colliderfriction

#if defined(__HIP__)
#include "pbf_kernels.hpp"

namespace pbf {

// pbf_set_collider_friction: one lane writes the ctx's friction record, in stream order with the steps before and after it.
// The record arrives by value, as in k_collider_pose_store.  reset: friction has just been turned on.
__global__ void k_friction_store(pbf_collider_friction v, pbf_collider_friction *dst, colliderfriction::Ctl *ctl, int reset) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  *dst = v;
  if (reset) ctl->pending = 0ull, ctl->nb = 0ull, ctl->passes = 0ull;
}

// pbf_set_collider_body while friction is on: the sums of a pass that ran before the body was placed are not handed to it
// (they stay readable through pbf_collider_friction_reaction)
__global__ void k_friction_pending_clear(colliderfriction::Ctl *ctl) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  ctl->pending = 0ull;
}

// vw: six doubles V.xyz, W.xyz — the friction record's, or the body record's st.velocity and st.angular_velocity
template <typename N>
__global__ __launch_bounds__(BLOCK) void k_collider_friction(uint32_t n, N scale, N dt, const pbf_collider_friction *__restrict__ rec,
                                                             const double *__restrict__ vw, const ColliderPose<N> *__restrict__ pose,
                                                             const vec4<N> *__restrict__ push, const uint32_t *__restrict__ slotOf,
                                                             const vec4<N> *__restrict__ pos4, vec4<N> *__restrict__ vel4,
                                                             WrenchPartial *__restrict__ partials, colliderfriction::Ctl *__restrict__ ctl) {
  __shared__ WrenchPartial waves[BLOCK / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t waveBase = blockIdx.x * DIAG_TILE + wave * 64u * DIAG_ITEMS;
  const N mu = N(rec->mu);
  const N Vx = N(vw[0]), Vy = N(vw[1]), Vz = N(vw[2]), Wx = N(vw[3]), Wy = N(vw[4]), Wz = N(vw[5]);
  const N tx = pose->trans[0], ty = pose->trans[1], tz = pose->trans[2];
  WrenchPartial a;
  wrench_identity(a);
#pragma unroll 1
  for (int j = 0; j < DIAG_ITEMS; ++j) {
    const uint32_t i = waveBase + j * 64u + lane;
    if (i >= n) continue;
    const vec4<N> A = push[2u * (slotOf ? slotOf[i] : i)];
    if (!(A.w > N(0))) continue;  // (never hit: nothing more is loaded)
    const N len = sqrt((A.x * A.x + A.y * A.y) + A.z * A.z);
    if (!(len > N(0))) continue;
    a.cnt[1] += 1ull;
    const vec4<N> p = pos4[i], v = vel4[i];
    const N nx = A.x / len, ny = A.y / len, nz = A.z / len;
    const N rx = p.x - tx, ry = p.y - ty, rz = p.z - tz;
    const N cx = Wy * rz - Wz * ry, cy = Wz * rx - Wx * rz, cz = Wx * ry - Wy * rx;
    const N bx = (Vx + cx) / scale, by = (Vy + cy) / scale, bz = (Vz + cz) / scale;
    const N ux = v.x - bx, uy = v.y - by, uz = v.z - bz;
    const N un = (ux * nx + uy * ny) + uz * nz;
    const N sx = ux - un * nx, sy = uy - un * ny, sz = uz - un * nz;
    const N s = sqrt((sx * sx + sy * sy) + sz * sz);
    if (!(s > N(0))) continue;
    const N jn = (N(VD) * (len / scale)) / dt;
    const N g = (mu * jn) / s;
    const N f = g < N(1) ? g : N(1);
    const N dx = -(f * sx), dy = -(f * sy), dz = -(f * sz);
    vel4[i] = make_vec4<N>(v.x + dx, v.y + dy, v.z + dz, v.w);
    const double m = double(p.w), sc = double(scale);
    const double px = m * (double(dx) * sc), py = m * (double(dy) * sc), pz = m * (double(dz) * sc);
    const double t[6] = {px, py, pz, double(ry) * pz - double(rz) * py, double(rz) * px - double(rx) * pz, double(rx) * py - double(ry) * px};
    for (int k = 0; k < 6; ++k) a.sum[k] += t[k], a.sum[6 + k] += fabs(t[k]);
    a.cnt[0] += 1ull;
  }
  wrench_block_fold(a, waves);
  if (threadIdx.x != 0) return;
  partials[blockIdx.x] = a;
  if (blockIdx.x == 0) ctl->pending = 1ull, ctl->nb = gridDim.x, ctl->passes = ctl->passes + 1ull;
}

// pbf_collider_friction_reaction: the last pass's partial records folded by ONE workgroup into the pinned record the host
// polls, as k_wrench_final does for the reaction.  The number of records is the device's (Ctl::nb).
__global__ __launch_bounds__(BLOCK) void k_friction_final(const WrenchPartial *__restrict__ partials, const colliderfriction::Ctl *__restrict__ ctl,
                                                          volatile WrenchRecord *__restrict__ host, uint32_t seq) {
  __shared__ WrenchPartial waves[BLOCK / 64];
  WrenchPartial t;
  wrench_fold_partials(uint32_t(ctl->nb), partials, waves, t);
  if (threadIdx.x != 0) return;
  for (int k = 0; k < 3; ++k) {
    host->impulse[k] = t.sum[k], host->angular[k] = t.sum[3 + k];
    host->abs_impulse[k] = t.sum[6 + k], host->abs_angular[k] = t.sum[9 + k];
  }
  host->hits = t.cnt[0], host->particles = t.cnt[1], host->step = ctl->passes;
  __threadfence_system();
  host->seq = seq;
  __threadfence_system();
}

// The body stage with friction on: k_body_advance with the kick in front.  ONE workgroup folds the friction partials of the
// previous step's pass when they are still pending (every thread reads the same two words, so the trip count is uniform),
// thread 0 kicks the body and clears the word; then the reaction's partials and the advance, exactly as k_body_advance.
template <typename N>
__global__ __launch_bounds__(BLOCK) void k_body_kick_advance(const WrenchPartial *__restrict__ frictionPartials, colliderfriction::Ctl *ctl,
                                                             uint32_t nb, const WrenchPartial *__restrict__ partials, double dt,
                                                             colliderbody::Record *body, ColliderPose<N> *pose) {
  __shared__ WrenchPartial waves[BLOCK / 64];
  const bool pending = ctl->pending != 0ull;
  const uint32_t fnb = uint32_t(ctl->nb);
  __syncthreads();  // (thread 0 clears the word below only after every thread has read it)
  WrenchPartial f, t;
  wrench_identity(f);
  if (pending) wrench_fold_partials(fnb, frictionPartials, waves, f);
  wrench_fold_partials(nb, partials, waves, t);
  if (threadIdx.x != 0) return;
  colliderbody::Record r = *body;
  if (pending) {
    colliderbody::kick(r.par, r.st, &f.sum[0], &f.sum[3]);
    ctl->pending = 0ull;
  }
  colliderbody::advance(r.par, r.st, dt, &t.sum[0], &t.sum[3], t.cnt[0]);
  body->st = r.st;
  for (int k = 0; k < 9; ++k) pose->rot[k] = N(r.st.pose.rot[k]);
  for (int k = 0; k < 3; ++k) pose->trans[k] = N(r.st.pose.trans[k]);
}

}  // namespace pbf
#endif
