// pbf_whitewater_solids.hpp — the diffuse particles of pbf_whitewater_step collide with the collider and the scenery
// (pbf_set_whitewater_solids, include/pbf_hip.h): the argument check, k_ww_solids — ONE streaming pass over the pool between
// k_ww_advect and the survivor scan — k_ww_solids_children over the slots k_ww_emit has just filled, and k_ww_solids_fold.
// Opt-in: a ctx that never sets it launches none of this.  No reference counterpart.
//
// The contract (the same text as the header's).  Everything is in N, in the order written, not contracted (the library is
// built with -ffp-contract=off); PBF_FLAG_FAST_MATH does not reach it; sqrt and divide are IEEE.  Per diffuse particle after
// k_ww_advect as it stands: x its world position (clamped to the box), v its velocity in the solver frame, its alive flag,
// and nF exactly as k_ww_advect forms it (weight == 0 ? 0 : count[0]).  A particle that is dead on entry is skipped: nothing
// of it is loaded, moved or counted (the compaction drops it).  e = N(restitution), f = N(friction).
//
//   q_a = x_a / scale
//   collider installed:  (q1, hit1) = what k_collider_sample computes for this q: the posed contract through the pose record
//                        when one is set, else the static contract        (collider_project[_posed], used as they stand)
//                        else q1 = q, hit1 = false
//   scenery installed:   (q2, hit2) = the static contract on q1 with the scenery's lattice;    else q2 = q1, hit2 = false
//   x'_a = (hit1 || hit2) ? min(maxB_a, max(minB_a, q2_a * scale)) : x_a                       (bits kept without a hit)
//
//   response(d, vb) for a solid that moved the point by d (solver frame) and has the velocity vb there:
//     len = sqrt((d_x d_x + d_y d_y) + d_z d_z)      act = hit && len > 0        n_a = d_a / len
//     u_a = v_a - vb_a      un = (u_x n_x + u_y n_y) + u_z n_z      ut_a = u_a - un * n_a
//     v_a <- (act && un < 0) ? (vb_a + (1 - f) * ut_a) - (e * un) * n_a : v_a                  (bits kept otherwise)
//   collider first:  d = q1 - q;   r_a = q1_a * scale - t_a;   c_x = W_y r_z - W_z r_y  (y, z cyclic; each product rounded,
//                    one subtraction, as the friction contract forms it);   vb_a = (V_a + c_a) / scale
//                    V, W = N(velocity), N(angular_velocity) of the body's state as the kernel finds it while a body is on;
//                    else the friction record's while friction is on;  else vb = 0.
//                    t = the pose record's trans as the kernel finds it (no pose ever set: the identity record, 0)
//   then scenery:    d = q2 - q1;  vb = 0, on the velocity the collider's response left
//   alive <- alive && !(absorb && nF == 0 && (hit1 || hit2))
//
// Life, kind and parent are untouched; a lane that hits nothing stores nothing.  Obstacle particles play no part.  Outside a
// lattice nothing is loaded, NaN included.  The box wins over both solids (each projection's own second clamp, then the
// clamp of x'), the scenery over the collider, as in delta-p.  The response is Bridson's particle - level-set collision with
// a restitution term: the approaching normal part of the relative velocity is reflected by e, the tangential part loses the
// share f, and a receding particle (un >= 0) is left alone, so a particle the moving collider has just pushed is not slowed.
// A push the box clamp undoes entirely (len == 0) moves nothing and changes no velocity, yet counts as a hit.
//
// Children.  A child k_ww_emit places is projected by the same two position contracts before the call returns; its velocity,
// life, kind and parent are kept and it never dies at birth.  It counts in born_inside when either lattice hit.  The number of
// children is the device's: k_ww_solids_children reads the two scans' totals as k_ww_final does.
//
// Counters.  Each workgroup counts its lanes' hit1, hit2 and absorbed flags (children: hit1 || hit2) with ballots, waves
// through LDS, and stores one partial record; k_ww_solids_fold, ONE workgroup, sums the partials in a fixed order into the
// device record pbf_whitewater_solids_stats copies out.  No atomics.
//
// Instantiations are chosen on the host by which lattices and records exist: a lane loads no pose record without a posed
// collider or a solid velocity, no V, W without a body or friction, and no lattice that is not installed.  The pool is at most
// a few hundred thousand particles: the pass is bound by its launch, not by bandwidth, so it is a plain one-lane-per-particle
// stream at BLOCK lanes with one LDS word triple per wave.
#pragma once

#include <cstddef>
#include <cstdint>

#include "pbf_hip.h"

namespace wwsolids {

// PBF_OK, or PBF_ERR_INVALID with *why (may be NULL) naming the condition
inline int check(const pbf_whitewater_solids *s, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  if (!(s->restitution >= 0 && s->restitution <= 1)) return *why = "pbf_set_whitewater_solids: restitution outside [0, 1] or NaN", PBF_ERR_INVALID;
  if (!(s->friction >= 0 && s->friction <= 1)) return *why = "pbf_set_whitewater_solids: friction outside [0, 1] or NaN", PBF_ERR_INVALID;
  if (s->reserved != 0) return *why = "pbf_set_whitewater_solids: reserved != 0", PBF_ERR_INVALID;
  return PBF_OK;
}

// workgroups of k_ww_solids_children: a grid-stride pass, the bound is the device's
constexpr uint32_t CHILD_BLOCKS = 64;

}  // namespace wwsolids

#if defined(__HIP__)
#include "pbf_collider.hpp"
#include "pbf_whitewater.hpp"

namespace pbf {

// the device's image of pbf_whitewater_solids_stats (pbf_hip.hip asserts that the two agree)
struct WwSolidsRecord {
  unsigned long long hitCollider, hitScenery, absorbed, bornInside, step;
};

// what both kernels need about the solids, by value
template <typename N> struct WwSolidsArgs {
  ColliderSdf<N> collider, scenery;  // (phi == NULL where the instantiation does not read it)
  const ColliderPose<N> *pose;       // POSED or VEL
  const double *vw;                  // VEL: V.xyz, W.xyz — the body's state or the friction record's
  ColliderFrame<N> frame;
  N e, f;
  uint32_t absorb;
};

// the two position contracts on q: q1, q2, hit1, hit2
template <typename N, bool COL, bool POSED, bool SCN>
__device__ __forceinline__ void ww_solids_project(const WwSolidsArgs<N> &a, const N q[3], N q1[3], N q2[3], bool &hit1, bool &hit2) {
  const ColliderFrame<N> &fr = a.frame;
  q1[0] = q[0], q1[1] = q[1], q1[2] = q[2];
  hit1 = false;
  if constexpr (COL) {
    if constexpr (POSED) hit1 = collider_project_posed<N>(a.collider, a.pose, fr.scale, fr.minB, fr.maxB, q1[0], q1[1], q1[2], nullptr);
    else hit1 = collider_project<N>(a.collider, fr.scale, fr.minB, fr.maxB, q1[0], q1[1], q1[2], nullptr);
  }
  q2[0] = q1[0], q2[1] = q1[1], q2[2] = q1[2];
  hit2 = false;
  if constexpr (SCN) hit2 = collider_project<N>(a.scenery, fr.scale, fr.minB, fr.maxB, q2[0], q2[1], q2[2], nullptr);
}

// response(d, vb) of the contract on v
template <typename N>
__device__ __forceinline__ void ww_solids_respond(bool hit, N dx, N dy, N dz, N bx, N by, N bz, N e, N omf, N &vx, N &vy, N &vz) {
  const N len = sqrt((dx * dx + dy * dy) + dz * dz);
  const bool act = hit && len > N(0);
  const N nx = dx / len, ny = dy / len, nz = dz / len;
  const N ux = vx - bx, uy = vy - by, uz = vz - bz;
  const N un = (ux * nx + uy * ny) + uz * nz;
  const N tx = ux - un * nx, ty = uy - un * ny, tz = uz - un * nz;
  const bool go = act && un < N(0);
  const N k = e * un;
  const N rx = (bx + omf * tx) - k * nx, ry = (by + omf * ty) - k * ny, rz = (bz + omf * tz) - k * nz;
  vx = go ? rx : vx, vy = go ? ry : vy, vz = go ? rz : vz;
}

// the workgroup's count of `flag` over its lanes (every lane of the workgroup calls it); valid in thread 0
template <int K> __device__ __forceinline__ void ww_solids_count(const bool (&flag)[K], uint32_t (&total)[K]) {
  __shared__ uint32_t waves[BLOCK / 64][K];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t mine[K];
  for (int k = 0; k < K; ++k) mine[k] = uint32_t(__popcll(__ballot(flag[k])));
  __syncthreads();  // (protects `waves` across back-to-back calls)
  if (lane == 0)
    for (int k = 0; k < K; ++k) waves[wave][k] = mine[k];
  __syncthreads();
  for (int k = 0; k < K; ++k) {
    total[k] = 0;
    for (int w = 0; w < BLOCK / 64; ++w) total[k] += waves[w][k];
  }
}

// the pass: one lane per diffuse particle, in place, after k_ww_advect.  partials: 3 words per workgroup.
template <typename N, bool COL, bool POSED, bool VEL, bool SCN>
__global__ __launch_bounds__(BLOCK) void k_ww_solids(WwSolidsArgs<N> a, uint32_t m, WwPool<N> pool, const N *__restrict__ weight,
                                                     const uint32_t *__restrict__ count, uint32_t *__restrict__ alive,
                                                     uint32_t *__restrict__ partials) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  bool flag[3] = {false, false, false};  // hit1, hit2, absorbed
  if (i < m && alive[i] != 0u) {
    const N scale = a.frame.scale;
    const vec4<N> p = pool.pos4[i];
    const N q[3] = {p.x / scale, p.y / scale, p.z / scale};
    N q1[3], q2[3];
    ww_solids_project<N, COL, POSED, SCN>(a, q, q1, q2, flag[0], flag[1]);
    if (flag[0] || flag[1]) {
      vec4<N> v = pool.vel4[i];
      const N omf = N(1) - a.f;
      if constexpr (COL) {
        N bx = N(0), by = N(0), bz = N(0);
        if constexpr (VEL) {
          const N Vx = N(a.vw[0]), Vy = N(a.vw[1]), Vz = N(a.vw[2]), Wx = N(a.vw[3]), Wy = N(a.vw[4]), Wz = N(a.vw[5]);
          const N rx = q1[0] * scale - a.pose->trans[0], ry = q1[1] * scale - a.pose->trans[1], rz = q1[2] * scale - a.pose->trans[2];
          const N cx = Wy * rz - Wz * ry, cy = Wz * rx - Wx * rz, cz = Wx * ry - Wy * rx;
          bx = (Vx + cx) / scale, by = (Vy + cy) / scale, bz = (Vz + cz) / scale;
        }
        ww_solids_respond<N>(flag[0], q1[0] - q[0], q1[1] - q[1], q1[2] - q[2], bx, by, bz, a.e, omf, v.x, v.y, v.z);
      }
      if constexpr (SCN)
        ww_solids_respond<N>(flag[1], q2[0] - q1[0], q2[1] - q1[1], q2[2] - q1[2], N(0), N(0), N(0), a.e, omf, v.x, v.y, v.z);
      const N x = min(a.frame.maxB[0], max(a.frame.minB[0], q2[0] * scale)), y = min(a.frame.maxB[1], max(a.frame.minB[1], q2[1] * scale)),
              z = min(a.frame.maxB[2], max(a.frame.minB[2], q2[2] * scale));
      pool.pos4[i] = make_vec4<N>(x, y, z, p.w);
      pool.vel4[i] = v;
      if (a.absorb != 0u) {
        const uint32_t nF = weight[i] == N(0) ? 0u : count[2 * size_t(i)];
        flag[2] = nF == 0u;
        if (flag[2]) alive[i] = 0u;
      }
    }
  }
  uint32_t total[3];
  ww_solids_count<3>(flag, total);
  if (threadIdx.x == 0) partials[3u * blockIdx.x] = total[0], partials[3u * blockIdx.x + 1u] = total[1], partials[3u * blockIdx.x + 2u] = total[2];
}

// the children: slots [survivors, survivors + emitted) of the new pool, the bound formed as k_ww_final forms it.
// gridDim.x = wwsolids::CHILD_BLOCKS; partials: 1 word per workgroup.
template <typename N, bool COL, bool POSED, bool SCN>
__global__ __launch_bounds__(BLOCK) void k_ww_solids_children(WwSolidsArgs<N> a, uint32_t n, const uint32_t *__restrict__ emit,
                                                              const uint32_t *__restrict__ offset, uint32_t m,
                                                              const uint32_t *__restrict__ alive, const uint32_t *__restrict__ aliveOffset,
                                                              uint32_t capacity, vec4<N> *__restrict__ pos4, uint32_t *__restrict__ partials) {
  const uint32_t survivors = m ? aliveOffset[m - 1u] + alive[m - 1u] : 0u;
  const uint32_t wanted = n ? offset[n - 1u] + emit[n - 1u] : 0u;
  const uint32_t room = capacity - survivors, emitted = wanted < room ? wanted : room;
  uint32_t born = 0;
  // (uniform over the workgroup.  emitted <= capacity < 2^31, pbf_whitewater_configure's bound, and a stride is
  // CHILD_BLOCKS * BLOCK = 2^14: base never wraps in 32 bits)
  for (uint32_t base = blockIdx.x * BLOCK; base < emitted; base += gridDim.x * BLOCK) {
    const uint32_t k = base + threadIdx.x;
    bool flag[1] = {false};
    if (k < emitted) {
      const size_t slot = size_t(survivors) + k;  // (< capacity)
      const N scale = a.frame.scale;
      const vec4<N> p = pos4[slot];
      const N q[3] = {p.x / scale, p.y / scale, p.z / scale};
      N q1[3], q2[3];
      bool h1, h2;
      ww_solids_project<N, COL, POSED, SCN>(a, q, q1, q2, h1, h2);
      flag[0] = h1 || h2;
      if (flag[0])
        pos4[slot] = make_vec4<N>(min(a.frame.maxB[0], max(a.frame.minB[0], q2[0] * scale)), min(a.frame.maxB[1], max(a.frame.minB[1], q2[1] * scale)),
                                  min(a.frame.maxB[2], max(a.frame.minB[2], q2[2] * scale)), p.w);
    }
    uint32_t total[1];
    ww_solids_count<1>(flag, total);
    born += total[0];
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = born;
}

// ONE workgroup: the partial records of both kernels summed into the device record.  nbPool / nbChild = 0 when that kernel
// did not run.  `step` = whitewater steps since the setting was turned on, this one included.
__global__ __launch_bounds__(BLOCK) void k_ww_solids_fold(uint32_t nbPool, const uint32_t *__restrict__ poolPartials, uint32_t nbChild,
                                                          const uint32_t *__restrict__ childPartials, unsigned long long step,
                                                          WwSolidsRecord *__restrict__ rec) {
  uint32_t s[4] = {0, 0, 0, 0}, t[4];
  for (uint32_t b = threadIdx.x; b < nbPool; b += BLOCK) s[0] += poolPartials[3u * b], s[1] += poolPartials[3u * b + 1u], s[2] += poolPartials[3u * b + 2u];
  for (uint32_t b = threadIdx.x; b < nbChild; b += BLOCK) s[3] += childPartials[b];
  for (int k = 0; k < 4; ++k) block_excl_scan(s[k], &t[k]);
  if (threadIdx.x != 0) return;
  rec->hitCollider = t[0], rec->hitScenery = t[1], rec->absorbed = t[2], rec->bornInside = t[3], rec->step = step;
}

}  // namespace pbf
#endif
