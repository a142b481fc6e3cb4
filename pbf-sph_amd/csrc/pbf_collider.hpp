// pbf_collider.hpp — static signed-distance collider (pbf_set_collider, include/pbf_hip.h): ONE device function, shared by
// DeltaOp::end (csrc/pbf_kernels.hpp) and the sample kernel behind pbf_collider_sample.
//
// The contract (the same text as the header's).  Everything is in N, in the order written, not contracted (the library is
// built with -ffp-contract=off); PBF_FLAG_FAST_MATH does not reach it.  The input is the q that DeltaOp::end computes
// without a collider: after the world-frame box clamp and the division by scale.
//
//   w_a = q_a * scale                         u_a = (w_a - origin_a) * inv
//   inside = for every a: u_a >= 0 && u_a <= N(dims_a - 1)            (NaN compares false: outside)
//   i_a = min(int(u_a), dims_a - 2)           f_a = u_a - N(i_a)       (the last node: i = dims - 2, f = 1)
//   c[x][y][z] = the eight nodes (i_x + x, i_y + y, i_z + z)
//   d[x][y]  = c[x][y][1] - c[x][y][0]        cz[x][y] = c[x][y][0] + f_z * d[x][y]
//   e[x]     = cz[x][1] - cz[x][0]            cy[x]    = cz[x][0] + f_y * e[x]
//   g_x = cy[1] - cy[0]                       phi = cy[0] + f_x * g_x
//   g_y = e[0] + f_x * (e[1] - e[0])
//   t[x] = d[x][0] + f_y * (d[x][1] - d[x][0])     g_z = t[0] + f_x * (t[1] - t[0])
//   len = sqrt((g_x g_x + g_y g_y) + g_z g_z)       (IEEE sqrt)
//   hit = inside && phi < margin && len > 0
//   s = (margin - phi) / len                         (IEEE divide)
//   q'_a = hit ? min(maxB_a / scale, max(minB_a / scale, (w_a + s * g_a) / scale)) : q_a
//
// g is the gradient of the trilinear interpolant in lattice units: the spacing is isotropic, so only its direction matters.
// A particle that does not hit keeps its q bit for bit (a select).  The second clamp uses the images of the box under the
// stock clamp, so the box always wins over the collider.  One projection runs per delta-p iteration; the K iterations
// converge it.  There is no restitution term, and friction is a pass of its own (csrc/pbf_collider_friction.hpp): finalise
// derives the velocity from the projected position, as it does for the box.
//
// With a pose (pbf_set_collider_pose; the same text as the header's) the lattice is read in a body frame, a world point
// being w = R b + t.  Everything is in N, in the order written, not contracted; PBF_FLAG_FAST_MATH does not reach it.
//
//   w_a  = q_a * scale                         d_a = w_a - t_a
//   b_a  = (R[0][a] d_0 + R[1][a] d_1) + R[2][a] d_2                 (R^T d)
//   u_a  = (b_a - origin_a) * inv
//   ... inside, i, f, the eight nodes, phi, g, len, hit, s: exactly the static contract, on u ...
//   b'_a = b_a + s * g_a
//   w'_a = ((R[a][0] b'_0 + R[a][1] b'_1) + R[a][2] b'_2) + t_a
//   q'_a = hit ? min(maxB_a / scale, max(minB_a / scale, w'_a / scale)) : q_a
//
// A particle that does not hit keeps its bits; outside the lattice, NaN included, nothing is loaded.  The margin and the
// spacing are lengths, so a rotation leaves them alone; the box is the world's, so the second clamp is not rotated.  With
// the identity pose every value compares equal to the static function's (x * 1, + 0 and - 0 are exact; a zero may change
// its sign, and an infinite coordinate becomes a NaN, which is outside as well).
//
// With scenery (pbf_set_scenery; the same text as the header's): a second, STATIC lattice in the world frame beside the
// collider.  Everything is in N, in the order written, not contracted; PBF_FLAG_FAST_MATH does not reach it.  q is the input
// of the static contract: after the world-frame box clamp and the division by scale.
//
//   scenery alone (no collider lattice):  q' = the static contract on q with the scenery's lattice — exactly the kernels and
//                                         arguments pbf_set_collider with that lattice would run
//   collider and scenery together:        q1 = the POSED contract on q with the collider's lattice (the pose record holds the
//                                              identity while no pose is set: a zero may change its sign); the reaction
//                                              record is updated from (q, q1) exactly as DeltaOp<.., COLLIDE_REACT> does
//                                         q2 = the static contract on q1 with the scenery's lattice
//
// q2 is stored, and the quantised copy is formed from it.  The scenery writes no record: A, B and hits describe the
// collider's push alone, with r taken at q1, so the friction pass, the body stage and pbf_collider_reaction see exactly what
// they would see without scenery for the same q.  The scenery comes last, so where both press on a particle the static wall
// wins, and the box wins over both through each projection's own second clamp; the K iterations converge the rest.  A lane
// that hits neither keeps its bits.  Obstacles and ghost copies are never moved.  collider_eval / collider_project below are
// used as they stand: there is no second copy of the trilinear code.
//
// The eight lattice loads are scalar-per-lane gathers from a read-only array that is small against L2 and shared by every
// wave of the launch (neighbouring particles read neighbouring nodes): plain loads, nothing staged.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// the lattice as the kernels see it: phi == NULL means no collider
template <typename N> struct ColliderSdf {
  const N *phi;      // device, N[dims product], node (i, j, k) at (i * dims[1] + j) * dims[2] + k
  uint32_t dims[3];  // nodes per axis, each >= 2, product < 2^31
  N origin[3];       // world position of node (0, 0, 0)
  N inv;             // N(1) / N(spacing)
  N margin;          // fluid is kept at phi >= margin
};

// the pose of pbf_set_collider_pose as the posed kernels read it: ONE record in a small device allocation of the ctx, rounded
// to N.  They take a pointer to it and not the values: a captured step holds its arguments, so a pose that travelled in them
// would mean a recapture per frame.  The address is the same for every lane, so the twelve loads can go the scalar path.
template <typename N> struct ColliderPose {
  N rot[9];    // row-major R, body -> world
  N trans[3];  // t, world
};

// the static contract from u to s, at the point (bx, by, bz) in the lattice's frame.  Returns inside; outside nothing is
// loaded and only *phiOut (may be NULL; +inf) is written.
template <typename N>
__device__ __forceinline__ bool collider_eval(const ColliderSdf<N> &s, N bx, N by, N bz, N *phiOut, bool &hit, N &k, N &gx, N &gy, N &gz) {
  const N *__restrict__ lat = s.phi;
  const N ux = (bx - s.origin[0]) * s.inv, uy = (by - s.origin[1]) * s.inv, uz = (bz - s.origin[2]) * s.inv;
  const bool inside = ux >= N(0) && ux <= N(s.dims[0] - 1u) && uy >= N(0) && uy <= N(s.dims[1] - 1u) && uz >= N(0) &&
                      uz <= N(s.dims[2] - 1u);
  if (!inside) {  // (no load: an outside u indexes nothing)
    if (phiOut) *phiOut = N(INFINITY);
    return false;
  }
  const uint32_t ix = min(uint32_t(ux), s.dims[0] - 2u), iy = min(uint32_t(uy), s.dims[1] - 2u), iz = min(uint32_t(uz), s.dims[2] - 2u);
  const N fx = ux - N(ix), fy = uy - N(iy), fz = uz - N(iz);
  // (ix + 1, iy + 1, iz + 1) <= dims - 1 each, so the largest index is the product - 1 < 2^31
  const uint32_t sy = s.dims[2], sx = s.dims[1] * s.dims[2];
  const uint32_t b = (ix * s.dims[1] + iy) * s.dims[2] + iz;
  const N c000 = lat[b], c001 = lat[b + 1u], c010 = lat[b + sy], c011 = lat[b + sy + 1u];
  const N c100 = lat[b + sx], c101 = lat[b + sx + 1u], c110 = lat[b + sx + sy], c111 = lat[b + sx + sy + 1u];
  const N d00 = c001 - c000, d01 = c011 - c010, d10 = c101 - c100, d11 = c111 - c110;
  const N cz00 = c000 + fz * d00, cz01 = c010 + fz * d01, cz10 = c100 + fz * d10, cz11 = c110 + fz * d11;
  const N e0 = cz01 - cz00, e1 = cz11 - cz10;
  const N cy0 = cz00 + fy * e0, cy1 = cz10 + fy * e1;
  gx = cy1 - cy0;
  const N phi = cy0 + fx * gx;
  gy = e0 + fx * (e1 - e0);
  const N t0 = d00 + fy * (d01 - d00), t1 = d10 + fy * (d11 - d10);
  gz = t0 + fx * (t1 - t0);
  const N len = sqrt((gx * gx + gy * gy) + gz * gz);
  if (phiOut) *phiOut = phi;
  hit = phi < s.margin && len > N(0);
  k = (s.margin - phi) / len;
  return true;
}

// q: in, the clamped position in the solver frame; out, q' (unchanged bit for bit without a hit).  Returns hit; *phiOut (may
// be NULL) receives the interpolated value, +inf outside the lattice.
template <typename N>
__device__ inline bool collider_project(const ColliderSdf<N> &s, N scale, const N *minB, const N *maxB, N &qx, N &qy, N &qz,
                                        N *phiOut) {
  const N wx = qx * scale, wy = qy * scale, wz = qz * scale;
  bool hit;
  N k, gx, gy, gz;
  if (!collider_eval<N>(s, wx, wy, wz, phiOut, hit, k, gx, gy, gz)) return false;
  const N px = min(maxB[0] / scale, max(minB[0] / scale, (wx + k * gx) / scale));
  const N py = min(maxB[1] / scale, max(minB[1] / scale, (wy + k * gy) / scale));
  const N pz = min(maxB[2] / scale, max(minB[2] / scale, (wz + k * gz) / scale));
  qx = hit ? px : qx, qy = hit ? py : qy, qz = hit ? pz : qz;
  return hit;
}

// the same with a pose: the lattice is read at b = R^T (w - t) and the projected point goes back through w' = R b' + t.
// g is a gradient in the body frame; it is b' that is rotated, so the push arrives in the world frame.
template <typename N>
__device__ inline bool collider_project_posed(const ColliderSdf<N> &s, const ColliderPose<N> *__restrict__ pose, N scale, const N *minB,
                                              const N *maxB, N &qx, N &qy, N &qz, N *phiOut) {
  const N r00 = pose->rot[0], r01 = pose->rot[1], r02 = pose->rot[2], r10 = pose->rot[3], r11 = pose->rot[4], r12 = pose->rot[5];
  const N r20 = pose->rot[6], r21 = pose->rot[7], r22 = pose->rot[8], tx = pose->trans[0], ty = pose->trans[1], tz = pose->trans[2];
  const N dx = qx * scale - tx, dy = qy * scale - ty, dz = qz * scale - tz;
  const N bx = (r00 * dx + r10 * dy) + r20 * dz, by = (r01 * dx + r11 * dy) + r21 * dz, bz = (r02 * dx + r12 * dy) + r22 * dz;
  bool hit;
  N k, gx, gy, gz;
  if (!collider_eval<N>(s, bx, by, bz, phiOut, hit, k, gx, gy, gz)) return false;
  const N cx = bx + k * gx, cy = by + k * gy, cz = bz + k * gz;
  const N wx = ((r00 * cx + r01 * cy) + r02 * cz) + tx, wy = ((r10 * cx + r11 * cy) + r12 * cz) + ty, wz = ((r20 * cx + r21 * cy) + r22 * cz) + tz;
  const N px = min(maxB[0] / scale, max(minB[0] / scale, wx / scale));
  const N py = min(maxB[1] / scale, max(minB[1] / scale, wy / scale));
  const N pz = min(maxB[2] / scale, max(minB[2] / scale, wz / scale));
  qx = hit ? px : qx, qy = hit ? py : qy, qz = hit ? pz : qz;
  return hit;
}

// pbf_set_collider_pose: one lane writes the ctx's record, in stream order with the steps before and after it.  The record
// arrives by value (no host buffer has to outlive the call) and is stored with ordinary vector stores.
template <typename N> __global__ void k_collider_pose_store(ColliderPose<N> v, ColliderPose<N> *dst) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (int k = 0; k < 9; ++k) dst->rot[k] = v.rot[k];
  for (int k = 0; k < 3; ++k) dst->trans[k] = v.trans[k];
}

// the box and scale of a pbf_params, rounded to N (pbf_collider_sample; DeltaOp::end takes them from its StepConsts)
template <typename N> struct ColliderFrame {
  N scale, minB[3], maxB[3];
};

// pbf_collider_sample: one lane per point.  points are already rounded to N (world); q = point / scale.
// pose: NULL without one (the static function)
template <typename N>
__global__ void k_collider_sample(ColliderSdf<N> s, const ColliderPose<N> *__restrict__ pose, ColliderFrame<N> f, uint32_t n,
                                  const N *__restrict__ points, N *__restrict__ phi, N *__restrict__ moved, uint8_t *__restrict__ hit) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  N qx = points[3 * i] / f.scale, qy = points[3 * i + 1] / f.scale, qz = points[3 * i + 2] / f.scale;
  N v;
  const bool h = pose ? collider_project_posed<N>(s, pose, f.scale, f.minB, f.maxB, qx, qy, qz, &v)
                       : collider_project<N>(s, f.scale, f.minB, f.maxB, qx, qy, qz, &v);
  phi[i] = v;
  moved[3 * i] = qx, moved[3 * i + 1] = qy, moved[3 * i + 2] = qz;
  hit[i] = h ? 1 : 0;
}
