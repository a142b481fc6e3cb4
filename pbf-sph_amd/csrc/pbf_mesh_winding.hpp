// pbf_mesh_winding.hpp — the winding-number sign of the mesh collider (PBF_MESH_SIGN_WINDING of pbf_sdf_from_mesh /
// pbf_set_collider_mesh, and pbf_mesh_winding, include/pbf_hip.h): the generalised winding number (Jacobson, Kavan &
// Sorkine-Hornung 2013, "Robust inside-outside segmentation using generalized winding numbers", ACM TOG 32(4)) of a triangle
// soup at every node of a lattice, the solid angles by van Oosterom & Strackee 1983.  It needs no adjacency, so it signs the
// exact distance (csrc/pbf_mesh_sdf.hpp, SOUP = true) of meshes that are open, misoriented or not manifold.  Opt-in and never
// part of a step.
//
// The sign (the same text as the header's).  Everything is in N, in the order written, not contracted; PBF_FLAG_FAST_MATH
// does not reach it; sqrt and divides are IEEE.  u . v = (u_x v_x + u_y v_y) + u_z v_z.
//   p as the distance fold forms it;   a = A - p   b = B - p   c = C - p          (A, B, C: record values)
//   la = sqrt(a . a)   lb = sqrt(b . b)   lc = sqrt(c . c)
//   x = (b_y c_z - b_z c_y, b_z c_x - b_x c_z, b_x c_y - b_y c_x)      num = a . x
//   den = ((la lb) lc + (a . b) lc) + ((b . c) la + (c . a) lb)
//   S += atan2(num, den)          ascending triangle index, from S = 0
//   w = S / N(2 pi)                                   (pbf_mesh_winding's output)
//   neg = best > 0 && S > N(pi)                       (a node on the mesh keeps the existing +0 / -0 convention)
//   phi = (neg != negate) ? -sqrt(best) : sqrt(best)
// atan2 is the device library's and has no bit contract: the sign and w are held by tolerance, sqrt(best) bit for bit.
//
// The shape is k_mesh_sdf's: one lane per node, one wave per 4 x 4 x 4 brick (lane = 16 x + 4 y + z), four bricks per
// workgroup, partial bricks masked (their lanes compute on out-of-range coordinates and store nothing).  The nine record
// values sit at a wave-uniform address in read-only memory, so they come over the scalar path into SGPRs and feed the VALU
// from there; no LDS, no atomics.  Every pair is evaluated: a solid angle has no exact cull, and the far-field expansion of
// Barill et al. 2018 would change the values.  The per-pair program is branch-free: three IEEE square roots and one atan2
// dominate it (profiles/mesh_winding.md).
//
// Launch size.  The sum is in index order, so the host splits it over triangle ranges like the distance fold: S is carried in
// a per-node array of N between launches (an exact copy, so the split changes no bit) and the last launch finishes —
// FINISH_PHI reads best from the lattice and writes phi over it, FINISH_W writes w over S.  The cap of a launch is the fold's
// own, WINDING_PAIRS_PER_LAUNCH, chosen by measurement: the largest power of two that keeps a launch under the distance
// fold's 28 ms in float and 61 ms in double.  A winding pair turned out to cost about one all-pairs distance pair (3.5e11
// pairs / s in float, 1.9e11 in double), so the cap is 2^33 too: 25 ms and 44 ms per launch (profiles/mesh_winding.md).
#pragma once
#include "pbf_mesh_sdf.hpp"

namespace meshsdf {

enum : uint32_t { FINISH_NONE = 0, FINISH_PHI = 1, FINISH_W = 2 };

template <typename N>
__global__ __launch_bounds__(256) void k_mesh_winding(SdfLattice<N> L, const N *__restrict__ rec, uint32_t t0, uint32_t t1, uint32_t first,
                                                      uint32_t finish, uint32_t negate, N *__restrict__ sum, N *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t brick = blockIdx.x * 4u + (threadIdx.x >> 6);  // wave-uniform
  if (brick >= L.bricks[0] * L.bricks[1] * L.bricks[2]) return;
  const uint32_t bz = brick % L.bricks[2], by = (brick / L.bricks[2]) % L.bricks[1], bx = brick / (L.bricks[2] * L.bricks[1]);
  const uint32_t i = bx * 4u + (lane >> 4), j = by * 4u + ((lane >> 2) & 3u), k = bz * 4u + (lane & 3u);
  const bool active = i < L.dims[0] && j < L.dims[1] && k < L.dims[2];
  const uint32_t node = (i * L.dims[1] + j) * L.dims[2] + k;  // (< 2^31 when active)
  const V3<N> p{L.origin[0] + N(i) * L.spacing, L.origin[1] + N(j) * L.spacing, L.origin[2] + N(k) * L.spacing};

  N S = N(0);
  if (!first && active) S = sum[node];
  for (uint32_t t = t0; t < t1; ++t) {
    const N *__restrict__ r = rec + 9u * size_t(t);
    const V3<N> a = vsub(vload(r), p), b = vsub(vload(r + 3), p), c = vsub(vload(r + 6), p);
    const N la = sqrt(vdot(a, a)), lb = sqrt(vdot(b, b)), lc = sqrt(vdot(c, c));
    const V3<N> x{b.y * c.z - b.z * c.y, b.z * c.x - b.x * c.z, b.x * c.y - b.y * c.x};
    const N num = vdot(a, x);
    const N den = ((la * lb) * lc + vdot(a, b) * lc) + (vdot(b, c) * la + vdot(c, a) * lb);
    S += atan2(num, den);
  }
  if (!active) return;
  if (finish == FINISH_PHI) {
    const N best = out[node];
    const N d = sqrt(best);
    const bool neg = best > N(0) && S > N(3.14159265358979323846);
    out[node] = (neg != (negate != 0u)) ? -d : d;
  } else if (finish == FINISH_W) {
    sum[node] = S / N(6.28318530717958647692);
  } else {
    sum[node] = S;
  }
}

// the cap on lane-triangle pairs per launch of the winding fold (measured: profiles/mesh_winding.md)
constexpr uint64_t WINDING_PAIRS_PER_LAUNCH = uint64_t(1) << 33;

// The whole winding fold, enqueued on `stream`: rec (9-value records) / sum (N[nodes]) / out (N[nodes], holding best when
// finish == FINISH_PHI; unused otherwise) are device pointers; `pairs` = the cap per launch (0 = WINDING_PAIRS_PER_LAUNCH).
template <typename N>
hipError_t launch_winding(hipStream_t stream, const SdfLattice<N> &L, const N *rec, size_t nt, uint32_t finish, bool negate, N *sum, N *out,
                          uint64_t pairs = 0) {
  const size_t bricks = brick_count(L);
  const uint64_t perLaunch = triangles_per_launch(bricks, pairs, WINDING_PAIRS_PER_LAUNCH);
  const dim3 grid(unsigned((bricks + 3) / 4)), block(256);
  for (uint64_t t0 = 0; t0 < nt; t0 += perLaunch) {
    const uint32_t t1 = uint32_t(std::min<uint64_t>(nt, t0 + perLaunch)), first = t0 == 0;
    hipLaunchKernelGGL(k_mesh_winding<N>, grid, block, 0, stream, L, rec, uint32_t(t0), t1, first, t1 == nt ? finish : uint32_t(FINISH_NONE),
                       uint32_t(negate), sum, out);
  }
  return hipGetLastError();
}

}  // namespace meshsdf
