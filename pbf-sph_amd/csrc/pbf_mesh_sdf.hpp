// pbf_mesh_sdf.hpp — the device half of the mesh collider (pbf_sdf_from_mesh / pbf_set_collider_mesh, include/pbf_hip.h):
// the signed distance from every node of a lattice to a closed triangle mesh, an all-pairs fold over the records that
// csrc/pbf_mesh_records.hpp builds.  Opt-in and never part of a step.
//
// The field (the same text as the header's).  Everything is in N, in the order written, not contracted;
// PBF_FLAG_FAST_MATH does not reach it; divides and the square root are IEEE.  u . v = (u_x v_x + u_y v_y) + u_z v_z.
//   p_a = origin_a + N(i_a) * N(spacing)
//   per triangle {a, b, c, fu, e_ab, e_bc, e_ca, n_a, n_b, n_c} (Ericson, Real-Time Collision Detection, 5.1.5):
//     ab = b - a   ac = c - a   ap = p - a   bp = p - b   cp = p - c   cb = c - b
//     d1 = ab . ap   d2 = ac . ap   d3 = ab . bp   d4 = ac . bp   d5 = ab . cp   d6 = ac . cp
//     vc = d1 d4 - d3 d2     vb = d5 d2 - d1 d6     va = d3 d6 - d5 d4     e = d4 - d3     f = d5 - d6
//     the first region that holds, in this order, gives the closest point q and the normal n:
//       vertex a   d1 <= 0 && d2 <= 0                q = a                                   n = n_a
//       vertex b   d3 >= 0 && d4 <= d3               q = b                                   n = n_b
//       edge ab    vc <= 0 && d1 >= 0 && d3 <= 0     t = d1 / (d1 - d3)     q = a + t ab     n = e_ab
//       vertex c   d6 >= 0 && d5 <= d6               q = c                                   n = n_c
//       edge ca    vb <= 0 && d2 >= 0 && d6 <= 0     t = d2 / (d2 - d6)     q = a + t ac     n = e_ca
//       edge bc    va <= 0 && e >= 0 && f >= 0       t = e / (e + f)        q = b + t cb     n = e_bc
//       face       otherwise     den = (va + vb) + vc   v = vb / den   w = vc / den   q = (a + v ab) + w ac   n = fu
//     r = p - q     d2 = r . r     s = r . n     neg = s < 0
//   the fold over triangles in ascending index: a triangle replaces {best, neg} only when d2 < best, strictly (best starts at
//   +inf, neg at false; a NaN d2 never replaces), so the lowest index among ties wins
//   phi = (neg != negate) ? -sqrt(best) : sqrt(best)
// Every candidate is a value and the result a chain of selects: no lane branches, and the 0 / 0 of a region that did not
// hold is dropped by the select that rejects it.  The kernel forms ONE quotient pair for the four candidates that divide:
// it selects the numerator, the denominator, the base point and the direction of the region that holds among {edge ab, edge
// ca, edge bc, face} and then computes q = base + (num / den) dir (and, for the face, + (vc / den) ac).  The operands of the
// selected region are the ones written above, so the bits are those of computing all four candidates and selecting.
//
// The shape.  One lane per node, one wave per 4 x 4 x 4 brick of nodes (lane = 16 x + 4 y + z), four bricks per workgroup.
// The triangle index is the same in every lane of a launch, so a record is one address for the whole wave: the loads are
// from read-only memory at a wave-uniform address, which the compiler issues on the scalar path (one fetch per wave, the
// values arrive in SGPRs) — nothing is fetched per lane and nothing is staged.  Lanes of a partial brick (dims no multiple of
// 4) compute on their out-of-range coordinates, store nothing and are left out of the cull's vote and of the pair count.
//
// The cull ("sdf_cull" 1).  Each triangle has a bounding sphere {m, R} (csrc/pbf_mesh_records.hpp, build_bounds).  Every 16
// triangles a lane refreshes sb = sqrt(best); a stale sb is only larger than the current one.  The wave skips a triangle when
// every lane of the brick that holds a node finds
//       |p - m|^2 > (R + sb)^2 * (1 + 16 eps)                                   (eps = the unit round-off of N)
// The skip is safe under rounding.  R was rounded up from the exact radius widened by a relative 2^-20 and by the absolute
// pad = 64 eps M, M = the largest |coordinate| of any lattice node or vertex.  The computed closest point q is a convex
// combination of a, b, c up to a few ulps of M (t, v, w lie in [0, 1] up to a rounding; each product and sum adds at most
// eps M), so |q - m| <= R_exact + 8 eps M, and r = p - q carries at most another eps M per component.  The left side is
// |p - m|^2 (1 + 3 eps) at worst, the right side at least ((R + sb)^2)(1 + 13 eps) in exact terms, so a lane that votes
// "skip" has |p - m| > (R + sb)(1 + 5 eps), hence |p - q| >= |p - m| - |q - m| > sb (1 + 5 eps) + 64 eps M - 8 eps M, and the
// computed d2 >= (|p - q| - 2 eps M)^2 (1 - 3 eps) > sb^2 (1 + 6 eps) >= best.  So a skipped triangle could not have replaced
// the lane's best, ties included (d2 is strictly above it): the fold's result is bit for bit the all-pairs one.  A lane whose
// best is still +inf, or any NaN, compares false and votes "test".
//
// Counts.  Each wave adds (nodes of its brick) x (triangles it tested) to its own slot of `tested` with an ordinary vector
// store from lane 0; the host sums the slots.  No atomics anywhere.
//
// Launch size.  The fold is in index order, so the host splits it over triangle ranges [t0, t1): best stays in the output
// lattice and neg in a byte per node between launches, and the last launch writes phi.  The host keeps a launch to at most
// 2^33 lane-triangle pairs (launch_fold below), never fewer than 16 triangles: 28 ms in float and 61 ms in double per launch
// with every pair tested, a fifth of that with the cull (profiles/mesh_sdf.md).  "sdf_launch_pairs" (pbf_set_option) lowers
// the cap so that a test reaches the split on a small lattice.
//
// SOUP = true is the distance alone, for the 9-value records of a triangle soup (csrc/pbf_mesh_records.hpp,
// build_soup_records): the same expressions in the same order and the same strict <, no normal loads and no s.  Its sign
// comes from the winding number (csrc/pbf_mesh_winding.hpp), which reads `best` from the lattice, so the host never asks
// this instantiation for the last launch's phi.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

#include "pbf_mesh_records.hpp"

namespace meshsdf {

template <typename N> struct V3 {
  N x, y, z;
};
template <typename N> __device__ inline V3<N> vsub(V3<N> u, V3<N> v) { return {u.x - v.x, u.y - v.y, u.z - v.z}; }
template <typename N> __device__ inline N vdot(V3<N> u, V3<N> v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
template <typename N> __device__ inline V3<N> vsel(bool c, V3<N> u, V3<N> v) { return {c ? u.x : v.x, c ? u.y : v.y, c ? u.z : v.z}; }
template <typename N> __device__ inline V3<N> vload(const N *__restrict__ r) { return {r[0], r[1], r[2]}; }

template <typename N> struct SdfLattice {
  uint32_t dims[3], bricks[3];  // nodes and 4-node bricks per axis
  N origin[3], spacing;
};

constexpr uint32_t SDF_REFRESH = 16;  // triangles between two refreshes of the cull's sqrt(best)

template <typename N, bool CULL, bool SOUP = false>
__global__ __launch_bounds__(256) void k_mesh_sdf(SdfLattice<N> L, const N *__restrict__ rec, const N *__restrict__ bnd, uint32_t t0,
                                                  uint32_t t1, uint32_t first, uint32_t last, uint32_t negate, N slack,
                                                  N *__restrict__ out, uint8_t *__restrict__ sign,
                                                  unsigned long long *__restrict__ tested) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t brick = blockIdx.x * 4u + (threadIdx.x >> 6);  // wave-uniform
  if (brick >= L.bricks[0] * L.bricks[1] * L.bricks[2]) return;
  const uint32_t bz = brick % L.bricks[2], by = (brick / L.bricks[2]) % L.bricks[1], bx = brick / (L.bricks[2] * L.bricks[1]);
  const uint32_t i = bx * 4u + (lane >> 4), j = by * 4u + ((lane >> 2) & 3u), k = bz * 4u + (lane & 3u);
  const bool active = i < L.dims[0] && j < L.dims[1] && k < L.dims[2];
  const uint32_t node = (i * L.dims[1] + j) * L.dims[2] + k;  // (< 2^31 when active)
  const V3<N> p{L.origin[0] + N(i) * L.spacing, L.origin[1] + N(j) * L.spacing, L.origin[2] + N(k) * L.spacing};

  N best = N(INFINITY);
  bool neg = false;
  if (!first && active) best = out[node], neg = sign[node] != 0;
  N sb = N(INFINITY);
  uint32_t ran = 0;  // wave-uniform: triangles this wave tested

  for (uint32_t t = t0; t < t1; ++t) {
    if constexpr (CULL) {
      if (((t - t0) % SDF_REFRESH) == 0u) sb = sqrt(best);
      const N *__restrict__ s = bnd + 4u * size_t(t);
      const V3<N> dm = vsub(p, vload(s));
      const N reach = s[3] + sb;
      const bool far = vdot(dm, dm) > (reach * reach) * slack;
      if (__ballot(active && !far) == 0ull) continue;
    }
    ++ran;
    const N *__restrict__ r = rec + (SOUP ? 9u : 30u) * size_t(t);
    const V3<N> a = vload(r), b = vload(r + 3), c = vload(r + 6);
    const V3<N> ab = vsub(b, a), ac = vsub(c, a), cb = vsub(c, b);
    const V3<N> ap = vsub(p, a), bp = vsub(p, b), cp = vsub(p, c);
    const N d1 = vdot(ab, ap), d2 = vdot(ac, ap), d3 = vdot(ab, bp), d4 = vdot(ac, bp), d5 = vdot(ab, cp), d6 = vdot(ac, cp);
    const N vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const N e = d4 - d3, f = d5 - d6;
    const bool inA = d1 <= N(0) && d2 <= N(0);
    const bool inB = d3 >= N(0) && d4 <= d3;
    const bool inAB = vc <= N(0) && d1 >= N(0) && d3 <= N(0);
    const bool inC = d6 >= N(0) && d5 <= d6;
    const bool inCA = vb <= N(0) && d2 >= N(0) && d6 <= N(0);
    const bool inBC = va <= N(0) && e >= N(0) && f >= N(0);
    // the region that holds among the four that divide (the vertex regions override below)
    const bool selCA = !inAB && inCA, selBC = !inAB && !inCA && inBC, face = !inAB && !inCA && !inBC;
    const N num = inAB ? d1 : selCA ? d2 : selBC ? e : vb;
    const N denAB = d1 - d3, denCA = d2 - d6, denBC = e + f, denF = (va + vb) + vc;  // (values first: selects, no lane branches)
    const N den = inAB ? denAB : selCA ? denCA : selBC ? denBC : denF;
    const N q1 = num / den, q2 = vc / den;
    const V3<N> base = vsel(selBC, b, a), dir = vsel(selCA, ac, vsel(selBC, cb, ab));
    const V3<N> q0{base.x + q1 * dir.x, base.y + q1 * dir.y, base.z + q1 * dir.z};
    const V3<N> qf{q0.x + q2 * ac.x, q0.y + q2 * ac.y, q0.z + q2 * ac.z};
    const bool useC = inC && !inAB;
    const V3<N> q = vsel(inA, a, vsel(inB, b, vsel(useC, c, vsel(face, qf, q0))));
    const V3<N> rr = vsub(p, q);
    const N dd = vdot(rr, rr);
    const bool take = dd < best;
    best = take ? dd : best;
    if constexpr (!SOUP) {
      const V3<N> n = vsel(inA, vload(r + 21), vsel(inB, vload(r + 24), vsel(useC, vload(r + 27),
                      vsel(inAB, vload(r + 12), vsel(selCA, vload(r + 18), vsel(selBC, vload(r + 15), vload(r + 9)))))));
      const N sn = vdot(rr, n);
      const bool below = sn < N(0);
      neg = take ? below : neg;
    }
  }

  const unsigned long long nodes = __popcll(__ballot(active));
  if (lane == 0u) {
    tested[brick] = (first ? 0ull : tested[brick]) + nodes * ran;
  }
  if (!active) return;
  if (last) {
    const N d = sqrt(best);
    out[node] = (neg != (negate != 0u)) ? -d : d;
  } else {
    out[node] = best;
    sign[node] = neg ? 1 : 0;
  }
}

// ---- host side: what pbf_sdf_from_mesh / pbf_set_collider_mesh (csrc/pbf_hip.hip) and tools/mesh_sdf_rate.hip share ----------

// The lattice as the kernel takes it, the cull's bounding spheres (4 nt values) and its relative slack, from the records.
// `stride` = values per record: RECORD, or SOUP_RECORD for a soup.
template <typename N>
void prepare(const uint32_t dims[3], const double origin[3], double spacing, const N *rec, size_t nt, int stride, SdfLattice<N> *L, N *bnd,
             N *slack) {
  double reach = 0;  // M: the largest |coordinate| of a node or a vertex
  for (int a = 0; a < 3; ++a) {
    L->dims[a] = dims[a], L->bricks[a] = (dims[a] + 3u) / 4u, L->origin[a] = N(origin[a]);
    reach = std::max({reach, std::fabs(origin[a]), std::fabs(origin[a] + double(dims[a] - 1u) * spacing)});
  }
  L->spacing = N(spacing);
  for (size_t k = 0; k < nt; ++k)
    for (int v = 0; v < 9; ++v) reach = std::max(reach, std::fabs(double(rec[size_t(stride) * k + v])));
  const double eps = double(std::numeric_limits<N>::epsilon()) / 2;
  build_bounds<N>(rec, nt, stride, 64 * eps * reach, bnd);
  *slack = N(1) + N(16 * eps);
}
template <typename N> size_t brick_count(const SdfLattice<N> &L) { return size_t(L.bricks[0]) * L.bricks[1] * L.bricks[2]; }

constexpr uint64_t SDF_PAIRS_PER_LAUNCH = uint64_t(1) << 33;

// triangles per launch under a cap of `pairs` lane-triangle pairs (0 = `fallback`), never fewer than SDF_REFRESH
inline uint64_t triangles_per_launch(size_t bricks, uint64_t pairs, uint64_t fallback) {
  return std::max<uint64_t>(SDF_REFRESH, (pairs ? pairs : fallback) / (uint64_t(bricks) * 64u));
}

// The whole fold, enqueued on `stream`: rec / bnd / out (N[nodes]) / sign (a byte per node) / tested (a uint64 per brick) are
// device pointers; `pairs` = the cap on lane-triangle pairs per launch (0 = SDF_PAIRS_PER_LAUNCH).  soup: rec holds 9-value
// records and out is left holding best, not phi (csrc/pbf_mesh_winding.hpp finishes it).  Returns the launches' error.
template <typename N>
hipError_t launch_fold(hipStream_t stream, const SdfLattice<N> &L, const N *rec, const N *bnd, size_t nt, bool cull, bool negate, N slack,
                       N *out, uint8_t *sign, unsigned long long *tested, uint64_t pairs = 0, bool soup = false) {
  const size_t bricks = brick_count(L);
  const uint64_t perLaunch = triangles_per_launch(bricks, pairs, SDF_PAIRS_PER_LAUNCH);
  const dim3 grid(unsigned((bricks + 3) / 4)), block(256);
  auto *kernel = soup ? (cull ? k_mesh_sdf<N, true, true> : k_mesh_sdf<N, false, true>) : (cull ? k_mesh_sdf<N, true> : k_mesh_sdf<N, false>);
  for (uint64_t t0 = 0; t0 < nt; t0 += perLaunch) {
    const uint32_t t1 = uint32_t(std::min<uint64_t>(nt, t0 + perLaunch)), first = t0 == 0, last = !soup && t1 == nt;
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, L, rec, bnd, uint32_t(t0), t1, first, last, uint32_t(negate), slack, out, sign, tested);
  }
  return hipGetLastError();
}

}  // namespace meshsdf
