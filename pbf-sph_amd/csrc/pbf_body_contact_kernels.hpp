// pbf_body_contact_kernels.hpp — the kernels of pbf_set_collider_body_contact (include/pbf_hip.h; the contract and the
// response are csrc/pbf_body_contact.hpp's): the body's surface as a point set, taken once from the collider's lattice, and
// the two launches of one contact pass.  collider_eval (csrc/pbf_collider.hpp) is used as it stands: there is no further copy
// of the trilinear code.
//
// The points (configure time): k_contact_count, the library's scan (launch_scans), k_contact_emit.  One lane per cell (i, j,
// k) of the collider's lattice whose three indices are multiples of `stride`, in the order (i * cells_y + j) * cells_z + k
// of the strided cells; contact_cell_point is the ONE expression both kernels evaluate, so what was counted is what is
// emitted, and the scan puts the points in that order.
//
// The pass (every step, `iterations` times): k_contact_partial, one lane per point in rounds of 64 like k_wrench_partial,
// DIAG_TILE points per workgroup, eight gathers from the scenery's lattice (small against L2, shared by every wave: plain
// loads); k_contact_resolve, ONE workgroup that folds the partial records BLOCK at a time in index order and whose thread 0
// runs bodycontact::resolve.  No atomics, no read-back, fixed arguments: a captured step replays them as they are.
#pragma once

#include "pbf_body_contact.hpp"
#include "pbf_kernels.hpp"

namespace pbf {

// the strided cells of a lattice
struct ContactCells {
  uint32_t cells[3];  // strided cells per axis: ceil((dims_a - 1) / stride)
  uint32_t stride;
  uint32_t lanes;     // their product (< 2^31: at most the node count)
};

// The cell of lane `l` gives a point?  s.margin is N(level).  p: the point (written only when it does).
template <typename N> __device__ inline bool contact_cell_point(const ColliderSdf<N> &s, N spacing, const ContactCells &c, uint32_t l, N *p) {
  const uint32_t kz = l % c.cells[2], t = l / c.cells[2], ky = t % c.cells[1], kx = t / c.cells[1];
  const uint32_t i[3] = {kx * c.stride, ky * c.stride, kz * c.stride};
  const uint32_t sy = s.dims[2], sx = s.dims[1] * s.dims[2];
  const uint32_t base = (i[0] * s.dims[1] + i[1]) * s.dims[2] + i[2];  // (i_a + 1 <= dims_a - 1: every index < the node count)
  bool below = false, notBelow = false, allFinite = true;
#pragma unroll
  for (uint32_t n = 0; n < 8u; ++n) {
    const N v = s.phi[base + ((n & 4u) ? sx : 0u) + ((n & 2u) ? sy : 0u) + (n & 1u)];
    allFinite = allFinite && (v - v == N(0));
    below = below || v < s.margin;
    notBelow = notBelow || v >= s.margin;
  }
  if (!allFinite || !below || !notBelow) return false;
  const N b[3] = {s.origin[0] + (N(i[0]) + N(0.5)) * spacing, s.origin[1] + (N(i[1]) + N(0.5)) * spacing,
                  s.origin[2] + (N(i[2]) + N(0.5)) * spacing};
  bool hit = false;
  N k, gx, gy, gz;
  if (!collider_eval<N>(s, b[0], b[1], b[2], nullptr, hit, k, gx, gy, gz)) return false;
  const N len = sqrt((gx * gx + gy * gy) + gz * gz);
  if (!(len > N(0))) return false;
  const N q[3] = {b[0] + k * gx, b[1] + k * gy, b[2] + k * gz};
  if (!(q[0] - q[0] == N(0)) || !(q[1] - q[1] == N(0)) || !(q[2] - q[2] == N(0))) return false;
  p[0] = q[0], p[1] = q[1], p[2] = q[2];
  return true;
}
template <typename N>
__global__ __launch_bounds__(BLOCK) void k_contact_count(ColliderSdf<N> s, N spacing, ContactCells c, uint32_t *__restrict__ counts) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= c.lanes) return;
  N p[3];
  counts[l] = contact_cell_point<N>(s, spacing, c, l, p) ? 1u : 0u;
}
template <typename N>
__global__ __launch_bounds__(BLOCK) void k_contact_emit(ColliderSdf<N> s, N spacing, ContactCells c, const uint32_t *__restrict__ offsets,
                                                        uint32_t total, N *__restrict__ points) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= c.lanes) return;
  N p[3];
  if (!contact_cell_point<N>(s, spacing, c, l, p)) return;
  const uint32_t at = offsets[l];
  if (at >= total) return;  // (never: the count pass evaluated the same expression)
  points[3u * at] = p[0], points[3u * at + 1u] = p[1], points[3u * at + 2u] = p[2];
}

// ---- the pass ----------------------------------------------------------------------------------------------------------
struct ContactPartial {
  double sum[7];  // S, M.xyz, A.xyz
  double dmax;    // D
  unsigned long long cnt;
};
__device__ inline void contact_identity(ContactPartial &p) {
  for (int k = 0; k < 7; ++k) p.sum[k] = 0.0;
  p.dmax = 0.0, p.cnt = 0ull;
}
__device__ inline void contact_fold(ContactPartial &a, const ContactPartial &b) {
  for (int k = 0; k < 7; ++k) a.sum[k] += b.sum[k];
  a.dmax = b.dmax > a.dmax ? b.dmax : a.dmax;
  a.cnt += b.cnt;
}
// wrench_block_fold's shape: the wave's lanes by an xor butterfly, the wave records through LDS in wave order
__device__ inline void contact_block_fold(ContactPartial &p, ContactPartial *waves) {
#pragma unroll 1
  for (int m = 1; m < 64; m <<= 1) {
    ContactPartial o;
    for (int k = 0; k < 7; ++k) o.sum[k] = __shfl_xor(p.sum[k], m);
    o.dmax = __shfl_xor(p.dmax, m);
    o.cnt = __shfl_xor(p.cnt, m);
    contact_fold(p, o);
  }
  if ((threadIdx.x & 63u) == 0) waves[threadIdx.x >> 6] = p;
  __syncthreads();
  if (threadIdx.x == 0)
    for (uint32_t w = 1; w < BLOCK / 64; ++w) contact_fold(p, waves[w]);
  __syncthreads();  // (the next round overwrites `waves`)
}

template <typename N>
__global__ __launch_bounds__(BLOCK) void k_contact_partial(ColliderSdf<N> s, uint32_t n, const N *__restrict__ points,
                                                           const colliderbody::Record *__restrict__ body,
                                                           const bodycontact::Record *__restrict__ contact, ContactPartial *__restrict__ partials) {
  __shared__ ContactPartial waves[BLOCK / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t waveBase = blockIdx.x * DIAG_TILE + wave * 64u * DIAG_ITEMS;
  // The skin comes from the record, not from the arguments: a captured step holds its arguments, and a changed skin is a
  // rewritten record, not a recapture.  (One address for every lane: these loads can go the scalar path.)
  s.margin = N(contact->par.skin);
  double R[9], x[3];
  for (int k = 0; k < 9; ++k) R[k] = body->st.pose.rot[k];
  for (int k = 0; k < 3; ++k) x[k] = body->st.pose.trans[k];
  ContactPartial a;
  contact_identity(a);
#pragma unroll 1
  for (int j = 0; j < DIAG_ITEMS; ++j) {
    const uint32_t i = waveBase + j * 64u + lane;
    if (i >= n) continue;
    const double b[3] = {double(points[3u * i]), double(points[3u * i + 1u]), double(points[3u * i + 2u])};
    double r[3];
    for (int c = 0; c < 3; ++c) r[c] = (R[3 * c] * b[0] + R[3 * c + 1] * b[1]) + R[3 * c + 2] * b[2];
    bool hit = false;
    N k, gx, gy, gz;
    if (!collider_eval<N>(s, N(r[0] + x[0]), N(r[1] + x[1]), N(r[2] + x[2]), nullptr, hit, k, gx, gy, gz)) continue;
    if (!hit) continue;
    const double m[3] = {double(k) * double(gx), double(k) * double(gy), double(k) * double(gz)};
    const double d = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    if (!(d > 0.0) || !(d - d == 0.0)) continue;
    a.sum[0] += d;
    for (int c = 0; c < 3; ++c) a.sum[1 + c] += m[c], a.sum[4 + c] += d * r[c];
    a.dmax = d > a.dmax ? d : a.dmax;
    a.cnt += 1ull;
  }
  contact_block_fold(a, waves);
  if (threadIdx.x == 0) partials[blockIdx.x] = a;
}

// the end of the pass's sum and its response: wrench_fold_partials' shape, then thread 0 alone
template <typename N>
__global__ __launch_bounds__(BLOCK) void k_contact_resolve(uint32_t nb, const ContactPartial *__restrict__ partials, colliderbody::Record *body,
                                                           bodycontact::Record *contact, ColliderPose<N> *pose) {
  __shared__ ContactPartial waves[BLOCK / 64];
  ContactPartial t;
  contact_identity(t);
  for (uint32_t base = 0; base < nb; base += BLOCK) {
    const uint32_t i = base + threadIdx.x;
    ContactPartial p;
    if (i < nb) p = partials[i];
    else contact_identity(p);
    contact_block_fold(p, waves);
    contact_fold(t, p);  // (thread 0's is the one that counts)
  }
  if (threadIdx.x != 0) return;
  colliderbody::Record r = *body;
  bodycontact::Record c = *contact;
  bodycontact::Sums s;
  s.S = t.sum[0], s.D = t.dmax, s.count = t.cnt;
  for (int k = 0; k < 3; ++k) s.M[k] = t.sum[1 + k], s.A[k] = t.sum[4 + k];
  bodycontact::resolve(r.par, r.st, c.par, s, c.st);
  body->st = r.st;
  contact->st = c.st;
  for (int k = 0; k < 3; ++k) pose->trans[k] = N(r.st.pose.trans[k]);
}

// pbf_set_collider_body_contact / a re-placed body: one lane writes the record (parameters, counters at zero), by value
__global__ void k_contact_store(bodycontact::Record v, bodycontact::Record *dst) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  *dst = v;
}
// struct pbf_body_contact_state into the pinned record the host polls
struct ContactStateRecord {
  struct pbf_body_contact_state st;
  uint32_t seq;
};
__global__ void k_contact_read(const bodycontact::Record *contact, volatile ContactStateRecord *host, uint32_t seq) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned long long *src = reinterpret_cast<const unsigned long long *>(&contact->st);
  volatile unsigned long long *dst = reinterpret_cast<volatile unsigned long long *>(&host->st);
  for (uint32_t k = 0; k < sizeof(struct pbf_body_contact_state) / 8; ++k) dst[k] = src[k];
  __threadfence_system();
  host->seq = seq;
  __threadfence_system();
}

}  // namespace pbf
