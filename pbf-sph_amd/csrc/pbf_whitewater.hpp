// pbf_whitewater.hpp — spray, foam and air bubbles after Ihmsen, Akinci, Akinci & Teschner 2012, "Unified spray, foam and
// air bubbles for particle-based fluids" (The Visual Computer 28), as a post-process on the resident state.  No reference
// counterpart.  pbf_whitewater_step (pbf_hip.hip) runs, on the ctx stream, never inside a step or a captured graph:
//
//   1 advect    k_sample (pbf_kernels.hpp) through WwPoolSource — the very kernel behind pbf_sample_points, so the fluid
//               neighbour count nF = count[0], `weight` and `mv` at a diffuse particle are bit for bit what
//               pbf_sample_points returns at its position — then k_ww_advect, one lane per diffuse particle;
//   2 normals   SurfaceDensityOp / SurfaceNormalOp through launch_gather into two fields of the whitewater state;
//   3 potential WhitewaterOp, one more gather over the final pStar: {I_ta, I_wc, E_k, n_d} and the child count per particle;
//   4 emit      exclusive scan of the child counts in device order (k_scan_*: no atomics), k_ww_emit writes child k of
//               parent i to slot survivors + offset_i + k, children past the capacity are dropped;
//   5 compact   exclusive scan of the survivor flags (the same scan launches, second job), k_ww_move keeps the survivors in
//               order, k_ww_final counts and hands the record to the host's pinned words (the k_drain_scan hand-over).
//
// Frames.  The fluid's pStar is in the solver frame (world / scale), pos4 in world units, and a stored velocity v is in
// solver-frame units per time: k_predict forms pStar = v dt + x / scale and k_finalise stores x = pStar * scale.  A diffuse
// particle keeps that relation: its position is stored in world units, its velocity in solver-frame units per time, and
//     xs = x / scale;  xs = v dt + xs;  x = xs * scale                                    (per component, in N)
// is what "x += dt v" means below.  The potentials are formed in the solver frame (x = pStar, h = pbf_desc.h) from the
// stored velocities.  All arithmetic in N, not contracted; excluded terms are SELECTED to +0, never multiplied by 0.
//
// Advection (g = pbf_params.constant_force; v_f = mv / weight per component, nF = 0 when the point is outside the grid or
// weight == 0; v_f is then 0):
//     spray   nF <  spray_below:   v = g dt + v
//     bubble  nF >= bubble_from:   v = (v + (dt * -k_b) g) + k_d (v_f - v)
//     foam    otherwise:           v = v_f;  life = life - dt
// then x += dt v as above, x clamped per axis as DeltaOp::end does, min(maxB, max(minB, x)).  The particle dies when
// life <= 0 (after the update), when a component of x or v is not finite, or when nF == 0 and the clamp changed a
// coordinate: it has left the fluid and hit a wall (a deviation from the paper, which keeps such spray for its lifetime).
//
// Potentials of fluid particle i over the fluid candidates j != i (by index) of its 27 predict-time cells with 0 < r <= h,
// r = |x_ij| by pair_geom (so PBF_FLAG_FAST_MATH takes its v_rsq form), x_ij = x_i - x_j, v_ij = v_i - v_j, W = 1 - r / h:
//     I_ta  = sum  |v_ij| (1 - (v_ij . x_ij) / (|v_ij| r)) W                 a term is 0 when |v_ij| == 0
//     kappa = sum over j with (x_ji . nhat_i) / r < 0 of  (1 - nhat_i . nhat_j) W       0 when n_i or n_j is zero
//     I_wc  = kappa if vhat_i . nhat_i >= 0.6, else 0                        (0 when v_i or n_i is zero)
//     E_k   = (m_i (vx^2 + vy^2 + vz^2)) * 0.5
// with n the SurfaceNormalOp field, nhat = n / |n|, |.| = sqrt of the left-to-right sum of squares.  Then
//     Phi(I, tau) = (min(I, tau[1]) - min(I, tau[0])) / (tau[1] - tau[0])
//     n_d = (Phi_k (k_ta Phi_ta + k_wc Phi_wc)) dt, selected to 0 when v_i == 0;   count_i = min(floor(n_d + u(i, 0)), 1024)
// Obstacles get a zero record and no children.
//
// Random numbers.  mix(x) = splitmix64: x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
// x = (x ^ x >> 27) * 0x94D049BB133111EB; return x ^ x >> 31.  For parent id, frame (whitewater steps since configure),
// child k and stream s:   u = (mix(seed ^ mix(id) ^ mix(frame * 2^32 + k * 4 + s)) >> 40) * 2^-24   in [0, 1), exact in N.
// count_i uses k = 0, s = 0; child k uses s = 1, 2, 3 for u1, u2, u3.
//
// Emission of child k of parent i (x_i = pos4 world, v_i stored velocity, |v_i| > 0), Ihmsen's cylinder:
//     vhat = v_i / |v_i|;  a = the unit axis of vhat's smallest |component| (x before y before z);
//     e1 = (vhat x a) / |vhat x a|;  e2 = vhat x e1;  r_V = (h * scale) * 0.5
//     r = r_V sqrt(u1);  theta = 6.283185307179586 u2;  hh = (u3 dt) |v_i|;  c = r cos(theta);  s = r sin(theta)
//     x_d = ((x_i + c e1) + s e2) + hh vhat;   v_d = (c e1 + s e2) + v_i;   life = l0 + Phi_k (l1 - l0);  parent_id = id_i
// A child's kind until its first advection is the class of its parent's count of fluid candidates within h (itself included).
#pragma once

#include "pbf_kernels.hpp"

namespace pbf {

constexpr uint8_t WW_SPRAY = 0, WW_FOAM = 1, WW_BUBBLE = 2;  // = PBF_WW_* (include/pbf_hip.h)
constexpr uint32_t WW_MAX_CHILDREN = 1024;                   // per parent and step

// the configuration in N, by value to every kernel
template <typename N> struct WwConsts {
  N kTa, kWc, tauTa[2], tauWc[2], tauK[2], life[2], kB, kD;
  uint32_t sprayBelow, bubbleFrom;
  uint64_t seed, frame;
};

// the pool: {x.xyz (world), life} {v.xyz, 0} kind parent
template <typename N> struct WwPool {
  vec4<N> *pos4, *vel4;
  uint8_t *kind;
  uint64_t *parent;
};

__device__ inline float ww_unit(uint64_t seed, uint64_t id, uint64_t frame, uint32_t k, uint32_t s) {
  const uint64_t w = splitmix64(seed ^ splitmix64(id) ^ splitmix64((frame << 32) + uint64_t(k) * 4u + s));
  return float(uint32_t(w >> 40)) * 0x1p-24f;  // 24 bits: exact in float, and in double
}

__device__ inline uint8_t ww_classify(uint32_t nF, uint32_t sprayBelow, uint32_t bubbleFrom) {
  return nF < sprayBelow ? WW_SPRAY : (nF >= bubbleFrom ? WW_BUBBLE : WW_FOAM);
}

template <typename N> __device__ inline N ww_phi(N I, const N tau[2]) { return (min(I, tau[1]) - min(I, tau[0])) / (tau[1] - tau[0]); }

// k_sample's third source: lane t owns diffuse particle t of the pool
template <typename N> struct WwPoolSource {
  const vec4<N> *pos4;
  uint32_t n;
  __device__ bool point(uint32_t &q, N &x, N &y, N &z) const {
    q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n) return false;
    const vec4<N> p = pos4[q];
    x = p.x, y = p.y, z = p.z;
    return true;
  }
};

// pass 1: one lane per diffuse particle, in place; alive[q] = 1 for a survivor (the compaction's scan input)
template <typename N>
__global__ __launch_bounds__(BLOCK) void k_ww_advect(StepConsts<N> c, WwConsts<N> w, uint32_t m, WwPool<N> pool,
                                                     const N *__restrict__ weight, const N *__restrict__ mv,
                                                     const uint32_t *__restrict__ count, uint32_t *__restrict__ alive) {
  const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
  if (q >= m) return;
  const vec4<N> p = pool.pos4[q];
  vec4<N> v = pool.vel4[q];
  const N wt = weight[q];
  const uint32_t nF = wt == N(0) ? 0u : count[2 * size_t(q)];  // (outside the grid the whole record is 0)
  const bool have = nF != 0u;
  const N fx = have ? mv[3 * size_t(q)] / wt : N(0), fy = have ? mv[3 * size_t(q) + 1] / wt : N(0),
          fz = have ? mv[3 * size_t(q) + 2] / wt : N(0);
  const uint8_t kind = ww_classify(nF, w.sprayBelow, w.bubbleFrom);
  N life = p.w;
  if (kind == WW_SPRAY) {
    v.x = c.force[0] * c.dt + v.x, v.y = c.force[1] * c.dt + v.y, v.z = c.force[2] * c.dt + v.z;
  } else if (kind == WW_BUBBLE) {
    const N b = c.dt * -w.kB;
    v.x = (v.x + b * c.force[0]) + w.kD * (fx - v.x);
    v.y = (v.y + b * c.force[1]) + w.kD * (fy - v.y);
    v.z = (v.z + b * c.force[2]) + w.kD * (fz - v.z);
  } else {
    v.x = fx, v.y = fy, v.z = fz;
    life = life - c.dt;
  }
  const N ux = (v.x * c.dt + p.x / c.scale) * c.scale, uy = (v.y * c.dt + p.y / c.scale) * c.scale,
          uz = (v.z * c.dt + p.z / c.scale) * c.scale;
  // (a NaN goes through min / max as the bound: the finiteness test below looks at the unclamped value)
  const N x = min(c.maxB[0], max(c.minB[0], ux)), y = min(c.maxB[1], max(c.minB[1], uy)), z = min(c.maxB[2], max(c.minB[2], uz));
  const bool finite = isfinite(ux) && isfinite(uy) && isfinite(uz) && isfinite(v.x) && isfinite(v.y) && isfinite(v.z);
  const bool hitWall = nF == 0u && (x != ux || y != uy || z != uz);
  const bool dead = !(life > N(0)) || !finite || hitWall;
  pool.pos4[q] = make_vec4<N>(x, y, z, life);
  pool.vel4[q] = v;
  pool.kind[q] = kind;
  alive[q] = dead ? 0u : 1u;
}

// pass 3 ----------------------------------------------------------------------------------------------------------
template <typename N> struct WwSrc {
  vec4<N> p, v, f;  // pStar, stored velocity, {n.xyz, rho} of the normal pass
  uint32_t idx, fluid;
};
template <typename N> __device__ inline void pin_registers(WwSrc<N> &b) {  // (the list readers' pipelining)
  pin_registers(b.p), pin_registers(b.v), pin_registers(b.f);
  asm volatile("" : "+v"(b.idx), "+v"(b.fluid));
}
template <typename N, bool FAST> struct WhitewaterOp {
  using Src = WwSrc<N>;
  struct Args {
    const vec4<N> *pstar, *pos4, *vel4, *field;
    const uint8_t *type;
    const uint64_t *id;
    vec4<N> *pot;       // {I_ta, I_wc, E_k, n_d}
    uint32_t *emit;     // count_i
    uint8_t *childKind;
    WwConsts<N> w;
  };
  static constexpr bool kNeedsCandidateType = false;  // (the type is read in load(): obstacles are selected away)
  static constexpr bool kFilter = true;
  static constexpr bool kTileable = false;
  __device__ static Src load(const Args &a, uint32_t b) {
    return Src{a.pstar[b], a.vel4[b], a.field[b], b, uint32_t((a.type[b] & 1) ^ 1u)};
  }
  vec4<N> pa, va;
  N nhx, nhy, nhz;  // nhat_i (0 when n_i is zero)
  N ita, kappa;
  uint32_t self, nbr;
  bool haveN;
  __device__ static N len3(N x, N y, N z) { return sqrt(x * x + y * y + z * z); }
  __device__ bool near(const StepConsts<N> &c, const Src &b) const { return maybe_within_h<N>(pa, b.p, c.h2filter); }
  __device__ bool begin(const StepConsts<N> &c, const Args &a, uint32_t i) {
    if (c.hasObstacles && a.type[i] != 0) {
      a.pot[i] = make_vec4<N>(N(0), N(0), N(0), N(0));
      a.emit[i] = 0u, a.childKind[i] = WW_SPRAY;
      return false;
    }
    pa = a.pstar[i], va = a.vel4[i];
    const vec4<N> n = a.field[i];
    const N nl = len3(n.x, n.y, n.z);
    haveN = nl > N(0);
    nhx = haveN ? n.x / nl : N(0), nhy = haveN ? n.y / nl : N(0), nhz = haveN ? n.z / nl : N(0);
    ita = kappa = N(0);
    self = i, nbr = 0u;
    return true;
  }
  __device__ void add(const StepConsts<N> &c, const Src &b) { add_bf(c, b); }
  __device__ void add_bf(const StepConsts<N> &c, const Src &b, bool valid = true) {
    const auto g = pair_geom<N, FAST>(pa, b.p, c.h);
    const bool fluidIn = g.inH && valid && b.fluid != 0u;
    // 0 < r: tested on the difference itself — sqrt_rsq's addend makes the r of a coincident pair tiny but positive
    const bool in = fluidIn && b.idx != self && (g.dx != N(0) || g.dy != N(0) || g.dz != N(0));
    const N W = N(1) - g.r / c.h;
    // trapped air
    const N vx = va.x - b.v.x, vy = va.y - b.v.y, vz = va.z - b.v.z;
    const N vm = len3(vx, vy, vz);
    const N ta = (vm * (N(1) - (vx * g.dx + vy * g.dy + vz * g.dz) / (vm * g.r))) * W;
    ita += (in && vm > N(0)) ? ta : N(0);
    // wave crest
    const N bl = len3(b.f.x, b.f.y, b.f.z);
    const N s = -(g.dx * nhx + g.dy * nhy + g.dz * nhz) / g.r;  // xhat_ji . nhat_i
    const N wc = (N(1) - (nhx * b.f.x + nhy * b.f.y + nhz * b.f.z) / bl) * W;
    kappa += (in && haveN && bl > N(0) && s < N(0)) ? wc : N(0);
    nbr += fluidIn ? 1u : 0u;
  }
  __device__ void end(const StepConsts<N> &c, const Args &a, uint32_t i) {
    const WwConsts<N> &w = a.w;
    const N v2 = va.x * va.x + va.y * va.y + va.z * va.z;
    const N vl = sqrt(v2);
    const bool moving = vl > N(0);
    const N along = (va.x * nhx + va.y * nhy + va.z * nhz) / vl;  // vhat_i . nhat_i
    const N iwc = (moving && haveN && along >= N(0.6)) ? kappa : N(0);
    const N ek = (a.pos4[i].w * v2) * N(0.5);
    const N rate = (ww_phi<N>(ek, w.tauK) * (w.kTa * ww_phi<N>(ita, w.tauTa) + w.kWc * ww_phi<N>(iwc, w.tauWc))) * c.dt;
    const N nd = moving ? rate : N(0);
    const N u = N(ww_unit(w.seed, a.id[i], w.frame, 0u, 0u));
    const N cnt = floor(nd + u);
    a.pot[i] = make_vec4<N>(ita, iwc, ek, nd);
    a.emit[i] = cnt >= N(1) ? (cnt >= N(WW_MAX_CHILDREN) ? WW_MAX_CHILDREN : uint32_t(cnt)) : 0u;  // (a NaN emits nothing)
    a.childKind[i] = ww_classify(nbr, w.sprayBelow, w.bubbleFrom);
  }
};

// pass 4: one lane per fluid particle.  survivors = the compaction's total (0 for an empty pool).
template <typename N>
__global__ __launch_bounds__(BLOCK) void k_ww_emit(StepConsts<N> c, WwConsts<N> w, const vec4<N> *__restrict__ pos4,
                                                   const vec4<N> *__restrict__ vel4, const uint64_t *__restrict__ id,
                                                   const vec4<N> *__restrict__ pot, const uint32_t *__restrict__ emit,
                                                   const uint32_t *__restrict__ offset, const uint8_t *__restrict__ childKind,
                                                   uint32_t m, const uint32_t *__restrict__ alive,
                                                   const uint32_t *__restrict__ aliveOffset, uint32_t capacity, WwPool<N> dst) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= c.n) return;
  const uint32_t cnt = emit[i];
  if (cnt == 0u) return;
  const uint64_t first = uint64_t(m ? aliveOffset[m - 1u] + alive[m - 1u] : 0u) + offset[i];
  if (first >= capacity) return;
  const vec4<N> x = pos4[i], v = vel4[i];
  const N vl = sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
  const N hx = v.x / vl, hy = v.y / vl, hz = v.z / vl;
  const N ax = fabs(hx), ay = fabs(hy), az = fabs(hz);
  const int axis = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
  const N ux = axis == 0 ? N(1) : N(0), uy = axis == 1 ? N(1) : N(0), uz = axis == 2 ? N(1) : N(0);
  N e1x = hy * uz - hz * uy, e1y = hz * ux - hx * uz, e1z = hx * uy - hy * ux;
  const N el = sqrt(e1x * e1x + e1y * e1y + e1z * e1z);
  e1x = e1x / el, e1y = e1y / el, e1z = e1z / el;
  const N e2x = hy * e1z - hz * e1y, e2y = hz * e1x - hx * e1z, e2z = hx * e1y - hy * e1x;
  const N rV = (c.h * c.scale) * N(0.5);
  const N life = w.life[0] + ww_phi<N>(pot[i].z, w.tauK) * (w.life[1] - w.life[0]);
  const uint64_t pid = id[i];
  const uint8_t kind = childKind[i];
  for (uint32_t k = 0; k < cnt; ++k) {
    const uint64_t slot = first + k;
    if (slot >= capacity) break;
    const N u1 = N(ww_unit(w.seed, pid, w.frame, k, 1u)), u2 = N(ww_unit(w.seed, pid, w.frame, k, 2u)),
            u3 = N(ww_unit(w.seed, pid, w.frame, k, 3u));
    const N r = rV * sqrt(u1), theta = N(6.283185307179586) * u2, hh = (u3 * c.dt) * vl;
    const N cs = r * cos(theta), sn = r * sin(theta);
    dst.pos4[slot] = make_vec4<N>(((x.x + cs * e1x) + sn * e2x) + hh * hx, ((x.y + cs * e1y) + sn * e2y) + hh * hy,
                                  ((x.z + cs * e1z) + sn * e2z) + hh * hz, life);
    dst.vel4[slot] = make_vec4<N>((cs * e1x + sn * e2x) + v.x, (cs * e1y + sn * e2y) + v.y, (cs * e1z + sn * e2z) + v.z, N(0));
    dst.kind[slot] = kind;
    dst.parent[slot] = pid;
  }
}

// pass 5: the survivors' records, in pool order, into the other pool set
template <typename N>
__global__ __launch_bounds__(BLOCK) void k_ww_move(uint32_t m, WwPool<N> src, const uint32_t *__restrict__ alive,
                                                   const uint32_t *__restrict__ aliveOffset, WwPool<N> dst) {
  const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
  if (q >= m || alive[q] == 0u) return;
  const uint32_t d = aliveOffset[q];  // (< m <= capacity)
  dst.pos4[d] = src.pos4[q], dst.vel4[d] = src.vel4[q], dst.kind[d] = src.kind[q], dst.parent[d] = src.parent[q];
}

// the device's image of pbf_whitewater_stats (pbf_hip.hip asserts that the two agree) + the polled word
struct WwRecord {
  unsigned long long alive, emitted, dropped, died, kind[3];
  uint32_t seq;
};

// one workgroup: the totals of the two scans, the new pool's kinds counted in a fixed order, the record handed to the host
__global__ __launch_bounds__(BLOCK) void k_ww_final(uint32_t n, const uint32_t *__restrict__ emit,
                                                    const uint32_t *__restrict__ offset, uint32_t m,
                                                    const uint32_t *__restrict__ alive, const uint32_t *__restrict__ aliveOffset,
                                                    uint32_t capacity, const uint8_t *__restrict__ kind,
                                                    volatile WwRecord *__restrict__ host, uint32_t seq) {
  const uint32_t survivors = m ? aliveOffset[m - 1u] + alive[m - 1u] : 0u;
  const uint32_t wanted = n ? offset[n - 1u] + emit[n - 1u] : 0u;
  const uint32_t room = capacity - survivors, emitted = wanted < room ? wanted : room;
  const uint32_t total = survivors + emitted;
  uint32_t k0 = 0, k1 = 0, k2 = 0;
  for (uint32_t q = threadIdx.x; q < total; q += BLOCK) {
    const uint8_t k = kind[q];
    k0 += k == WW_SPRAY, k1 += k == WW_FOAM, k2 += k == WW_BUBBLE;
  }
  uint32_t t0, t1, t2;
  block_excl_scan(k0, &t0);
  block_excl_scan(k1, &t1);
  block_excl_scan(k2, &t2);
  if (threadIdx.x != 0) return;
  host->alive = total, host->emitted = emitted, host->dropped = wanted - emitted, host->died = m - survivors;
  host->kind[0] = t0, host->kind[1] = t1, host->kind[2] = t2;
  __threadfence_system();
  host->seq = seq;
  __threadfence_system();
}

}  // namespace pbf
