// pbf_anisotropy.hpp — per-particle anisotropy after Yu & Turk 2013, "Reconstructing surfaces of particle-based fluids
// using anisotropic kernels" (ACM TOG 32(1)), as an observer of the resident state: pbf_anisotropy_compute
// (include/pbf_hip.h states the quantity expression by expression).  No reference counterpart.
//
// Two parts.  The first is plain C++ on scalars — no HIP types — compiled for the device by the kernels and for the host by
// host/test_aniso_eig.cpp: the symmetric 3 x 3 eigen-solver and the step from a particle's eleven sums to its record.  The
// second (under __HIPCC__) is AnisotropyOp, one more gather Op behind begin / near / add / add_bf / end.
//
// Deviation from the paper: the support radius is h, not 2 h — the cells are h wide and the walk sees 27 of them.
//
// Sums of fluid particle i over the FLUID candidates j of its 27 predict-time cells with r = |p_j - p_i| <= h on the final
// pStar, i itself included, d = p_j - p_i, one accumulator set per lane in walk order, everything in N, not contracted, an
// excluded term SELECTED to +0:
//     q = r / h;  w = 1 - q q q;   S += w;   M += w d (3);   Q += (w d_a) d_b (6: xx yy zz xy xz yz);   n += (j != i)
// Then (aniso_finish):
//     mu = M / S;   centre = (p_i + lambda_s mu) scale;   C_ab = (Q_ab / S - mu_a mu_b) / (h h)
//     C = R diag(sigma) R^T by aniso_eig3, sigma_1 >= sigma_2 >= sigma_3 >= 0
//     n > min_neighbours:  st_k = k_s max(sigma_k, sigma_1 / k_r)       otherwise  st_k = k_n and R = I
//     G_ab = (((R_a1 R_b1) (1 / st_1) + (R_a2 R_b2) (1 / st_2)) + (R_a3 R_b3) (1 / st_3)) / h;   axes = the columns of R as
//     rows, the third negated when their determinant is negative;   radii = st.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PBF_HD __host__ __device__
#else
#define PBF_HD
#endif

namespace pbf {

// Sweeps of the cyclic Jacobi iteration, fixed per precision (no data-dependent exit: every lane of a wave runs the same
// instructions).  The smallest counts at which host/test_aniso_eig's figures over its 10^5 matrices stay within four times
// numpy.linalg.eigh's in the same precision (tests/test_anisotropy_cpu.py) — DESIGN 5d has the measurement.
template <typename N> struct AnisoSweeps;
template <> struct AnisoSweeps<float> {
  static constexpr int value = 4;
};
template <> struct AnisoSweeps<double> {
  static constexpr int value = 4;
};

// One Jacobi rotation in the (p, q) plane, Rutishauser's form: theta = (a_qq - a_pp) / (2 a_pq),
// t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c, tau = s / (1 + c); t is SELECTED to 0
// where a_pq == 0 (theta is then infinite or NaN).  arp / arq: the two remaining off-diagonal entries a_rp, a_rq of the
// third index r; vp / vq: columns p and q of the accumulated rotation.
template <typename N> PBF_HD inline void aniso_rotate(N &app, N &aqq, N &apq, N &arp, N &arq, N vp[3], N vq[3]) {
  const N theta = (aqq - app) / (N(2) * apq);
  const N tt = N(1) / (std::fabs(theta) + std::sqrt(theta * theta + N(1)));
  const N t = apq == N(0) ? N(0) : (theta < N(0) ? -tt : tt);
  const N c = N(1) / std::sqrt(t * t + N(1));
  const N s = t * c;
  const N tau = s / (N(1) + c);
  const N h = t * apq;
  app = app - h, aqq = aqq + h, apq = N(0);
  const N g = arp, k = arq;
  arp = g - s * (k + tau * g);
  arq = k + s * (g - tau * k);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int m = 0; m < 3; ++m) {
    const N x = vp[m], y = vq[m];
    vp[m] = x - s * (y + tau * x);
    vq[m] = y + s * (x - tau * y);
  }
}

// c = {xx, yy, zz, xy, xz, yz} of a symmetric matrix.  sigma: the eigenvalues in descending order, negative round-off
// clamped to 0.  v[k][:] = the unit eigenvector of sigma[k].  Cyclic Jacobi, pivots (0,1), (0,2), (1,2), SWEEPS sweeps, then
// a three-exchange compare-select network.
template <typename N, int SWEEPS> PBF_HD inline void aniso_eig3(const N c[6], N sigma[3], N v[3][3]) {
  N a00 = c[0], a11 = c[1], a22 = c[2], a01 = c[3], a02 = c[4], a12 = c[5];
  N v0[3] = {N(1), N(0), N(0)}, v1[3] = {N(0), N(1), N(0)}, v2[3] = {N(0), N(0), N(1)};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int sweep = 0; sweep < SWEEPS; ++sweep) {
    aniso_rotate<N>(a00, a11, a01, a02, a12, v0, v1);  // (0,1): r = 2
    aniso_rotate<N>(a00, a22, a02, a01, a12, v0, v2);  // (0,2): r = 1
    aniso_rotate<N>(a11, a22, a12, a01, a02, v1, v2);  // (1,2): r = 0
  }
  auto exchange = [](N &sa, N &sb, N va[3], N vb[3]) {  // afterwards sa >= sb
    const bool swap = sb > sa;
    const N s0 = sa, s1 = sb;
    sa = swap ? s1 : s0, sb = swap ? s0 : s1;
    for (int m = 0; m < 3; ++m) {
      const N x = va[m], y = vb[m];
      va[m] = swap ? y : x, vb[m] = swap ? x : y;
    }
  };
  exchange(a00, a11, v0, v1);
  exchange(a11, a22, v1, v2);
  exchange(a00, a11, v0, v1);
  sigma[0] = a00 > N(0) ? a00 : N(0), sigma[1] = a11 > N(0) ? a11 : N(0), sigma[2] = a22 > N(0) ? a22 : N(0);
  for (int m = 0; m < 3; ++m) v[0][m] = v0[m], v[1][m] = v1[m], v[2][m] = v2[m];
}

// the configuration in N, by value to the kernel (pbf_anisotropy, include/pbf_hip.h)
template <typename N> struct AnisoConsts {
  N smoothing, kR, kS, kN;
  uint32_t minNeighbours;
};

template <typename N> struct AnisoRecord {
  N centre[3];  // world
  N G[6];       // xx yy zz xy xz yz, solver frame
  N axes[9];    // three unit rows, descending, right-handed
  N radii[3];
};

// From the eleven sums of one fluid particle to its record.  p = its pStar (solver frame).
template <typename N, int SWEEPS>
PBF_HD inline void aniso_finish(const AnisoConsts<N> &k, N h, N scale, const N p[3], N S, const N M[3], const N Q[6],
                                uint32_t n, AnisoRecord<N> &out) {
  const N mu[3] = {M[0] / S, M[1] / S, M[2] / S};
  for (int a = 0; a < 3; ++a) out.centre[a] = (p[a] + k.smoothing * mu[a]) * scale;
  const N hh = h * h;
  const N c[6] = {(Q[0] / S - mu[0] * mu[0]) / hh, (Q[1] / S - mu[1] * mu[1]) / hh, (Q[2] / S - mu[2] * mu[2]) / hh,
                  (Q[3] / S - mu[0] * mu[1]) / hh, (Q[4] / S - mu[0] * mu[2]) / hh, (Q[5] / S - mu[1] * mu[2]) / hh};
  N sigma[3], v[3][3];
  aniso_eig3<N, SWEEPS>(c, sigma, v);
  const bool enough = n > k.minNeighbours;
  const N floor1 = sigma[0] / k.kR;
  N st[3];
  for (int m = 0; m < 3; ++m) st[m] = enough ? k.kS * (sigma[m] > floor1 ? sigma[m] : floor1) : k.kN;
  for (int m = 0; m < 3; ++m)
    for (int a = 0; a < 3; ++a) v[m][a] = enough ? v[m][a] : (m == a ? N(1) : N(0));
  const N det = v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) - v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0]) +
                v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
  for (int a = 0; a < 3; ++a) v[2][a] = det < N(0) ? -v[2][a] : v[2][a];
  const N g[3] = {N(1) / st[0], N(1) / st[1], N(1) / st[2]};
  auto entry = [&](int a, int b) {
    return (((v[0][a] * v[0][b]) * g[0] + (v[1][a] * v[1][b]) * g[1]) + (v[2][a] * v[2][b]) * g[2]) / h;
  };
  out.G[0] = entry(0, 0), out.G[1] = entry(1, 1), out.G[2] = entry(2, 2);
  out.G[3] = entry(0, 1), out.G[4] = entry(0, 2), out.G[5] = entry(1, 2);
  for (int m = 0; m < 3; ++m) {
    out.radii[m] = st[m];
    for (int a = 0; a < 3; ++a) out.axes[3 * m + a] = v[m][a];
  }
}

}  // namespace pbf

#if defined(__HIPCC__)
#include "pbf_kernels.hpp"

namespace pbf {

// The candidate: position, its index (which tells a particle meeting itself from a coincident neighbour, as in DensityOp)
// and whether it is fluid — the type is read in load() and an obstacle is selected away, which adds the same +0 to every
// sum that skipping it does (DiffuseOp's kNeedsCandidateType only reaches the unfiltered walk).
template <typename N> struct AnisoSrc {
  vec4<N> p;
  uint32_t idx, fluid;
};
template <typename N> __device__ inline void pin_registers(AnisoSrc<N> &b) {  // (the list readers' pipelining)
  pin_registers(b.p);
  asm volatile("" : "+v"(b.idx), "+v"(b.fluid));
}

// Outputs are component-major planes of n elements each (value k of particle i at [k n + i]): consecutive lanes store
// consecutive elements, and each array travels to the caller in one plain copy.
template <typename N, bool FAST> struct AnisotropyOp {
  using Src = AnisoSrc<N>;
  struct Args {
    const vec4<N> *pstar, *pos4;
    const uint8_t *type;
    N *centre, *G, *axes, *radii;  // N[3n], N[6n], N[9n], N[3n]
    uint32_t *neighbours;          // uint32[n]
    AnisoConsts<N> k;
  };
  static constexpr bool kNeedsCandidateType = false;  // (the type is read in load(): obstacles are selected away)
  static constexpr bool kFilter = true;
  static constexpr bool kTileable = false;
  __device__ static Src load(const Args &a, uint32_t b) { return Src{a.pstar[b], b, uint32_t((a.type[b] & 1) ^ 1u)}; }
  vec4<N> pa;
  N S, mx, my, mz, qxx, qyy, qzz, qxy, qxz, qyz;
  uint32_t self, nbr;
  __device__ bool near(const StepConsts<N> &c, const Src &b) const { return maybe_within_h<N>(pa, b.p, c.h2filter); }
  __device__ bool begin(const StepConsts<N> &c, const Args &a, uint32_t i) {
    if (c.hasObstacles && a.type[i] != 0) {  // centre = the stored position, every other field 0
      const vec4<N> x = a.pos4[i];
      const size_t n = c.n;
      a.centre[i] = x.x, a.centre[n + i] = x.y, a.centre[2 * n + i] = x.z;
      for (int k = 0; k < 6; ++k) a.G[k * n + i] = N(0);
      for (int k = 0; k < 9; ++k) a.axes[k * n + i] = N(0);
      for (int k = 0; k < 3; ++k) a.radii[k * n + i] = N(0);
      a.neighbours[i] = 0u;
      return false;
    }
    pa = a.pstar[i];
    S = mx = my = mz = qxx = qyy = qzz = qxy = qxz = qyz = N(0);
    self = i, nbr = 0u;
    return true;
  }
  __device__ void add(const StepConsts<N> &c, const Src &b) { add_bf(c, b); }
  // every term of an excluded candidate is selected to +0: the sums are the same bits on every gather kernel
  __device__ void add_bf(const StepConsts<N> &c, const Src &b, bool valid = true) {
    const auto g = pair_geom<N, FAST>(pa, b.p, c.h);
    const bool in = g.inH && valid && b.fluid != 0u;
    const N dx = -g.dx, dy = -g.dy, dz = -g.dz;  // p_j - p_i
    const N q = g.r / c.h;
    const N w = N(1) - q * q * q;
    const N wx = w * dx, wy = w * dy, wz = w * dz;
    S += in ? w : N(0);
    mx += in ? wx : N(0), my += in ? wy : N(0), mz += in ? wz : N(0);
    qxx += in ? wx * dx : N(0), qyy += in ? wy * dy : N(0), qzz += in ? wz * dz : N(0);
    qxy += in ? wx * dy : N(0), qxz += in ? wx * dz : N(0), qyz += in ? wy * dz : N(0);
    nbr += (in && b.idx != self) ? 1u : 0u;
  }
  __device__ void end(const StepConsts<N> &c, const Args &a, uint32_t i) {
    const N p[3] = {pa.x, pa.y, pa.z}, M[3] = {mx, my, mz}, Q[6] = {qxx, qyy, qzz, qxy, qxz, qyz};
    AnisoRecord<N> r;
    aniso_finish<N, AnisoSweeps<N>::value>(a.k, c.h, c.scale, p, S, M, Q, nbr, r);
    const size_t n = c.n;
#pragma unroll
    for (int k = 0; k < 3; ++k) a.centre[k * n + i] = r.centre[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) a.G[k * n + i] = r.G[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) a.axes[k * n + i] = r.axes[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) a.radii[k * n + i] = r.radii[k];
    a.neighbours[i] = nbr;
  }
};

}  // namespace pbf
#endif
