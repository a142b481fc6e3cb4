// pbf_aniso_field.hpp — the scalar field of Yu & Turk 2013 on the marching-cubes lattice: phi(a) = sum_j W(a - centre_j, G_j)
// over the records pbf_anisotropy_compute makes (pbf_surface_anisotropic; include/pbf_hip.h states the same text).  No
// reference counterpart: the stock field k_mc_field (pbf_mc.hpp) is the reference's and stays as it is.
//
// Two parts, like pbf_anisotropy.hpp.  The first is plain C++ on scalars — no HIP types — compiled for the device by the
// kernels and for the host by host/test_aniso_field.cpp: a particle's record and one candidate's term.  The second (under
// __HIPCC__) holds k_aniso_pack, k_mc_field_aniso and k_mc_fill_far.
//
// CONTRACT.  The field is a function of exactly these bytes: the arrays pbf_anisotropy_compute returns for the same state and
// `kernel` (centre, G, radii), pos4, col4, the types and the predict-time table.  Everything in N, evaluated in the order
// written, not contracted.
//
// RECORD of fluid particle j (aniso_field_record; k_aniso_pack, one lane per particle), H = h * scale:
//     e     = centre_j - pos_j                                            (world)
//     disp  = sqrt((e_x e_x + e_y e_y) + e_z e_z) / H
//     f     = max(1, radii_1 / (0.99 - disp))
//     G''_ab = G_ab * (f / scale)        the world frame, shrunk uniformly by f: the ellipsoid |G''(a - centre_j)| < 1 has
//             the largest semi-axis H radii_1 / f, so it reaches at most disp + radii_1 / f <= 0.99 (in units of H) from
//             pos_j: it lies inside the ball of radius H around its particle, the region the 27-cell walk of a node sees.
//             SECOND DEVIATION from the paper (the first: a support of h, not 2 h).  f = 1 wherever radii_1 + disp <= 0.99.
//             (max(1, radii_1 + disp) would not do: shrinking about the centre leaves the displacement as it is, and the
//             reach disp + radii_1 / (radii_1 + disp) exceeds 1 whenever disp > 0 and radii_1 + disp > 1.)
//     D     = 1 / (((f f) f) ((radii_1 radii_2) radii_3))                 det(h f G): Yu & Turk's ||G|| normalisation
//     rho2  = (((H radii_1) / f) ((H radii_1) / f)) * 1.5                 a conservative pre-test, see below
//   The constraint holds the fluid density at rho_0, so the paper's m_j / rho_j is one constant for all particles: it is
//   absorbed into the isolevel.
//   An obstacle, a particle whose D or G'' is not finite (sigma_1 == 0, include/pbf_hip.h) or one with disp >= 0.99 (its
//   centre would have to lie a whole h from it: mu is a mean of displacements below h that includes the particle's own 0)
//   gets rho2 = 0, G'' = 0, D = 0 and contributes nothing; the field kernel loads no type.
//   Three vec4<N> per particle: {centre.xyz, rho2} {G''xx, G''yy, G''zz, D} {G''xy, G''xz, G''yz, 0}.
//
// NODE a (k_mc_field_aniso; the coordinates and the node's cell z exactly as k_mc_field computes them).  Candidates: the
// particles of the cells z - 1, z, z + 1 per axis; a slot outside [0, extent - 1] is SKIPPED, not clamped, so every cell is
// visited once (the node whose cell is the extent on every axis needs no special case).  Slots in ascending slot order
// (x fastest), candidates in table order.  Per candidate (aniso_field_term):
//     d   = a - centre
//     pre-test: (d_x d_x + d_y d_y) + d_z d_z < rho2, else no hit.  |G'' d| < 1 implies |d| < H radii_1 / f, and the factor
//               1.5 (22 % on the radius) is far above the rounding of G'' and of the test itself: it never decides a hit.
//     y_a = (G''_ax d_x + G''_ay d_y) + G''_az d_z
//     q2  = (y_x y_x + y_y y_y) + y_z y_z;                                 a hit iff q2 < 1
//   per hit:
//     s = 1 - q2;   t = D ((s s) s);   phi += t
//     z_a = (G''_ax y_x + G''_ay y_y) + G''_az y_z;   g_a += ((-6 D) (s s)) z_a           (grad phi: points INTO the fluid)
//     C += t colour_j                                                      (the colour is loaded on a hit only)
//   stored, with len = sqrt((g_x g_x + g_y g_y) + g_z g_z):
//     phi > 0:  latticePN = {phi, n}, n_a = len > 0 ? (-g_a) / len : 0 (outwards, the stock convention: mc_case's
//               `v < isolevel` means outside in both fields);  latticeC = C / phi
//     otherwise (no hit, or hits whose terms all underflow): phi = 0, normal 0, colour 0.  Never NaN.
//
// k_mc_fill_far (one lane per node).  The support is compact, so the outer end of a crossed edge often has no hit at all,
// and the vertex colours k_mc_emit interpolates would be mixed with zero.  A node with phi == 0 that has a 6-neighbour with
// phi > 0 takes as colour the sum of those neighbours' colours in the order -x +x -y +y -z +z, divided by their number.  Its
// normal stays zero (a unit normal mixed with zero keeps its direction).  Writers have phi == 0, sources phi > 0: in place,
// no race.  Every far end of a crossed edge has such a neighbour since isolevel > 0.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PBF_HD __host__ __device__
#else
#define PBF_HD
#endif

namespace pbf {

template <typename N> struct AnisoFieldRecord {
  N centre[3], rho2;
  N G[6];  // G'': xx yy zz xy xz yz, world frame
  N D;
};

// how far from its particle an ellipsoid may reach, in units of H
template <typename N> PBF_HD constexpr N aniso_field_reach() { return N(0.99); }
// the pre-test's slack on the squared radius
template <typename N> PBF_HD constexpr N aniso_field_slack() { return N(1.5); }

template <typename N>
PBF_HD inline void aniso_field_record(N H, N scale, const N centre[3], const N pos[3], const N G[6], const N radii[3],
                                      bool fluid, AnisoFieldRecord<N> &r) {
  const N ex = centre[0] - pos[0], ey = centre[1] - pos[1], ez = centre[2] - pos[2];
  const N disp = std::sqrt((ex * ex + ey * ey) + ez * ez) / H;
  const N room = aniso_field_reach<N>() - disp;
  const N fr = radii[0] / room;
  const N f = fr > N(1) ? fr : N(1);
  const N fs = f / scale;
  bool ok = fluid && room > N(0);
  for (int k = 0; k < 6; ++k) {
    r.G[k] = G[k] * fs;
    ok = ok && std::isfinite(r.G[k]);
  }
  r.D = N(1) / (((f * f) * f) * ((radii[0] * radii[1]) * radii[2]));
  ok = ok && std::isfinite(r.D);
  const N rad = (H * radii[0]) / f;
  r.rho2 = ok ? (rad * rad) * aniso_field_slack<N>() : N(0);
  for (int k = 0; k < 3; ++k) r.centre[k] = centre[k];
  if (!ok) {
    for (int k = 0; k < 6; ++k) r.G[k] = N(0);
    r.D = N(0);
  }
}

// One candidate at node a: a hit iff the return value; then t and the three components of its gradient term.
template <typename N> PBF_HD inline bool aniso_field_term(const AnisoFieldRecord<N> &r, const N a[3], N &t, N gt[3]) {
  const N dx = a[0] - r.centre[0], dy = a[1] - r.centre[1], dz = a[2] - r.centre[2];
  if (!((dx * dx + dy * dy) + dz * dz < r.rho2)) return false;
  const N yx = (r.G[0] * dx + r.G[3] * dy) + r.G[4] * dz;
  const N yy = (r.G[3] * dx + r.G[1] * dy) + r.G[5] * dz;
  const N yz = (r.G[4] * dx + r.G[5] * dy) + r.G[2] * dz;
  const N q2 = (yx * yx + yy * yy) + yz * yz;
  if (!(q2 < N(1))) return false;
  const N s = N(1) - q2;
  const N ss = s * s;
  t = r.D * (ss * s);
  const N k = (N(-6) * r.D) * ss;
  gt[0] = k * ((r.G[0] * yx + r.G[3] * yy) + r.G[4] * yz);
  gt[1] = k * ((r.G[3] * yx + r.G[1] * yy) + r.G[5] * yz);
  gt[2] = k * ((r.G[4] * yx + r.G[5] * yy) + r.G[2] * yz);
  return true;
}

}  // namespace pbf

#if defined(__HIPCC__)
#include "pbf_mc.hpp"

namespace pbf {

// centre / G / radii: pbf_anisotropy_compute's component-major planes of n elements (AnisotropyOp's outputs, still on the
// device); rec: three vec4 per particle
template <typename N>
__global__ __launch_bounds__(BLOCK) void k_aniso_pack(uint32_t n, N H, N scale, uint32_t hasObstacles,
                                                      const vec4<N> *__restrict__ pos4, const uint8_t *__restrict__ type,
                                                      const N *__restrict__ centre, const N *__restrict__ G,
                                                      const N *__restrict__ radii, vec4<N> *__restrict__ rec) {
  const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
  if (j >= n) return;
  const size_t np = n;
  const vec4<N> p = pos4[j];
  const N pos[3] = {p.x, p.y, p.z};
  N c[3], g[6], rd[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = centre[k * np + j], rd[k] = radii[k * np + j];
#pragma unroll
  for (int k = 0; k < 6; ++k) g[k] = G[k * np + j];
  const bool fluid = !(hasObstacles && (type[j] & TYPE_OBSTACLE));
  AnisoFieldRecord<N> r;
  aniso_field_record<N>(H, scale, c, pos, g, rd, fluid, r);
  rec[3 * size_t(j) + 0] = make_vec4<N>(r.centre[0], r.centre[1], r.centre[2], r.rho2);
  rec[3 * size_t(j) + 1] = make_vec4<N>(r.G[0], r.G[1], r.G[2], r.D);
  rec[3 * size_t(j) + 2] = make_vec4<N>(r.G[3], r.G[4], r.G[5], N(0));
}

// k_mc_field's lane -> node map (2 x 2 x 2 blocks of nodes per 8 lanes, 4 x 4 x 4 per wave), its node coordinates and cell,
// and its candidates-in-flight loop: two candidates' three vectors (24 registers in fp32) are loaded before either is folded
template <typename N>
__global__ __launch_bounds__(BLOCK) void k_mc_field_aniso(McConsts<N> m, const uint32_t *__restrict__ table,
                                                          const vec4<N> *__restrict__ rec, const vec4<N> *__restrict__ col4,
                                                          const uint32_t *__restrict__ nearMask,
                                                          vec4<N> *__restrict__ latticePN, vec4<N> *__restrict__ latticeC) {
  const uint32_t sx = m.planes, sy = m.sample[1], sz = m.sample[2];
  const uint32_t bx = (sx + 3u) / 4u, by = (sy + 3u) / 4u, bz = (sz + 3u) / 4u;
  const uint32_t t = blockIdx.x * BLOCK + threadIdx.x, blk = t >> 6, l = t & 63u;
  if (blk >= bx * by * bz) return;
  const uint32_t x = (blk / (by * bz)) * 4u + ((l >> 5) & 1u) * 2u + ((l >> 2) & 1u),
                 y = ((blk / bz) % by) * 4u + ((l >> 4) & 1u) * 2u + ((l >> 1) & 1u),
                 z = (blk % bz) * 4u + ((l >> 3) & 1u) * 2u + (l & 1u);
  if (x >= sx || y >= sy || z >= sz) return;
  const uint32_t idx = (x * sy + y) * sz + z;
  const N px = N(x + m.nodeX0), py = N(y), pz = N(z);
  const N a[3] = {(m.minExtent[0] + (px * m.step)) * m.scale, (m.minExtent[1] + (py * m.step)) * m.scale,
                  (m.minExtent[2] + (pz * m.step)) * m.scale};
  const uint32_t zX = uint32_t(uint64_t(px / m.res)) & 1023u, zY = uint32_t(uint64_t(py / m.res)) & 1023u,
                 zZ = uint32_t(uint64_t(pz / m.res)) & 1023u;
  // the slots inside the grid: per axis bit d + 1 for the offsets d = -1, 0, +1 with 0 <= z + d <= extent - 1
  auto valid = [](uint32_t zc, uint32_t ext) {
    return (zc >= 1u && zc <= ext ? 1u : 0u) | (zc < ext ? 2u : 0u) | (zc + 1u < ext ? 4u : 0u);
  };
  const uint32_t vx = valid(zX, m.extent[0]), vy = valid(zY, m.extent[1]), vz = valid(zZ, m.extent[2]);
  uint32_t slots = 0;
#pragma unroll
  for (uint32_t k = 0; k < 27; ++k)
    if ((vx >> (k % 3u) & 1u) && (vy >> ((k / 3u) % 3u) & 1u) && (vz >> (k / 9u) & 1u)) slots |= 1u << k;
  // k_mc_mark_near's mask names the non-empty cells; its fold bits belong to slots skipped above
  const bool inside = zX < m.extent[0] && zY < m.extent[1] && zZ < m.extent[2];
  if (inside) slots &= nearMask[morton_encode(zX - m.xoff, zY, zZ)];
  N phi = 0, gx = 0, gy = 0, gz = 0, cr = 0, cg = 0, cb = 0, ca = 0;
  auto fold = [&](const vec4<N> &r0, const vec4<N> &r1, const vec4<N> &r2, uint32_t b) {
    const AnisoFieldRecord<N> r{{r0.x, r0.y, r0.z}, r0.w, {r1.x, r1.y, r1.z, r2.x, r2.y, r2.z}, r1.w};
    N tt, gt[3];
    if (!aniso_field_term<N>(r, a, tt, gt)) return;
    phi += tt;
    gx += gt[0], gy += gt[1], gz += gt[2];
    const vec4<N> c = col4[b];
    cr += tt * c.x, cg += tt * c.y, cb += tt * c.z, ca += tt * c.w;
  };
  while (slots) {
    const int k = __builtin_ctz(slots);
    slots &= slots - 1u;
    const uint32_t off = morton_encode(zX + uint32_t(k % 3) - 1u - m.xoff, zY + uint32_t((k / 3) % 3) - 1u, zZ + uint32_t(k / 9) - 1u);
    if (off >= m.tableN) continue;
    const uint32_t s0 = table[off], e0 = (off + 1u) < m.tableN ? table[off + 1u] : s0;
    for (uint32_t b = s0; b < e0; b += 2u) {
      vec4<N> r[2][3];
#pragma unroll
      for (uint32_t w = 0; w < 2; ++w) {
        const size_t bw = min(b + w, e0 - 1u);  // a tail slot re-reads the last candidate and is masked
#pragma unroll
        for (uint32_t v = 0; v < 3; ++v) r[w][v] = rec[3 * bw + v];
      }
#pragma unroll
      for (uint32_t w = 0; w < 2; ++w)
        if (b + w < e0) fold(r[w][0], r[w][1], r[w][2], b + w);
    }
  }
  const vec4<N> zero = make_vec4<N>(N(0), N(0), N(0), N(0));
  if (!(phi > N(0))) {
    latticePN[idx] = zero, latticeC[idx] = zero;
    return;
  }
  const N len = sqrt((gx * gx + gy * gy) + gz * gz);
  const bool has = len > N(0);
  latticePN[idx] = make_vec4<N>(phi, has ? (-gx) / len : N(0), has ? (-gy) / len : N(0), has ? (-gz) / len : N(0));
  latticeC[idx] = make_vec4<N>(cr / phi, cg / phi, cb / phi, ca / phi);
}

// one lane per node of the sample[0] x sample[1] x sample[2] lattice, z fastest
template <typename N>
__global__ __launch_bounds__(BLOCK) void k_mc_fill_far(uint32_t sx, uint32_t sy, uint32_t sz,
                                                       const vec4<N> *__restrict__ latticePN, vec4<N> *latticeC) {
  const uint32_t idx = blockIdx.x * BLOCK + threadIdx.x;
  const uint32_t plane = sy * sz;
  if (idx >= sx * plane) return;
  if (latticePN[idx].x != N(0)) return;
  const uint32_t x = idx / plane, y = (idx / sz) % sy, z = idx % sz;
  const bool in[6] = {x > 0u, x + 1u < sx, y > 0u, y + 1u < sy, z > 0u, z + 1u < sz};
  const uint32_t at[6] = {idx - plane, idx + plane, idx - sz, idx + sz, idx - 1u, idx + 1u};
  N c[4] = {N(0), N(0), N(0), N(0)};
  uint32_t k = 0;
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    if (!in[s]) continue;
    if (!(latticePN[at[s]].x > N(0))) continue;
    const vec4<N> v = latticeC[at[s]];
    c[0] += v.x, c[1] += v.y, c[2] += v.z, c[3] += v.w;
    ++k;
  }
  if (k == 0u) return;
  const N nk = N(k);
  latticeC[idx] = make_vec4<N>(c[0] / nk, c[1] / nk, c[2] / nk, c[3] / nk);
}

}  // namespace pbf
#endif
