// test_aniso_field — the plain-C++ half of csrc/pbf_aniso_field.hpp (aniso_field_record, aniso_field_term: what k_aniso_pack
// and k_mc_field_aniso run per particle and per candidate), compiled for the host and run in float and double against a long
// double evaluation of the same expressions on the same rounded inputs.  No HIP, not linked against the library.
//
// Inputs, fixed seed: records that are isotropic (radii = k_n, G = I / (h k_n)), k_r-clamped (radii r, r / 4, r / 4 in a random
// frame) and general; with f == 1 and f > 1 (small and large radii, displacements up to 0.9 H); obstacles and non-finite G
// (radii 0), which must come out with rho2 == 0, G'' == 0 and D == 0; and per record nodes spread through the ellipsoid and
// along random directions at q = 1 -+ 1e-2, 1e-4, 1e-6: q2 just below and just above 1.
//
// The bound is the one tests/aniso_surface_ref.py counts (u = the unit round-off of N), without the node coordinate's share
// (the node is an input here):  C_F = 5.5 disp / room + 2,  G'' entries C_G = C_F + 2,  D: C_D = 3 C_F + 6, relative;
//   delta y_a <= (C_G + 4) u yabs_a;   delta q2 <= 2 sum |y_a| delta y_a + 3 u q2;   delta t <= D 3 s^2 delta q2 + (6 + C_D) u t
//   delta k <= 12 D s delta q2 + (C_D + 5) u |k|;   delta z_a <= sum_b |G''_ab| delta y_b + (C_G + 3) u zabs_a
//   delta term_a <= delta k |z_a| + |k| delta z_a + u |term_a|
// A node with |q2 - 1| <= delta q2 may fall on either side; everywhere else hit / no hit must agree, and the pre-test must
// hold with room to spare: rho2 >= 1.4 |d|^2 on every hit.
// Prints the largest error / bound per quantity and precision; exit status 0 iff every ratio is <= 1 and every rule holds.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "pbf_aniso_field.hpp"

namespace {

using L = long double;

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t x = (s += 0x9E3779B97F4A7C15ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
  }
  double unit() { return double(next() >> 11) * 0x1p-53; }
  double sym() { return 2 * unit() - 1; }
};

void rotation(Rng &r, double R[3][3]) {
  double q[4], n = 0;
  do {
    n = 0;
    for (double &x : q) x = r.sym(), n += x * x;
  } while (n < 1e-3 || n > 1);
  n = std::sqrt(n);
  const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  R[0][0] = 1 - 2 * (y * y + z * z), R[0][1] = 2 * (x * y - w * z), R[0][2] = 2 * (x * z + w * y);
  R[1][0] = 2 * (x * y + w * z), R[1][1] = 1 - 2 * (x * x + z * z), R[1][2] = 2 * (y * z - w * x);
  R[2][0] = 2 * (x * z - w * y), R[2][1] = 2 * (y * z + w * x), R[2][2] = 1 - 2 * (x * x + y * y);
}

struct Worst {
  L G = 0, D = 0, t = 0, g = 0;
  bool rules = true;
  size_t records = 0, nodes = 0, hits = 0, band = 0, f1 = 0, fbig = 0, skipped = 0;
};

template <typename N> Worst run() {
  const L u = L(std::numeric_limits<N>::epsilon()) / 2;
  const N h = N(0.1), scale = N(500), H = h * scale;
  Rng r{20130102ull};
  Worst w;
  for (int i = 0; i < 20000; ++i) {
    double R[3][3], st[3];
    rotation(r, R);
    const int kind = i % 5;
    if (kind == 0) {  // isotropic: radii = k_n, R = I
      st[0] = st[1] = st[2] = 0.5;
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) R[a][b] = a == b ? 1.0 : 0.0;
    } else if (kind == 1) {  // k_r-clamped
      st[0] = 0.3 + 1.5 * r.unit(), st[1] = st[2] = st[0] / 4;
    } else if (kind == 2) {  // small: f == 1 unless the displacement is large
      st[0] = 0.2 + 0.3 * r.unit(), st[1] = st[0] * (0.25 + 0.75 * r.unit()), st[2] = st[1] * (0.5 + 0.5 * r.unit());
    } else if (kind == 3) {  // general, f > 1 mostly
      st[0] = 0.8 + r.unit(), st[1] = st[0] * (0.25 + 0.75 * r.unit()), st[2] = st[0] * 0.25;
    } else {  // non-finite: the documented sigma_1 == 0 record
      st[0] = st[1] = st[2] = 0.0;
    }
    const bool obstacle = i % 37 == 0;
    N G[6], radii[3], pos[3], centre[3];
    {
      auto e = [&](int a, int b) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += R[a][k] * R[b][k] / st[k];
        return s / double(h);
      };
      const double g6[6] = {e(0, 0), e(1, 1), e(2, 2), e(0, 1), e(0, 2), e(1, 2)};
      for (int k = 0; k < 6; ++k) G[k] = N(g6[k]);
      for (int k = 0; k < 3; ++k) radii[k] = N(st[k]);
    }
    const double dispWant = (i % 3 == 0 ? 0.0 : 0.9 * r.unit() * r.unit());
    double dir[3] = {r.sym(), r.sym(), r.sym()};
    const double dn = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]) + 1e-300;
    for (int k = 0; k < 3; ++k) {
      pos[k] = N(100.0 + 800.0 * r.unit());
      centre[k] = N(double(pos[k]) + dispWant * double(H) * dir[k] / dn);
    }
    pbf::AnisoFieldRecord<N> rec;
    pbf::aniso_field_record<N>(H, scale, centre, pos, G, radii, !obstacle, rec);
    ++w.records;
    // the same in long double, from the same rounded inputs
    const L e0 = L(centre[0]) - L(pos[0]), e1 = L(centre[1]) - L(pos[1]), e2 = L(centre[2]) - L(pos[2]);
    const L disp = std::sqrt(e0 * e0 + e1 * e1 + e2 * e2) / (L(h) * L(scale));
    const L room = L(pbf::aniso_field_reach<N>()) - disp;
    const L fr = L(radii[0]) / room, f = fr > 1 ? fr : L(1);
    const L Dref = 1 / (f * f * f * L(radii[0]) * L(radii[1]) * L(radii[2]));
    const bool finite = kind != 4;
    if (obstacle || !finite) {
      bool zero = rec.rho2 == N(0) && rec.D == N(0);
      for (int k = 0; k < 6; ++k) zero = zero && rec.G[k] == N(0);
      w.rules = w.rules && zero;
      ++w.skipped;
      N t, gt[3];
      const N a[3] = {centre[0], centre[1], centre[2]};
      w.rules = w.rules && !pbf::aniso_field_term<N>(rec, a, t, gt);  // (contributes nothing, even on its own centre)
      continue;
    }
    (f == 1 ? w.f1 : w.fbig) += 1;
    const L cF = L(5.5) * disp / room + 2, cG = cF + 2, cD = 3 * cF + 6;
    L Gref[6];
    for (int k = 0; k < 6; ++k) {
      Gref[k] = L(G[k]) * f / L(scale);
      const L ratio = std::fabs(L(rec.G[k]) - Gref[k]) / (cG * u * std::fabs(Gref[k]) + 1e-4900L);
      if (!(ratio <= w.G)) w.G = ratio;
    }
    {
      const L ratio = std::fabs(L(rec.D) - Dref) / (cD * u * Dref);
      if (!(ratio <= w.D)) w.D = ratio;
    }
    w.rules = w.rules && rec.rho2 > N(0) && rec.centre[0] == centre[0] && rec.centre[1] == centre[1] && rec.centre[2] == centre[2];
    // nodes: the terms are evaluated from the record AS STORED (what the field kernel sees), against long double on it
    const L g[3][3] = {{rec.G[0], rec.G[3], rec.G[4]}, {rec.G[3], rec.G[1], rec.G[5]}, {rec.G[4], rec.G[5], rec.G[2]}};
    for (int j = 0; j < 12; ++j) {
      // a point at "radius" q of the ellipsoid along a random direction of the unit ball: d = (H / f) R diag(st) v q
      double v[3], vn;
      do {
        v[0] = r.sym(), v[1] = r.sym(), v[2] = r.sym();
        vn = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      } while (vn < 1e-3 || vn > 1);
      const double edge[6] = {1 - 1e-2, 1 + 1e-2, 1 - 1e-4, 1 + 1e-4, 1 - 1e-6, 1 + 1e-6};
      const double q = j < 6 ? edge[j] : 1.3 * r.unit();
      N a[3];
      for (int c = 0; c < 3; ++c) {
        double d = 0;
        for (int k = 0; k < 3; ++k) d += R[c][k] * st[k] * (v[k] / vn);
        a[c] = N(double(centre[c]) + q * d * double(H) / double(f));
      }
      N t = 0, gt[3] = {0, 0, 0};
      const bool hit = pbf::aniso_field_term<N>(rec, a, t, gt);
      ++w.nodes;
      const L d[3] = {L(a[0]) - L(centre[0]), L(a[1]) - L(centre[1]), L(a[2]) - L(centre[2])};
      L y[3], yabs[3], q2 = 0, dy[3], dq2 = 0;
      for (int c = 0; c < 3; ++c) {
        y[c] = g[c][0] * d[0] + g[c][1] * d[1] + g[c][2] * d[2];
        yabs[c] = std::fabs(g[c][0] * d[0]) + std::fabs(g[c][1] * d[1]) + std::fabs(g[c][2] * d[2]);
        q2 += y[c] * y[c];
        dy[c] = 4 * u * yabs[c];  // (the record is exact here: C_G belongs to the comparison above)
        dq2 += 2 * std::fabs(y[c]) * dy[c];
      }
      dq2 += 3 * u * q2;
      if (std::fabs(q2 - 1) <= dq2) {
        ++w.band;
        continue;
      }
      const bool want = q2 < 1;
      w.rules = w.rules && hit == want;
      if (!want || !hit) continue;
      ++w.hits;
      const L d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
      w.rules = w.rules && L(rec.rho2) >= L(1.4) * d2;
      const L s = 1 - q2, Dr = rec.D;
      const L tref = Dr * s * s * s;
      const L dt = Dr * 3 * s * s * dq2 + 6 * u * tref;
      {
        const L ratio = std::fabs(L(t) - tref) / dt;
        if (!(ratio <= w.t)) w.t = ratio;
      }
      const L k = -6 * Dr * s * s, dk = 12 * Dr * s * dq2 + 5 * u * std::fabs(k);
      for (int c = 0; c < 3; ++c) {
        const L z = g[c][0] * y[0] + g[c][1] * y[1] + g[c][2] * y[2];
        const L zabs = std::fabs(g[c][0] * y[0]) + std::fabs(g[c][1] * y[1]) + std::fabs(g[c][2] * y[2]);
        const L dz = std::fabs(g[c][0]) * dy[0] + std::fabs(g[c][1]) * dy[1] + std::fabs(g[c][2]) * dy[2] + 3 * u * zabs;
        const L term = k * z, dterm = dk * std::fabs(z) + std::fabs(k) * dz + u * std::fabs(term);
        const L ratio = std::fabs(L(gt[c]) - term) / dterm;
        if (!(ratio <= w.g)) w.g = ratio;
      }
    }
  }
  return w;
}

template <typename N> bool report(const char *name) {
  const Worst w = run<N>();
  std::printf("%s records %zu ( f==1 %zu f>1 %zu skipped %zu ) nodes %zu hits %zu band %zu ratio G %.4Lf D %.4Lf t %.4Lf g %.4Lf rules %d\n",
              name, w.records, w.f1, w.fbig, w.skipped, w.nodes, w.hits, w.band, w.G, w.D, w.t, w.g, int(w.rules));
  return w.rules && w.G <= 1 && w.D <= 1 && w.t <= 1 && w.g <= 1 && w.f1 > 100 && w.fbig > 100 && w.hits > 1000 && w.skipped > 100;
}

}  // namespace

int main() {
  const bool f = report<float>("float");
  const bool d = report<double>("double");
  return f && d ? 0 : 1;
}
