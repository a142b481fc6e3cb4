// test_aniso_eig — the eigen-solver pbf_anisotropy_compute's kernels run (csrc/pbf_anisotropy.hpp, aniso_eig3), compiled for
// the host and run in float and double over a fixed-seed set of 10^5 symmetric positive semi-definite matrices: the
// identity, rank 1, rank 2, already diagonal, two equal eigenvalues, entries spanning 2^-60 ... 1, off-diagonals of exactly
// 0, and general ones.  No HIP, not linked against the library.
//
// Prints, per precision and for the sweep count the kernels use (AnisoSweeps<N>), the largest
//     recon = |R diag(sigma) R^T - C|_F / tr C        orth = |R^T R - I|_F        and whether sigma is sorted and >= 0,
// evaluated in long double from the solver's outputs, C being the matrix as rounded to N.  `--scan` prints the same for
// 1 ... 8 sweeps; `--dump FILE` also writes the matrices (6 doubles each: xx yy zz xy xz yz) so that another solver can be
// run on the very same set.  The bars are held by tests/test_anisotropy_cpu.py: four times what numpy.linalg.eigh reaches
// in the same precision on these matrices.  A rounding count of the rotation bounds the rounding alone (about 8 eps_N per
// rotation for either figure, 24 SWEEPS eps_N in all — loose by a factor of 30), not what the sweeps leave off the
// diagonal, so it cannot decide the sweep count; the comparison can.
// Exit status 0 iff sigma is sorted and non-negative and both figures are finite, in both precisions.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pbf_anisotropy.hpp"

namespace {

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t x = (s += 0x9E3779B97F4A7C15ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
  }
  double unit() { return double(next() >> 11) * 0x1p-53; }
};

struct Sym {
  double c[6];  // xx yy zz xy xz yz
};

void rotation(Rng &r, double R[3][3]) {  // a random rotation from a random unit quaternion
  double q[4], n = 0;
  do {
    n = 0;
    for (double &x : q) x = 2 * r.unit() - 1, n += x * x;
  } while (n < 1e-3 || n > 1);
  n = std::sqrt(n);
  const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  R[0][0] = 1 - 2 * (y * y + z * z), R[0][1] = 2 * (x * y - w * z), R[0][2] = 2 * (x * z + w * y);
  R[1][0] = 2 * (x * y + w * z), R[1][1] = 1 - 2 * (x * x + z * z), R[1][2] = 2 * (y * z - w * x);
  R[2][0] = 2 * (x * z - w * y), R[2][1] = 2 * (y * z + w * x), R[2][2] = 1 - 2 * (x * x + y * y);
}

Sym from_spectrum(Rng &r, double l0, double l1, double l2) {
  double R[3][3];
  rotation(r, R);
  const double l[3] = {l0, l1, l2};
  auto e = [&](int a, int b) { return R[a][0] * l[0] * R[b][0] + R[a][1] * l[1] * R[b][1] + R[a][2] * l[2] * R[b][2]; };
  return Sym{{e(0, 0), e(1, 1), e(2, 2), e(0, 1), e(0, 2), e(1, 2)}};
}

std::vector<Sym> matrices() {
  Rng r{20130101ull};
  std::vector<Sym> set;
  set.reserve(100000);
  for (int i = 0; i < 100000; ++i) {
    const double a = 0.01 + r.unit(), b = 0.01 + r.unit(), c = 0.01 + r.unit();
    switch (i % 9) {
      case 0: set.push_back(Sym{{a, a, a, 0, 0, 0}}); break;             // the identity, scaled (i == 0: exactly I)
      case 1: set.push_back(from_spectrum(r, a, 0, 0)); break;           // rank 1
      case 2: set.push_back(from_spectrum(r, a, b, 0)); break;           // rank 2
      case 3: set.push_back(Sym{{a, b, c, 0, 0, 0}}); break;             // already diagonal (any order)
      case 4: set.push_back(from_spectrum(r, a, b, b)); break;           // two equal eigenvalues
      case 5: set.push_back(from_spectrum(r, a, b * 0x1p-30, c * 0x1p-60)); break;  // a spectrum spanning 2^-60 ... 1
      case 6: {                                                          // ENTRIES spanning 2^-60 ... 1, in any positions
        double x[3] = {1.0, std::ldexp(1.0, -int(r.next() % 31)), std::ldexp(1.0, -30)};
        for (int k = 2; k > 0; --k) {
          const int j = int(r.next() % uint64_t(k + 1));
          const double t = x[k];
          x[k] = x[j], x[j] = t;
        }
        const double h = 0.5 * r.unit();  // h x x^T + (1 - h) diag(x^2): PSD
        set.push_back(Sym{{x[0] * x[0], x[1] * x[1], x[2] * x[2], h * x[0] * x[1], h * x[0] * x[2], h * x[1] * x[2]}});
        break;
      }
      case 7: {                                                          // off-diagonals of exactly 0: a 2 x 2 block + 1
        const double t = 6.283185307179586 * r.unit(), cs = std::cos(t), sn = std::sin(t);
        const double p = cs * cs * a + sn * sn * b, q = sn * sn * a + cs * cs * b, o = cs * sn * (a - b);
        const int which = int(r.next() % 3);
        if (which == 0) set.push_back(Sym{{p, q, c, o, 0, 0}});
        else if (which == 1) set.push_back(Sym{{p, c, q, 0, o, 0}});
        else set.push_back(Sym{{c, p, q, 0, 0, o}});
        break;
      }
      default: set.push_back(from_spectrum(r, a, b, c)); break;          // general
    }
  }
  set[0] = Sym{{1, 1, 1, 0, 0, 0}};
  return set;
}

struct Worst {
  long double recon = 0, orth = 0;
  bool sorted = true;
};

template <typename N, int SWEEPS> Worst run(const std::vector<Sym> &set) {
  Worst w;
  for (const Sym &m : set) {
    N c[6], sigma[3], v[3][3];
    for (int k = 0; k < 6; ++k) c[k] = N(m.c[k]);
    pbf::aniso_eig3<N, SWEEPS>(c, sigma, v);
    const long double C[3][3] = {{c[0], c[3], c[4]}, {c[3], c[1], c[5]}, {c[4], c[5], c[2]}};
    long double recon = 0, orth = 0;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        long double e = -C[a][b], o = a == b ? -1.0L : 0.0L;
        for (int k = 0; k < 3; ++k) {
          e += (long double)v[k][a] * (long double)sigma[k] * (long double)v[k][b];
          o += (long double)v[a][k] * (long double)v[b][k];
        }
        recon += e * e, orth += o * o;
      }
    recon = std::sqrt(recon) / (C[0][0] + C[1][1] + C[2][2]), orth = std::sqrt(orth);
    if (!(recon <= w.recon)) w.recon = recon;  // (a NaN sticks)
    if (!(orth <= w.orth)) w.orth = orth;
    w.sorted = w.sorted && sigma[0] >= sigma[1] && sigma[1] >= sigma[2] && sigma[2] >= N(0);
  }
  return w;
}

template <typename N, int SWEEPS> bool report(const std::vector<Sym> &set, const char *name, long double eps) {
  const Worst w = run<N, SWEEPS>(set);
  std::printf("%s sweeps %d recon %.4Le ( %.3Lf eps ) orth %.4Le ( %.3Lf eps ) sorted %d\n", name, SWEEPS, w.recon,
              w.recon / eps, w.orth, w.orth / eps, int(w.sorted));
  return w.sorted && std::isfinite(double(w.recon)) && std::isfinite(double(w.orth));
}

template <typename N, int... S> void scan(const std::vector<Sym> &set, const char *name, long double eps) {
  const bool all[] = {report<N, S>(set, name, eps)...};
  (void)all;
}

}  // namespace

int main(int argc, char **argv) {
  const std::vector<Sym> set = matrices();
  std::printf("matrices %zu\n", set.size());
  if (argc > 2 && std::strcmp(argv[1], "--dump") == 0) {
    std::FILE *f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(set.data(), sizeof(Sym), set.size(), f) != set.size()) return 2;
    std::fclose(f);
  }
  if (argc > 1 && std::strcmp(argv[1], "--scan") == 0) {
    scan<float, 1, 2, 3, 4, 5, 6, 7, 8>(set, "float", FLT_EPSILON);
    scan<double, 1, 2, 3, 4, 5, 6, 7, 8>(set, "double", DBL_EPSILON);
    return 0;
  }
  const bool f = report<float, pbf::AnisoSweeps<float>::value>(set, "float", FLT_EPSILON);
  const bool d = report<double, pbf::AnisoSweeps<double>::value>(set, "double", DBL_EPSILON);
  return f && d ? 0 : 1;
}
