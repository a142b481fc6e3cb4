// mesh_sdf_rate — times the mesh collider's fold (csrc/pbf_mesh_sdf.hpp, launch_fold: the launches pbf_sdf_from_mesh makes) on
// the workload of profiles/mesh_sdf.md: the 201^3 lattice over the stock 1000-unit box at spacing 5 (origin -0, dims 201) from
// an icosphere with five subdivisions (20 480 triangles, R 250, centre (520, 500, 600)), in float and double, cull off and on.
// HIP events bracket the kernel launches only; two warm-up runs, then the median of five.  Also checks that the culled lattice
// equals the all-pairs one byte for byte.  Then the same mesh as a triangle soup signed by the winding number
// (csrc/pbf_mesh_winding.hpp): the distance-only fold, cull off and on, and the winding fold (launch_winding: every pair, split
// over launches of at most 2^[log2 winding pairs per launch] pairs), with the time of one launch and the pairs per second
// against the distance fold's all-pairs rate.  Prints one JSON line per case.  (GPU box)
//   hipcc -std=c++17 -O3 -ffp-contract=off -fno-slp-vectorize --offload-arch=gfx950 -I include -I pbf-sph_amd/csrc
//         tools/mesh_sdf_rate.hip -o tools/mesh_sdf_rate
//   tools/mesh_sdf_rate [subdivisions = 5] [nodes per axis = 201] [log2 winding pairs per launch = the library's]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "pbf_mesh_winding.hpp"

#define CHECK(e)                                                                                  \
  do {                                                                                            \
    const hipError_t r_ = (e);                                                                    \
    if (r_ != hipSuccess) {                                                                       \
      std::fprintf(stderr, "%s: %s (line %d)\n", #e, hipGetErrorString(r_), __LINE__);            \
      return 1;                                                                                   \
    }                                                                                             \
  } while (0)

namespace {

void icosphere(int subdivisions, double R, const double c[3], std::vector<double> &v, std::vector<uint32_t> &t) {
  const double g = (1 + std::sqrt(5.0)) / 2;
  const double base[12][3] = {{-1, g, 0}, {1, g, 0}, {-1, -g, 0}, {1, -g, 0}, {0, -1, g}, {0, 1, g},
                              {0, -1, -g}, {0, 1, -g}, {g, 0, -1}, {g, 0, 1}, {-g, 0, -1}, {-g, 0, 1}};
  const uint32_t faces[20][3] = {{0, 11, 5}, {0, 5, 1}, {0, 1, 7}, {0, 7, 10}, {0, 10, 11}, {1, 5, 9}, {5, 11, 4}, {11, 10, 2}, {10, 7, 6}, {7, 1, 8},
                                 {3, 9, 4}, {3, 4, 2}, {3, 2, 6}, {3, 6, 8}, {3, 8, 9}, {4, 9, 5}, {2, 4, 11}, {6, 2, 10}, {8, 6, 7}, {9, 8, 1}};
  std::vector<double> u;  // unit vectors
  auto push = [&](double x, double y, double z) {
    const double l = std::sqrt(x * x + y * y + z * z);
    u.insert(u.end(), {x / l, y / l, z / l});
    return uint32_t(u.size() / 3 - 1);
  };
  for (const auto &b : base) push(b[0], b[1], b[2]);
  t.clear();
  for (const auto &f : faces) t.insert(t.end(), f, f + 3);
  for (int s = 0; s < subdivisions; ++s) {
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> mid;
    auto m = [&](uint32_t a, uint32_t b) {
      const auto key = std::make_pair(std::min(a, b), std::max(a, b));
      const auto it = mid.find(key);
      if (it != mid.end()) return it->second;
      const uint32_t i = push(u[3 * a] + u[3 * b], u[3 * a + 1] + u[3 * b + 1], u[3 * a + 2] + u[3 * b + 2]);
      mid[key] = i;
      return i;
    };
    std::vector<uint32_t> out;
    for (size_t k = 0; k < t.size(); k += 3) {
      const uint32_t a = t[k], b = t[k + 1], c2 = t[k + 2], ab = m(a, b), bc = m(b, c2), ca = m(c2, a);
      out.insert(out.end(), {a, ab, ca, b, bc, ab, c2, ca, bc, ab, bc, ca});
    }
    t.swap(out);
  }
  v.resize(u.size());
  for (size_t k = 0; k < u.size(); ++k) v[k] = u[k] * R + c[k % 3];
}

template <typename N>
int run(const char *tag, const std::vector<double> &v, const std::vector<uint32_t> &t, uint32_t side, double spacing, uint64_t windingPairs) {
  const pbf_mesh mesh{v.size() / 3, t.size() / 3, v.data(), t.data()};
  const size_t nt = t.size() / 3;
  std::vector<N> rec(size_t(meshsdf::RECORD) * nt), bnd(4 * nt);
  const char *why = nullptr;
  if (meshsdf::build_records(&mesh, sizeof(N) == 8, rec.data(), nullptr, &why) != PBF_OK) {
    std::fprintf(stderr, "%s\n", why);
    return 1;
  }
  const uint32_t dims[3] = {side, side, side};
  const double origin[3] = {0, 0, 0};
  meshsdf::SdfLattice<N> L;
  N slack;
  meshsdf::prepare<N>(dims, origin, spacing, rec.data(), nt, meshsdf::RECORD, &L, bnd.data(), &slack);
  const size_t nodes = size_t(side) * side * side, bricks = meshsdf::brick_count(L);
  N *dRec, *dBnd, *dOut;
  uint8_t *dSign;
  unsigned long long *dTested;
  CHECK(hipMalloc(&dRec, rec.size() * sizeof(N)));
  CHECK(hipMalloc(&dBnd, bnd.size() * sizeof(N)));
  CHECK(hipMalloc(&dOut, nodes * sizeof(N)));
  CHECK(hipMalloc(&dSign, nodes));
  CHECK(hipMalloc(&dTested, bricks * sizeof(unsigned long long)));
  CHECK(hipMemcpy(dRec, rec.data(), rec.size() * sizeof(N), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dBnd, bnd.data(), bnd.size() * sizeof(N), hipMemcpyHostToDevice));
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a));
  CHECK(hipEventCreate(&b));
  std::vector<N> plain(nodes), culled(nodes);
  std::vector<unsigned long long> slots(bricks);
  for (int cull = 0; cull < 2; ++cull) {
    std::vector<float> ms;
    for (int rep = 0; rep < 7; ++rep) {
      CHECK(hipEventRecord(a, nullptr));
      CHECK(meshsdf::launch_fold<N>(nullptr, L, dRec, dBnd, nt, cull != 0, false, slack, dOut, dSign, dTested));
      CHECK(hipEventRecord(b, nullptr));
      CHECK(hipEventSynchronize(b));
      float x = 0;
      CHECK(hipEventElapsedTime(&x, a, b));
      if (rep >= 2) ms.push_back(x);
    }
    std::sort(ms.begin(), ms.end());
    CHECK(hipMemcpy((cull ? culled : plain).data(), dOut, nodes * sizeof(N), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(slots.data(), dTested, bricks * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long tested = 0;
    for (unsigned long long s : slots) tested += s;
    const double total = double(nodes) * double(nt);
    const bool same = !cull || std::memcmp(plain.data(), culled.data(), nodes * sizeof(N)) == 0;
    std::printf("{\"type\": \"%s\", \"sdf_cull\": %d, \"nodes\": %zu, \"triangles\": %zu, \"ms_median\": %.3f, \"ms_min\": %.3f, \"ms_max\": %.3f, "
                "\"pairs_total\": %.0f, \"pairs_tested\": %llu, \"tested_pairs_per_s\": %.4g, \"total_pairs_per_s\": %.4g, \"same_bytes_as_all_pairs\": %s}\n",
                tag, cull, nodes, nt, ms[2], ms.front(), ms.back(), total, tested, double(tested) / (ms[2] * 1e-3), total / (ms[2] * 1e-3),
                same ? "true" : "false");
    std::fflush(stdout);
    if (!same) return 1;
  }
  double allPairsRate = 0;
  {  // the soup: the distance-only fold, then the winding fold
    std::vector<N> soup(size_t(meshsdf::SOUP_RECORD) * nt);
    if (meshsdf::build_soup_records(&mesh, sizeof(N) == 8, soup.data(), nullptr, &why) != PBF_OK) {
      std::fprintf(stderr, "%s\n", why);
      return 1;
    }
    meshsdf::prepare<N>(dims, origin, spacing, soup.data(), nt, meshsdf::SOUP_RECORD, &L, bnd.data(), &slack);
    N *dSum;
    CHECK(hipMalloc(&dSum, nodes * sizeof(N)));
    CHECK(hipMemcpy(dRec, soup.data(), soup.size() * sizeof(N), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dBnd, bnd.data(), bnd.size() * sizeof(N), hipMemcpyHostToDevice));
    const double total = double(nodes) * double(nt);
    for (int cull = 0; cull < 2; ++cull) {
      std::vector<float> ms;
      for (int rep = 0; rep < 7; ++rep) {
        CHECK(hipEventRecord(a, nullptr));
        CHECK(meshsdf::launch_fold<N>(nullptr, L, dRec, dBnd, nt, cull != 0, false, slack, dOut, dSign, dTested, 0, true));
        CHECK(hipEventRecord(b, nullptr));
        CHECK(hipEventSynchronize(b));
        float x = 0;
        CHECK(hipEventElapsedTime(&x, a, b));
        if (rep >= 2) ms.push_back(x);
      }
      std::sort(ms.begin(), ms.end());
      if (!cull) allPairsRate = total / (ms[2] * 1e-3);
      std::printf("{\"type\": \"%s\", \"fold\": \"soup distance\", \"sdf_cull\": %d, \"ms_median\": %.3f, \"ms_min\": %.3f, \"ms_max\": %.3f, "
                  "\"total_pairs_per_s\": %.4g}\n", tag, cull, ms[2], ms.front(), ms.back(), total / (ms[2] * 1e-3));
    }
    const uint64_t perLaunch = meshsdf::triangles_per_launch(bricks, windingPairs, meshsdf::WINDING_PAIRS_PER_LAUNCH);
    const uint64_t launches = (nt + perLaunch - 1) / perLaunch;
    std::vector<float> ms;
    for (int rep = 0; rep < 7; ++rep) {
      CHECK(hipEventRecord(a, nullptr));
      CHECK(meshsdf::launch_winding<N>(nullptr, L, dRec, nt, meshsdf::FINISH_PHI, false, dSum, dOut, windingPairs));
      CHECK(hipEventRecord(b, nullptr));
      CHECK(hipEventSynchronize(b));
      float x = 0;
      CHECK(hipEventElapsedTime(&x, a, b));
      if (rep >= 2) ms.push_back(x);
      // (dOut now holds phi: put best back for the next repetition, outside the events)
      CHECK(meshsdf::launch_fold<N>(nullptr, L, dRec, dBnd, nt, true, false, slack, dOut, dSign, dTested, 0, true));
    }
    std::sort(ms.begin(), ms.end());
    const double rate = total / (ms[2] * 1e-3);
    std::printf("{\"type\": \"%s\", \"fold\": \"winding\", \"ms_median\": %.3f, \"ms_min\": %.3f, \"ms_max\": %.3f, \"launches\": %llu, "
                "\"triangles_per_launch\": %llu, \"ms_per_full_launch\": %.3f, \"pairs_per_s\": %.4g, \"distance_all_pairs_per_s\": %.4g, "
                "\"distance_pairs_per_winding_pair\": %.2f}\n",
                tag, ms[2], ms.front(), ms.back(), (unsigned long long)launches, (unsigned long long)perLaunch,
                double(perLaunch) * double(bricks) * 64.0 / rate * 1e3, rate, allPairsRate, allPairsRate / rate);
    std::fflush(stdout);
    CHECK(hipFree(dSum));
  }
  CHECK(hipFree(dRec));
  CHECK(hipFree(dBnd));
  CHECK(hipFree(dOut));
  CHECK(hipFree(dSign));
  CHECK(hipFree(dTested));
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  const int subdivisions = argc > 1 ? std::atoi(argv[1]) : 5;
  const uint32_t side = argc > 2 ? uint32_t(std::atoi(argv[2])) : 201u;
  const int log2Pairs = argc > 3 ? std::atoi(argv[3]) : 0;
  if (subdivisions < 0 || subdivisions > 6 || side < 2 || side > 512 || log2Pairs < 0 || log2Pairs > 40) {
    std::fprintf(stderr, "usage: mesh_sdf_rate [subdivisions 0..6] [nodes per axis 2..512] [log2 winding pairs per launch 1..40]\n");
    return 2;
  }
  const double centre[3] = {520, 500, 600};
  std::vector<double> v;
  std::vector<uint32_t> t;
  icosphere(subdivisions, 250.0, centre, v, t);
  const double spacing = 1000.0 / double(side - 1);
  const uint64_t windingPairs = log2Pairs ? uint64_t(1) << log2Pairs : 0;
  if (int rc = run<float>("fp32", v, t, side, spacing, windingPairs)) return rc;
  return run<double>("fp64", v, t, side, spacing, windingPairs);
}
