// test_mesh_soup_records — the soup's checks and records of csrc/pbf_mesh_records.hpp (build_soup_records, behind
// pbf_mesh_soup_records) on the box of test_mesh_records, in double and in float.  No HIP, not linked against the library.
//   the box (300, 310, 320) - (700, 640, 820), 12 triangles: a record is the triangle's three corners, copied; 18 edges,
//     volume 66 000 000.
//   spoilt by hand and ACCEPTED, with the count that says so and everything else measured: the last triangle removed (3
//     boundary edges, 18 edges still: the diagonal and two box edges lose a use), triangle 1 flipped (3 misoriented edges),
//     triangle 2 doubled (3 non-manifold edges).
//   REFUSED, each with its message, `info` as stated in include/pbf_hip.h and the records buffer untouched: an index out of
//     range (the box of the vertices, the rest zero), a NaN vertex (all zero), a triangle of zero area (every field,
//     degenerate_triangles 1), no triangles, NULL.
// Prints "ok <name>" / "FAIL <name>" lines and "ALL OK"; exit status 0 iff all ok.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pbf_mesh_records.hpp"
#include "shim_check.hpp"

using shim::check;

namespace {

struct Mesh {
  std::vector<double> v;
  std::vector<uint32_t> t;
  pbf_mesh view() const { return pbf_mesh{v.size() / 3, t.size() / 3, v.data(), t.data()}; }
};

Mesh box() {
  const double lo[3] = {300, 310, 320}, hi[3] = {700, 640, 820};
  Mesh m;
  for (int n = 0; n < 8; ++n)
    for (int a = 0; a < 3; ++a) m.v.push_back(((n >> a) & 1) ? hi[a] : lo[a]);
  const uint32_t quads[6][4] = {{0, 2, 6, 4}, {1, 5, 7, 3}, {0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1}, {2, 3, 7, 6}};
  for (const auto &q : quads)
    for (uint32_t i : {q[0], q[2], q[1], q[0], q[3], q[2]}) m.t.push_back(i);
  return m;
}

bool box_of(const pbf_mesh_info &i) {
  return i.aabb_min[0] == 300 && i.aabb_min[1] == 310 && i.aabb_min[2] == 320 && i.aabb_max[0] == 700 && i.aabb_max[1] == 640 &&
         i.aabb_max[2] == 820;
}
bool all_zero(const pbf_mesh_info &i) {
  const pbf_mesh_info z{};
  return std::memcmp(&i, &z, sizeof z) == 0;
}
bool counts(const pbf_mesh_info &i, uint64_t edges, uint64_t boundary, uint64_t nonmanifold, uint64_t misoriented, uint64_t degenerate) {
  return i.n_edges == edges && i.boundary_edges == boundary && i.nonmanifold_edges == nonmanifold && i.misoriented_edges == misoriented &&
         i.degenerate_triangles == degenerate;
}

template <typename N> void run(const char *tag) {
  const std::string name = tag;
  const int fp64 = sizeof(N) == 8;
  const Mesh good = box();

  // accepted: -> (rc == OK, the records are the corners rounded once, info)
  auto accepted = [&](const Mesh &m, pbf_mesh_info *info) {
    const pbf_mesh view = m.view();
    const size_t nt = m.t.size() / 3;
    std::vector<N> rec(9 * nt, N(12345));
    const char *why = nullptr;
    std::memset(info, 0xAB, sizeof *info);
    bool ok = meshsdf::build_soup_records(&view, fp64, rec.data(), info, &why) == PBF_OK;
    for (size_t k = 0; k < nt && ok; ++k)
      for (int s = 0; s < 3; ++s)
        for (int a = 0; a < 3; ++a) ok = ok && rec[9 * k + 3 * s + a] == N(m.v[3 * m.t[3 * k + s] + a]);
    pbf_mesh_info only{};
    std::memset(&only, 0xAB, sizeof only);
    ok = ok && meshsdf::build_soup_records(&view, fp64, nullptr, &only, &why) == PBF_OK && std::memcmp(&only, info, sizeof only) == 0;
    return ok && meshsdf::build_soup_records(&view, fp64, nullptr, nullptr, &why) == PBF_OK;
  };
  pbf_mesh_info info;
  check(name + "_box_accepted", accepted(good, &info) && counts(info, 18, 0, 0, 0, 0) && info.volume == 66000000.0 && box_of(info));
  Mesh open = good, flipped = good, doubled = good;
  open.t.resize(open.t.size() - 3);
  std::swap(flipped.t[3], flipped.t[4]);
  doubled.t.insert(doubled.t.end(), good.t.begin() + 6, good.t.begin() + 9);
  check(name + "_accepts_an_open_mesh", accepted(open, &info) && counts(info, 18, 3, 0, 0, 0) && box_of(info) && info.volume < 66000000.0);
  check(name + "_accepts_a_flipped_triangle", accepted(flipped, &info) && counts(info, 18, 0, 0, 3, 0) && box_of(info));
  check(name + "_accepts_a_doubled_triangle", accepted(doubled, &info) && counts(info, 18, 0, 3, 0, 0) && box_of(info));

  // refused: -> (rc, the message, the buffer untouched); info is left for the caller to judge
  auto refused = [&](const pbf_mesh *view, size_t nt, const char *message, pbf_mesh_info *out) {
    std::vector<N> rec(9 * (nt ? nt : 1), N(12345));
    const char *why = nullptr;
    if (out) std::memset(out, 0xAB, sizeof *out);
    const int rc = meshsdf::build_soup_records(view, fp64, rec.data(), out, &why);
    bool untouched = true;
    for (N x : rec) untouched = untouched && x == N(12345);
    if (why && std::string(why) != message) std::printf("   got \"%s\"\n", why);
    return rc == PBF_ERR_INVALID && why && std::string(why) == message && untouched;
  };
  Mesh range = good, nan = good, flat = good;
  range.t[5] = 8;
  nan.v[7] = std::nan("");
  flat.t[10] = flat.t[9];
  pbf_mesh view = range.view();
  check(name + "_refuses_an_index_out_of_range",
        refused(&view, 12, "pbf_mesh_soup_records: a vertex index is out of range", &info) && box_of(info) && counts(info, 0, 0, 0, 0, 0) &&
            info.volume == 0);
  view = nan.view();
  check(name + "_refuses_a_nan_vertex", refused(&view, 12, "pbf_mesh_soup_records: a vertex is not finite", &info) && all_zero(info));
  view = flat.view();
  check(name + "_refuses_a_flat_triangle",
        refused(&view, 12, "pbf_mesh_soup_records: a triangle has zero area", &info) && info.degenerate_triangles == 1 && info.n_edges > 0 &&
            info.boundary_edges > 0 && box_of(info) && info.volume != 0);
  view = good.view();
  view.n_triangles = 0;
  check(name + "_refuses_no_triangles", refused(&view, 12, "pbf_mesh_soup_records: no vertices or no triangles", &info) && all_zero(info));
  view = good.view();
  view.n_vertices = uint64_t(1) << 31;
  check(name + "_refuses_2^31_vertices", refused(&view, 12, "pbf_mesh_soup_records: 2^31 vertices or triangles, or more", &info) && all_zero(info));
  view = good.view();
  view.vertices = nullptr;
  check(name + "_refuses_null_vertices", refused(&view, 12, "pbf_mesh_soup_records: vertices or triangles == NULL", &info) && all_zero(info));
  check(name + "_refuses_null", refused(nullptr, 0, "pbf_mesh_soup_records: mesh == NULL", nullptr));
}

}  // namespace

int main() {
  run<double>("fp64");
  run<float>("fp32");
  return shim::finish();
}
