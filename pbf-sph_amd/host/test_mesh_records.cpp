// test_mesh_records — the mesh checks and records of csrc/pbf_mesh_records.hpp (pbf_mesh_records) on two meshes whose records
// can be written down by hand, in double and in float.  No HIP, not linked against the library.
//   box (300, 310, 320) - (700, 640, 820), 12 triangles: fu is +-an axis; the pseudonormal of an edge between two faces is the
//     sum of their axes, of a face's diagonal twice its axis; every vertex's is (pi / 2) (+-1, +-1, +-1), because the angles a
//     rectangular face contributes at a corner add up to a right angle however it is split; volume 66 000 000, 18 edges.
//   tetra corner (310, 290, 333), legs of 300 along the axes, 4 triangles: three axis faces and the face (1, 1, 1) / sqrt 3,
//     whose angles are pi / 3; at the corner (pi / 2) (-1, -1, -1); at the end of the x leg
//     (pi / (3 sqrt 3), pi / (3 sqrt 3) - pi / 4, pi / (3 sqrt 3) - pi / 4) and alike for y and z; volume 4 500 000, 6 edges.
// Then the refusals: one triangle removed, one flipped, one doubled, an index out of range, a NaN vertex — each with the
// matching count and the records buffer untouched.  Prints "ok <name>" / "FAIL <name>" lines and "ALL OK"; exit status 0 iff all ok.
#include <cmath>
#include <cstdint>
#include <cstdio>
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

Mesh tetra() {
  Mesh m;
  m.v = {310, 290, 333, 610, 290, 333, 310, 590, 333, 310, 290, 633};
  m.t = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};
  return m;
}

const double kPi = 3.14159265358979323846;

template <typename N> bool close3(const N *got, double x, double y, double z, double tol) {
  return std::fabs(double(got[0]) - x) <= tol && std::fabs(double(got[1]) - y) <= tol && std::fabs(double(got[2]) - z) <= tol;
}

// what both meshes share: the vertices copied exactly, fu a unit vector, each edge pseudonormal fu + a unit vector
template <typename N> bool sane(const Mesh &m, const std::vector<N> &rec, double tol) {
  bool ok = true;
  for (size_t k = 0; k < m.t.size() / 3; ++k) {
    const N *r = rec.data() + 30 * k;
    for (int s = 0; s < 3; ++s)
      for (int a = 0; a < 3; ++a) ok = ok && r[3 * s + a] == N(m.v[3 * m.t[3 * k + s] + a]);
    ok = ok && std::fabs(std::sqrt(double(r[9]) * r[9] + double(r[10]) * r[10] + double(r[11]) * r[11]) - 1) <= tol;
    for (int s = 0; s < 3; ++s) {
      const double d[3] = {double(r[12 + 3 * s]) - r[9], double(r[13 + 3 * s]) - r[10], double(r[14 + 3 * s]) - r[11]};
      ok = ok && std::fabs(std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) - 1) <= tol;
    }
  }
  return ok;
}

template <typename N> void run(const char *tag) {
  const double tol = sizeof(N) == 8 ? 1e-12 : 1e-6;
  const std::string name = tag;
  const char *why = nullptr;
  {
    const Mesh m = box();
    const pbf_mesh view = m.view();
    std::vector<N> rec(30 * 12);
    pbf_mesh_info info{};
    const int rc = meshsdf::build_records(&view, sizeof(N) == 8, rec.data(), &info, &why);
    check(name + "_box_accepted", rc == PBF_OK && info.n_edges == 18 && info.boundary_edges == 0 && info.nonmanifold_edges == 0 &&
                                      info.misoriented_edges == 0 && info.degenerate_triangles == 0);
    check(name + "_box_volume", info.volume == 66000000.0 && info.aabb_min[0] == 300 && info.aabb_min[1] == 310 && info.aabb_min[2] == 320 &&
                                    info.aabb_max[0] == 700 && info.aabb_max[1] == 640 && info.aabb_max[2] == 820);
    bool faces = true, edges = true, corners = true;
    for (size_t k = 0; k < 12; ++k) {
      const N *r = rec.data() + 30 * k;
      const int axis = int(k / 4) == 0 ? 0 : int(k / 4) == 1 ? 2 : 1;  // the quads: x, x, z, z, y, y
      const double sign = (k / 2) % 2 ? 1.0 : -1.0;
      double fu[3] = {0, 0, 0};
      fu[axis] = sign;
      faces = faces && close3(r + 9, fu[0], fu[1], fu[2], 0.0);
      for (int s = 0; s < 3; ++s) {
        // an edge pseudonormal: twice fu on the diagonal, else fu plus the axis normal of the face across
        const double e[3] = {double(r[12 + 3 * s]), double(r[13 + 3 * s]), double(r[14 + 3 * s])};
        const double l1 = std::fabs(e[0]) + std::fabs(e[1]) + std::fabs(e[2]);
        edges = edges && l1 == 2.0 && e[axis] == (std::fabs(e[axis]) == 2.0 ? 2 * sign : sign);
        const uint32_t v = m.t[3 * k + s];
        corners = corners && close3(r + 21 + 3 * s, (v & 1 ? 1 : -1) * kPi / 2, (v & 2 ? 1 : -1) * kPi / 2, (v & 4 ? 1 : -1) * kPi / 2, 4 * tol);
      }
    }
    check(name + "_box_face_normals", faces);
    check(name + "_box_edge_pseudonormals", edges);
    check(name + "_box_vertex_pseudonormals", corners);
    check(name + "_box_sane", sane(m, rec, tol));
  }
  {
    const Mesh m = tetra();
    const pbf_mesh view = m.view();
    std::vector<N> rec(30 * 4);
    pbf_mesh_info info{};
    const int rc = meshsdf::build_records(&view, sizeof(N) == 8, rec.data(), &info, &why);
    check(name + "_tetra_accepted", rc == PBF_OK && info.n_edges == 6 && info.volume == 4500000.0);
    const double o = 1 / std::sqrt(3.0), w = kPi / 3 * o;
    const double fu[4][3] = {{0, 0, -1}, {0, -1, 0}, {-1, 0, 0}, {o, o, o}};
    bool faces = true, corners = true;
    for (size_t k = 0; k < 4; ++k) faces = faces && close3(rec.data() + 30 * k + 9, fu[k][0], fu[k][1], fu[k][2], tol);
    const double vn[4][3] = {{-kPi / 2, -kPi / 2, -kPi / 2}, {w, w - kPi / 4, w - kPi / 4}, {w - kPi / 4, w, w - kPi / 4}, {w - kPi / 4, w - kPi / 4, w}};
    for (size_t k = 0; k < 4; ++k)
      for (int s = 0; s < 3; ++s) {
        const uint32_t v = m.t[3 * k + s];
        corners = corners && close3(rec.data() + 30 * k + 21 + 3 * s, vn[v][0], vn[v][1], vn[v][2], 4 * tol);
      }
    check(name + "_tetra_face_normals", faces);
    check(name + "_tetra_vertex_pseudonormals", corners);
    // the edge between two axis faces carries their sum; between an axis face and the oblique one, axis + (1, 1, 1) / sqrt 3
    check(name + "_tetra_edge_pseudonormals", close3(rec.data() + 12, -1.0, 0.0, -1.0, tol)           // triangle 0, edge 0 -> 2, across: face x
                                                  && close3(rec.data() + 15, o, o, o - 1, tol)        // edge 2 -> 1, across: the oblique face
                                                  && close3(rec.data() + 18, 0.0, -1.0, -1.0, tol));  // edge 1 -> 0, across: face y
    check(name + "_tetra_sane", sane(m, rec, tol));
  }
  {  // refusals
    const Mesh good = box();
    auto refused = [&](const Mesh &m, uint64_t pbf_mesh_info::*field, uint64_t count) {
      const pbf_mesh view = m.view();
      std::vector<N> rec(30 * (m.t.size() / 3), N(12345));
      pbf_mesh_info info{};
      const int rc = meshsdf::build_records(&view, sizeof(N) == 8, rec.data(), &info, &why);
      bool untouched = true;
      for (N x : rec) untouched = untouched && x == N(12345);
      return rc == PBF_ERR_INVALID && why && untouched && (!field || info.*field == count);
    };
    Mesh open = good, flipped = good, doubled = good, range = good, nan = good, flat = good;
    open.t.resize(open.t.size() - 3);
    std::swap(flipped.t[3], flipped.t[4]);
    doubled.t.insert(doubled.t.end(), good.t.begin() + 6, good.t.begin() + 9);
    range.t[5] = 8;
    nan.v[7] = std::nan("");
    flat.t[10] = flat.t[9];
    check(name + "_refuses_an_open_mesh", refused(open, &pbf_mesh_info::boundary_edges, 3));
    check(name + "_refuses_a_flipped_triangle", refused(flipped, &pbf_mesh_info::misoriented_edges, 3));
    check(name + "_refuses_a_doubled_triangle", refused(doubled, &pbf_mesh_info::nonmanifold_edges, 3));
    check(name + "_refuses_an_index_out_of_range", refused(range, &pbf_mesh_info::n_edges, 0));
    check(name + "_refuses_a_nan_vertex", refused(nan, &pbf_mesh_info::n_edges, 0));
    check(name + "_refuses_a_flat_triangle", refused(flat, &pbf_mesh_info::degenerate_triangles, 1));
    pbf_mesh none = good.view();
    none.n_triangles = 0;
    pbf_mesh_info info{};
    check(name + "_refuses_no_triangles", meshsdf::build_records(&none, 1, nullptr, &info, &why) == PBF_ERR_INVALID);
    check(name + "_refuses_null", meshsdf::build_records(nullptr, 1, nullptr, nullptr, &why) == PBF_ERR_INVALID);
  }
}

}  // namespace

int main() {
  run<double>("fp64");
  run<float>("fp32");
  return shim::finish();
}
