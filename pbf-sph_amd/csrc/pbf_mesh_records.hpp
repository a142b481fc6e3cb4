// pbf_mesh_records.hpp — the host half of the mesh collider (pbf_mesh_records, include/pbf_hip.h): a closed, consistently
// oriented triangle mesh checked and turned into the per-triangle records the field kernel (csrc/pbf_mesh_sdf.hpp) reads.
// Plain C++: no HIP and no library call in it, so host/test_mesh_records.cpp compiles it alone.
//
// The record of triangle k, 30 values, everything formed in double in the order written (built with -ffp-contract=off) and
// rounded to N once at the end:
//   [0..8]   a, b, c
//   [9..11]  fu = n / sqrt((n_x n_x + n_y n_y) + n_z n_z),  n = (b - a) x (c - a)
//   [12..20] the edge pseudonormals of ab, bc, ca: fu_k + fu_k' of the two triangles on the edge
//   [21..29] the vertex pseudonormals of a, b, c: 0 + the sum, over the triangles around the vertex in ascending triangle
//            index, of angle * fu, angle = atan2(|e1 x e2|, e1 . e2) with e1, e2 the triangle's two edges leaving the vertex
//            (at a: b - a, c - a; at b: c - b, a - b; at c: a - c, b - c)
// with u x v = (u_y v_z - u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x) and u . v = (u_x v_x + u_y v_y) + u_z v_z.
// Pseudonormals are not normalised: only the sign of r . n is used (Baerentzen & Aanaes 2005).
//
// The edge table is built by sorting the 3 nt directed edges by their undirected key: O(nt log nt).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "pbf_hip.h"

namespace meshsdf {

constexpr int RECORD = 30;       // values per triangle
constexpr int SOUP_RECORD = 9;   // values per triangle of a soup record (build_soup_records below): a, b, c alone

struct D3 {
  double x, y, z;
};
inline D3 sub(D3 u, D3 v) { return {u.x - v.x, u.y - v.y, u.z - v.z}; }
inline D3 cross(D3 u, D3 v) { return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }
inline double dot(D3 u, D3 v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }

struct Edge {  // one directed use of an undirected edge (lo < hi unless the triangle repeats an index)
  uint32_t lo, hi, tri;
  uint8_t slot, forward;  // slot: 0 ab, 1 bc, 2 ca; forward: the triangle runs it lo -> hi
};

// the 3 nt directed edges sorted by (lo, hi, triangle, slot): a run of equal (lo, hi) is one undirected edge
inline std::vector<Edge> sorted_edges(const uint32_t *T, size_t nt) {
  std::vector<Edge> E(3 * nt);
  for (size_t k = 0; k < nt; ++k)
    for (int s = 0; s < 3; ++s) {
      const uint32_t from = T[3 * k + s], to = T[3 * k + (s + 1) % 3];
      E[3 * k + s] = {std::min(from, to), std::max(from, to), uint32_t(k), uint8_t(s), uint8_t(from < to)};
    }
  std::sort(E.begin(), E.end(), [](const Edge &p, const Edge &q) {
    return p.lo != q.lo ? p.lo < q.lo : p.hi != q.hi ? p.hi < q.hi : p.tri != q.tri ? p.tri < q.tri : p.slot < q.slot;
  });
  return E;
}

// Checks the mesh and fills `info`; on success writes 30 * n_triangles values of N (fp64 ? double : float) to `records`
// (records == NULL: check only).  Returns PBF_OK or PBF_ERR_INVALID with *why set; a refused mesh leaves `records` untouched.
// What `info` holds after a refusal:
//   mesh / vertices / triangles NULL, a count zero or >= 2^31, a vertex that is not finite: all zero (nothing is measured);
//   an index >= n_vertices: aabb_min / aabb_max, the rest zero;
//   otherwise every field (degenerate_triangles, the edge counts, volume, the box).
inline int build_records(const pbf_mesh *mesh, int fp64, void *records, pbf_mesh_info *info, const char **why) {
  pbf_mesh_info I{};
  auto refuse = [&](const char *msg) {
    if (info) *info = I;
    *why = msg;
    return int(PBF_ERR_INVALID);
  };
  if (!mesh) return refuse("pbf_mesh_records: mesh == NULL");
  if (!mesh->vertices || !mesh->triangles) return refuse("pbf_mesh_records: vertices or triangles == NULL");
  if (mesh->n_vertices == 0 || mesh->n_triangles == 0) return refuse("pbf_mesh_records: no vertices or no triangles");
  if (mesh->n_vertices >= (uint64_t(1) << 31) || mesh->n_triangles >= (uint64_t(1) << 31))
    return refuse("pbf_mesh_records: 2^31 vertices or triangles, or more");
  const size_t nv = size_t(mesh->n_vertices), nt = size_t(mesh->n_triangles);
  const double *V = mesh->vertices;
  const uint32_t *T = mesh->triangles;
  for (size_t k = 0; k < 3 * nv; ++k)
    if (!std::isfinite(V[k])) return refuse("pbf_mesh_records: a vertex is not finite");
  for (int a = 0; a < 3; ++a) I.aabb_min[a] = I.aabb_max[a] = V[a];
  for (size_t v = 0; v < nv; ++v)
    for (int a = 0; a < 3; ++a) I.aabb_min[a] = std::min(I.aabb_min[a], V[3 * v + a]), I.aabb_max[a] = std::max(I.aabb_max[a], V[3 * v + a]);
  for (size_t k = 0; k < 3 * nt; ++k)
    if (T[k] >= nv) return refuse("pbf_mesh_records: a vertex index is out of range");
  auto vertex = [&](uint32_t i) { return D3{V[3 * size_t(i)], V[3 * size_t(i) + 1], V[3 * size_t(i) + 2]}; };

  // faces: unit normals, the degenerate count, the signed volume
  std::vector<D3> fu(nt);
  double six = 0;
  for (size_t k = 0; k < nt; ++k) {
    const D3 a = vertex(T[3 * k]), b = vertex(T[3 * k + 1]), c = vertex(T[3 * k + 2]);
    const D3 n = cross(sub(b, a), sub(c, a));
    const double len = std::sqrt(dot(n, n));
    if (!(len > 0)) I.degenerate_triangles++;
    fu[k] = {n.x / len, n.y / len, n.z / len};
    six += dot(a, cross(b, c));
  }
  I.volume = six / 6;

  // edges: sorted by (lo, hi, triangle); a run of equal (lo, hi) is one undirected edge
  const std::vector<Edge> E = sorted_edges(T, nt);
  std::vector<uint32_t> mate(3 * nt, 0);  // [3 k + slot] = the triangle across that edge (valid on an accepted mesh)
  for (size_t i = 0; i < E.size();) {
    size_t j = i + 1;
    while (j < E.size() && E[j].lo == E[i].lo && E[j].hi == E[i].hi) ++j;
    I.n_edges++;
    if (j - i == 1) I.boundary_edges++;
    else if (j - i > 2) I.nonmanifold_edges++;
    else if (E[i].forward == E[i + 1].forward) I.misoriented_edges++;
    else mate[3 * size_t(E[i].tri) + E[i].slot] = E[i + 1].tri, mate[3 * size_t(E[i + 1].tri) + E[i + 1].slot] = E[i].tri;
    i = j;
  }
  if (I.degenerate_triangles) return refuse("pbf_mesh_records: a triangle has zero area");
  if (I.boundary_edges) return refuse("pbf_mesh_records: the mesh is open (an edge with one triangle)");
  if (I.nonmanifold_edges) return refuse("pbf_mesh_records: an edge is shared by more than two triangles");
  if (I.misoriented_edges) return refuse("pbf_mesh_records: two triangles run a shared edge the same way (inconsistent orientation)");
  if (info) *info = I;
  if (!records) return PBF_OK;

  // vertex pseudonormals: triangles in ascending index, so each vertex's sum is in that order
  std::vector<D3> vn(nv, D3{0, 0, 0});
  for (size_t k = 0; k < nt; ++k) {
    const D3 p[3] = {vertex(T[3 * k]), vertex(T[3 * k + 1]), vertex(T[3 * k + 2])};
    for (int s = 0; s < 3; ++s) {
      const D3 e1 = sub(p[(s + 1) % 3], p[s]), e2 = sub(p[(s + 2) % 3], p[s]);
      const D3 x = cross(e1, e2);
      const double angle = std::atan2(std::sqrt(dot(x, x)), dot(e1, e2));
      D3 &acc = vn[T[3 * k + s]];
      acc = {acc.x + angle * fu[k].x, acc.y + angle * fu[k].y, acc.z + angle * fu[k].z};
    }
  }
  auto put = [&](size_t at, double v) {
    if (fp64) static_cast<double *>(records)[at] = v;
    else static_cast<float *>(records)[at] = float(v);
  };
  auto put3 = [&](size_t at, D3 v) { put(at, v.x), put(at + 1, v.y), put(at + 2, v.z); };
  for (size_t k = 0; k < nt; ++k) {
    const size_t r = size_t(RECORD) * k;
    for (int s = 0; s < 3; ++s) {
      put3(r + 3 * s, vertex(T[3 * k + s]));
      const D3 o = fu[mate[3 * k + s]];
      put3(r + 12 + 3 * s, D3{fu[k].x + o.x, fu[k].y + o.y, fu[k].z + o.z});
      put3(r + 21 + 3 * s, vn[T[3 * k + s]]);
    }
    put3(r + 9, fu[k]);
  }
  return PBF_OK;
}

// The cull's bounding spheres, 4 values of N per triangle {m, R}: internal to pbf_sdf_from_mesh, not part of the record.
// m = N(the centre of the triangle's box); R = the largest |N(vertex) - N(m)| in double, widened by (1 + 2^-20) and by `pad`
// and rounded UP to N.  `pad` is the absolute slack of the kernel's skip test (csrc/pbf_mesh_sdf.hpp states the argument).
// `stride` = values per record (RECORD, or SOUP_RECORD for a soup): a, b, c lead either.
template <typename N> void build_bounds(const N *records, size_t nt, int stride, double pad, N *bounds) {
  for (size_t k = 0; k < nt; ++k) {
    const N *r = records + size_t(stride) * k;
    double m[3], R = 0;
    for (int a = 0; a < 3; ++a) {
      const double lo = std::min({double(r[a]), double(r[3 + a]), double(r[6 + a])});
      const double hi = std::max({double(r[a]), double(r[3 + a]), double(r[6 + a])});
      bounds[4 * k + a] = N(lo + (hi - lo) / 2);
      m[a] = double(bounds[4 * k + a]);
    }
    for (int s = 0; s < 3; ++s) {
      const D3 d{double(r[3 * s]) - m[0], double(r[3 * s + 1]) - m[1], double(r[3 * s + 2]) - m[2]};
      R = std::max(R, std::sqrt(dot(d, d)));
    }
    R = R * (1.0 + 1.0 / 1048576.0) + pad;
    N up = N(R);
    if (double(up) < R) up = std::nextafter(up, N(INFINITY));
    bounds[4 * k + 3] = up;
  }
}

// pbf_mesh_soup_records: the mesh as a triangle soup for the winding-number sign (PBF_MESH_SIGN_WINDING, csrc/pbf_mesh_winding.hpp).
// A record is a, b, c formed in double and rounded to N once: 9 values per triangle.  Only what the kernels cannot survive
// is refused; boundary, non-manifold and misoriented edges are counted into `info` and accepted.  `info` after a refusal
// holds what build_records leaves there in the same case; on success every field.  records == NULL: check only.
inline int build_soup_records(const pbf_mesh *mesh, int fp64, void *records, pbf_mesh_info *info, const char **why) {
  pbf_mesh_info I{};
  auto refuse = [&](const char *msg) {
    if (info) *info = I;
    *why = msg;
    return int(PBF_ERR_INVALID);
  };
  if (!mesh) return refuse("pbf_mesh_soup_records: mesh == NULL");
  if (!mesh->vertices || !mesh->triangles) return refuse("pbf_mesh_soup_records: vertices or triangles == NULL");
  if (mesh->n_vertices == 0 || mesh->n_triangles == 0) return refuse("pbf_mesh_soup_records: no vertices or no triangles");
  if (mesh->n_vertices >= (uint64_t(1) << 31) || mesh->n_triangles >= (uint64_t(1) << 31))
    return refuse("pbf_mesh_soup_records: 2^31 vertices or triangles, or more");
  const size_t nv = size_t(mesh->n_vertices), nt = size_t(mesh->n_triangles);
  const double *V = mesh->vertices;
  const uint32_t *T = mesh->triangles;
  for (size_t k = 0; k < 3 * nv; ++k)
    if (!std::isfinite(V[k])) return refuse("pbf_mesh_soup_records: a vertex is not finite");
  for (int a = 0; a < 3; ++a) I.aabb_min[a] = I.aabb_max[a] = V[a];
  for (size_t v = 0; v < nv; ++v)
    for (int a = 0; a < 3; ++a) I.aabb_min[a] = std::min(I.aabb_min[a], V[3 * v + a]), I.aabb_max[a] = std::max(I.aabb_max[a], V[3 * v + a]);
  for (size_t k = 0; k < 3 * nt; ++k)
    if (T[k] >= nv) return refuse("pbf_mesh_soup_records: a vertex index is out of range");
  auto vertex = [&](uint32_t i) { return D3{V[3 * size_t(i)], V[3 * size_t(i) + 1], V[3 * size_t(i) + 2]}; };

  double six = 0;
  for (size_t k = 0; k < nt; ++k) {
    const D3 a = vertex(T[3 * k]), b = vertex(T[3 * k + 1]), c = vertex(T[3 * k + 2]);
    const D3 n = cross(sub(b, a), sub(c, a));
    if (!(std::sqrt(dot(n, n)) > 0)) I.degenerate_triangles++;
    six += dot(a, cross(b, c));
  }
  I.volume = six / 6;

  // the edge counts, as build_records forms them: reports here, not refusals
  const std::vector<Edge> E = sorted_edges(T, nt);
  for (size_t i = 0; i < E.size();) {
    size_t j = i + 1;
    while (j < E.size() && E[j].lo == E[i].lo && E[j].hi == E[i].hi) ++j;
    I.n_edges++;
    if (j - i == 1) I.boundary_edges++;
    else if (j - i > 2) I.nonmanifold_edges++;
    else if (E[i].forward == E[i + 1].forward) I.misoriented_edges++;
    i = j;
  }
  if (I.degenerate_triangles) return refuse("pbf_mesh_soup_records: a triangle has zero area");
  if (info) *info = I;
  if (!records) return PBF_OK;
  for (size_t k = 0; k < nt; ++k)
    for (int s = 0; s < 3; ++s)
      for (int a = 0; a < 3; ++a) {
        const size_t at = size_t(SOUP_RECORD) * k + 3 * s + a;
        const double x = V[3 * size_t(T[3 * k + s]) + a];
        if (fp64) static_cast<double *>(records)[at] = x;
        else static_cast<float *>(records)[at] = float(x);
      }
  return PBF_OK;
}

}  // namespace meshsdf
