// obj_mesh.hpp — the minimal Wavefront OBJ reader behind `benchmark --collider=mesh:FILE.obj`: `v x y z` lines and triangular
// `f` lines whose corners are a, a/b, a//c or a/b/c (only the vertex index a is used; a negative index counts back from the
// vertices read so far).  Comments, blank lines and the lines a triangle mesh can carry without changing its shape (vn, vt,
// o, g, s, usemtl, mtllib) are skipped.  Anything else — a face with other than three corners, an index of 0 or out of
// range, a malformed number, an unknown keyword — is an error that names the file and the line.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace objmesh {

struct Mesh {
  std::vector<double> vertices;     // 3 per vertex
  std::vector<uint32_t> triangles;  // 3 per triangle, zero-based
};

inline Mesh read(const std::string &path) {
  std::ifstream in(path);
  if (!in) throw std::runtime_error("cannot open " + path);
  Mesh m;
  std::string line;
  size_t lineNo = 0;
  auto bad = [&](const std::string &what) { return std::runtime_error(path + ":" + std::to_string(lineNo) + ": " + what); };
  while (std::getline(in, line)) {
    ++lineNo;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    std::istringstream ss(line);
    std::string key;
    if (!(ss >> key) || key[0] == '#') continue;
    if (key == "v") {
      double x[3];
      if (!(ss >> x[0] >> x[1] >> x[2])) throw bad("expected v x y z");
      m.vertices.insert(m.vertices.end(), x, x + 3);
    } else if (key == "f") {
      std::string corner;
      std::vector<uint32_t> idx;
      while (ss >> corner) {
        const std::string a = corner.substr(0, corner.find('/'));
        char *end = nullptr;
        const long long i = std::strtoll(a.c_str(), &end, 10);
        const long long nv = (long long)(m.vertices.size() / 3);
        if (a.empty() || *end != '\0' || i == 0 || i > nv || i < -nv) throw bad("bad vertex index '" + corner + "'");
        idx.push_back(uint32_t(i > 0 ? i - 1 : nv + i));
      }
      if (idx.size() != 3) throw bad("only triangular faces are read (this one has " + std::to_string(idx.size()) + " corners)");
      m.triangles.insert(m.triangles.end(), idx.begin(), idx.end());
    } else if (key == "vn" || key == "vt" || key == "o" || key == "g" || key == "s" || key == "usemtl" || key == "mtllib") {
      continue;
    } else {
      throw bad("unsupported OBJ keyword '" + key + "'");
    }
  }
  if (m.vertices.empty() || m.triangles.empty()) throw std::runtime_error(path + ": no vertices or no faces");
  return m;
}

}  // namespace objmesh
