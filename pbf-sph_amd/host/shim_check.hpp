// shim_check.hpp — what the test_*_shim programs share: the "ok <name>" / "FAIL <name>" lines the GPU tests parse, the count
// of failures behind the exit status, the bit-compare of two downloaded particle vectors and the closing "ALL OK" / "FAILED".
#pragma once

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace shim {

inline int failures = 0;

// `detail` (printf-style, optional) follows the name on a FAIL line
__attribute__((format(printf, 3, 4))) inline void check(const std::string &name, bool ok, const char *detail = nullptr, ...) {
  std::printf("%s %s", ok ? "ok" : "FAIL", name.c_str());
  if (!ok && detail) {
    va_list args;
    va_start(args, detail);
    std::printf(" ");
    std::vprintf(detail, args);
    va_end(args);
  }
  std::printf("\n");
  failures += ok ? 0 : 1;
}

// the same particles in the same order with the same bytes in every field
template <typename P> bool same_particles(const std::vector<P> &a, const std::vector<P> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].id != b[i].id || a[i].type != b[i].type || std::memcmp(&a[i].mass, &b[i].mass, sizeof(a[i].mass)) ||
        std::memcmp(&a[i].position, &b[i].position, sizeof(a[i].position)) ||
        std::memcmp(&a[i].velocity, &b[i].velocity, sizeof(a[i].velocity)) ||
        std::memcmp(&a[i].colour, &b[i].colour, sizeof(a[i].colour)))
      return false;
  return true;
}

// two arrays of plain values, byte for byte
template <typename A> bool same_bytes(const std::vector<A> &a, const std::vector<A> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(A)) == 0);
}

// main's last statement: the line the GPU tests look for, and the exit status
inline int finish() {
  std::printf(failures ? "FAILED %d\n" : "ALL OK\n", failures);
  return failures ? 1 : 0;
}

}  // namespace shim
