// pbf_solid_lattice.hpp — the signed-distance lattice of one solid: the buffer on the device and the geometry as given
// (pbf_collider_sdf, include/pbf_hip.h).  pbf_ctx holds two, the collider's (pbf_set_collider) and the scenery's
// (pbf_set_scenery); which kernels read them is ColliderState's business (pbf_collider_state.hpp), not this record's.
// The fields are read freely and changed through put() ONLY, which solid_install (pbf_hip.hip) alone calls
// (tests/test_collider_state_cpu.py holds it to that).  No HIP in here: the buffer's type is the includer's.
#pragma once

#include <cstdint>
#include <utility>

#include "pbf_hip.h"

namespace pbf {

template <typename Buf> struct SolidLattice {
  Buf phi;  // the lattice in N on the device, an allocation of its own, exactly sized; empty (p == NULL): no solid
  uint32_t dims[3] = {0, 0, 0};
  double origin[3] = {0, 0, 0}, spacing = 0, margin = 0;

  bool present() const { return phi.p != nullptr; }
  // `fresh` becomes the lattice (the old one is freed) with the geometry of `sdf`; sdf == NULL clears, and `fresh` is then empty
  void put(const pbf_collider_sdf *sdf, Buf &fresh) {
    phi = std::move(fresh);
    for (int a = 0; a < 3; ++a) dims[a] = sdf ? sdf->dims[a] : 0u, origin[a] = sdf ? sdf->origin[a] : 0.0;
    spacing = sdf ? sdf->spacing : 0.0, margin = sdf ? sdf->margin : 0.0;
  }
};

}  // namespace pbf
