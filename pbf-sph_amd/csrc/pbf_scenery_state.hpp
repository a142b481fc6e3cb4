// pbf_scenery_state.hpp — the scenery (pbf_set_scenery, include/pbf_hip.h): ONE static lattice in the world frame beside the
// collider.  It has no pose, no reaction, no friction and no body, so unlike ColliderState (pbf_collider_state.hpp) there are
// no modes to own and no rules between them: the buffer, the geometry as given and a generation.  Fields only, no logic —
// the one function that changes them is scenery_install (pbf_hip.hip).  No HIP in here: the buffer's type is the includer's.
//
// `gen` is part of a captured step's key (GraphKey::scenery).  Every install, a replacement and a clear included, bumps it
// and destroys the captured graphs: a replay never runs on a replaced or freed lattice.
#pragma once

#include <cstdint>

namespace pbf {

template <typename Buf> struct SceneryState {
  Buf phi;  // the lattice in N on the device, an allocation of its own, exactly sized; empty (p == NULL): no scenery
  uint32_t dims[3] = {0, 0, 0};
  double origin[3] = {0, 0, 0}, spacing = 0, margin = 0;
  uint64_t gen = 0;  // installs so far
};

}  // namespace pbf
