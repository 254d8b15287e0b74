// Floor friction of one node (Solver.cpp:473-484): once per floor contact of the node, perpVel = (vx, 0, vz).  The one statement of
// it: k_pd_velocity applies it to the nodes in no contact, the sequential passes of the point-triangle contacts, the node-node
// contacts and the listed node pairs to their own nodes, after their friction.
#pragma once
#include <cstdint>

#include "dev_math.h"

namespace pies {

PIES_DEV void floor_friction(float& vx, float& vy, float& vz, uint32_t ns, float friction, float staticThreshold) {
  for (uint32_t c = 0; c < ns; ++c) {
    const float px = vx, pz = vz;
    float fr = friction;
    if (sqrtf(px * px + 0.0f * 0.0f + pz * pz) < staticThreshold) fr = 1.0f;
    vx += -fr * px;
    vy += -fr * 0.0f;
    vz += -fr * pz;
  }
}

}  // namespace pies
