// Force fields (pies_apply_forces, an extension): the device side.  The rule for one (node, force) and one (triangle, force) pair
// is stated in pies_hip.h and lives in force_rule.h.  Every force reads the state the call found, so a lane owns one node and the
// only thing that depends on an order between lanes is the wind's read of its neighbours' velocities: the new velocities then go
// to a scratch array and a second launch commits them.  The reaction sums are the props' (prop_kernels.h): tiles of kPropTile
// consecutive HOST node ids, then the tiles, without atomics.  Launch wrappers like kernels.h: no allocation, no synchronisation,
// everything on the caller's stream.
#pragma once
#include "prop_kernels.h"

namespace pies {

constexpr uint32_t kForceWaves = kPropTile / 64;  // words of VelocityScratch::affected per tile

// What a velocity edit that reads triangles walks (forces with a wind, surface loads): the scene's triangles in DEVICE numbering
// and the node -> triangle incidence by HOST node id, CSR, one entry per (triangle, corner) that names the node, ascending triangle
// index within a row
struct SurfaceIncidence {
  const uint32_t* tri = nullptr;
  uint32_t nTris = 0;
  const uint32_t* incPtr = nullptr;  // nd.n + 1
  const uint32_t* inc = nullptr;
};

// The scratch variant of a velocity edit (newVel nullptr: the evaluate launch writes nd.vel in place, which a list whose lanes
// read other nodes' velocities must not): the new velocity per HOST node id, written for affected nodes only, and per wavefront of
// the evaluate launch the lanes it affected
struct VelocityScratch {
  float4* newVel = nullptr;
  uint64_t* affected = nullptr;  // kForceWaves words per tile
};

struct ForcePass {
  PropPass base;                         // nd, inv, nProps = the force count, the reaction's buffers (props and nodeProp unused)
  const pies_force_t* forces = nullptr;  // base.nProps records in HBM
  float dt = 0.0f;
  SurfaceIncidence surface;  // the wind's (unset without one)
  VelocityScratch scratch;   // a list with a wind must use it
};

// One lane per host node id, one workgroup per tile: the forces staged in LDS once, the node's position read, its velocity at the
// first force that affects it; the reaction's tile sums when P.base.tileMask is set.
void launch_force_evaluate(hipStream_t st, const ForcePass& P);
// The second launch of any velocity edit's scratch variant (forces, surface loads): newVel -> nd.vel for the affected nodes.
// Nothing without a scratch array.
void launch_velocity_commit(hipStream_t st, const NodeArrays& nd, const uint32_t* inv, const VelocityScratch& scratch);

}  // namespace pies
