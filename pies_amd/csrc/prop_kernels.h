// Kinematic props (pies_collide_props, an extension): the device side.  The rule for one (node, prop) pair is stated in pies_hip.h
// and lives in prop_rule.h; a node meets the props in ascending index, so a lane owns one node and nothing about the edit depends
// on an order between lanes.  The reaction sums do: they are taken in the fixed two-level order of the header - per tile of
// kPropTile consecutive HOST node ids in ascending id, then the tile sums in ascending tile index - without atomics, a function of
// the node count alone.  Launch wrappers like kernels.h: no allocation, no synchronisation, everything on the caller's stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pies_hip.h"
#include "kernels.h"

namespace pies {

constexpr uint32_t kPropTile = 256;    // host node ids per workgroup and per first-level sum (fixed: the order of the sums)
constexpr uint32_t kPropSumWords = 8;  // one (tile, prop) record: impulse x y z, torque x y z, the hit count's bits, one spare

inline uint32_t prop_tiles(uint32_t n) { return (n + kPropTile - 1) / kPropTile; }

struct PropPass {
  NodeArrays nd;                        // the state every schedule and both solvers start a substep from
  const uint32_t* inv = nullptr;        // host id -> device index of a renumbered scene (nullptr: identity)
  const pies_prop_t* props = nullptr;   // nProps records in HBM
  uint32_t nProps = 0;
  // the reaction, or nullptr: per tile the set of props that touched a node of it (bit k: prop k), and per (tile, prop) of that set
  // a record of kPropSumWords words at tileSums[(tile * nProps + k) * kPropSumWords]; records outside the set are not written
  uint64_t* tileMask = nullptr;
  float* tileSums = nullptr;
  uint32_t* nodeProp = nullptr;         // or nullptr: per host id the last prop that touched the node, PIES_PROP_NONE
};

// One lane per host node id, one workgroup per tile: the props staged in LDS once, the node's position and radius read, its
// velocity at the first touch; position, previous position and velocity stored on a touch only.
void launch_prop_collide(hipStream_t st, const PropPass& P);
// out[k * kPropSumWords + c]: the tile records of prop k folded in ascending tile index (c < 6 from 0.0f, c == 6 the hit count)
void launch_prop_fold(hipStream_t st, const PropPass& P, float* out);
// ... of nTiles tiles that are not tiles of node ids (anchor_kernels.h: tiles of anchor indices), nRecords <= PIES_PROP_MAX
void launch_prop_fold_tiles(hipStream_t st, const uint64_t* tileMask, const float* tileSums, uint32_t nTiles, uint32_t nRecords, float* out);

}  // namespace pies
