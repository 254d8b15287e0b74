// Surface loads (pies_apply_surface_loads, an extension): the device side.  The rule for one (triangle, load) pair is stated in
// pies_hip.h and lives in load_rule.h.  Three launches chained on the caller's stream: the ranges' volumes and areas per tile of
// kLoadTile container indices, the fold of the tiles that leaves V, A and the gas pressure per load in HBM, and the edit, a
// velocity edit like the forces' (node_edit_device.h) with their reaction (k_prop_fold) and commit launch (force_kernels.h).
// Launch wrappers like kernels.h: no allocation, no synchronisation.
#pragma once
#include "force_kernels.h"

namespace pies {

constexpr uint32_t kLoadTile = 256;  // container indices per workgroup and per first-level sum (fixed: the order of the sums)

// what the fold leaves per load for the evaluate launch: V_k, A_k, the pressure of a PRESSURE or GAS load and whether the load
// acts at all (a GAS load iff V_k > 0)
struct LoadState {
  float volume, area, pressure;
  uint32_t acts;
};

struct LoadPass {
  PropPass base;                               // nd, inv, nProps = the load count, the reaction's buffers (props and nodeProp unused)
  const pies_surface_load_t* loads = nullptr;  // base.nProps records in HBM, their ranges resolved (no UINT32_MAX count)
  float dt = 0.0f;
  SurfaceIncidence surface;                    // (force_kernels.h)
  // the measure: the tiles some range meets in ascending index, per (slot of that list, load) the tile's sums of six_t and
  // area_t - written for the loads whose range meets the tile only - and per load what the fold leaves
  const uint32_t* tiles = nullptr;
  uint32_t nSlots = 0;
  float2* tileSums = nullptr;  // nSlots x base.nProps
  LoadState* state = nullptr;  // base.nProps
  VelocityScratch scratch;  // (force_kernels.h) a list with a drag must use it
};

// one workgroup per slot, one lane per triangle of its tile: the tile's sums per load whose range meets it
void launch_load_measure(hipStream_t st, const LoadPass& P);
// one workgroup per load: the tile sums in ascending tile index, then V, A and the pressure to P.state
void launch_load_fold(hipStream_t st, const LoadPass& P);
// One lane per host node id, one workgroup per tile: the loads and their state staged in LDS, the node's row of the incidence
// walked per load; the reaction's tile sums when P.base.tileMask is set.  The scratch variant is committed by
// launch_velocity_commit (force_kernels.h).
void launch_load_evaluate(hipStream_t st, const LoadPass& P);

}  // namespace pies
