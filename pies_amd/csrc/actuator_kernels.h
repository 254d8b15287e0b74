// Actuators (pies_add_actuators / pies_drive_actuators, extensions): the device side.  The rule for one actuator is stated in
// pies_hip.h and lives in actuator_rule.h.  A set is a persistent asset in HBM in its own order, every record naming the SLOT of
// its constraint in the plan-ordered rest records (d_dc_rw / d_bc_aw, device_scene.cpp); a lane owns one actuator, no two actuators
// of a set share a constraint, and nothing about the edit depends on an order between lanes.  The channel sums do: they are taken
// in the fixed two-level order of the header - per tile of kActuatorTile consecutive actuator indices in ascending index, then
// the tile records in ascending tile index - without atomics, a function of the set alone.  Launch wrappers like kernels.h: no
// allocation, no synchronisation, everything on the caller's stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pies_hip.h"

namespace pies {

constexpr uint32_t kActuatorTile = 256;      // actuator indices per workgroup and per first-level sum (fixed: the order of the sums)
constexpr uint32_t kActuatorTileWords = 3;   // one (tile, channel) record: the value sum's bits, the rest sum's bits, the live count

struct ActuatorRecord {  // pies_actuator_t with the host index replaced by the slot of the plan the device holds
  int32_t type;
  uint32_t slot;
  uint32_t channel;
  float gain, lo, hi, base;
  uint32_t flags;
};
static_assert(sizeof(ActuatorRecord) == 32 && sizeof(pies_actuator_t) == 32, "eight words without padding");

inline uint32_t actuator_tiles(uint32_t n) { return (n + kActuatorTile - 1) / kActuatorTile; }

struct ActuatorPass {
  const float4* pos = nullptr;       // node positions, device numbering (read only)
  const uint2* dcIds = nullptr;      // distance constraints in plan order: node ids in device numbering ...
  float2* dcRw = nullptr;            // ... and (rest length, w): .x is written
  const uint4* bcIds = nullptr;      // bend constraints likewise
  float2* bcAw = nullptr;            // (rest angle, w): .x is written
  const ActuatorRecord* records = nullptr;
  uint32_t nActuators = 0, nChannels = 0;
  const float* activation = nullptr;  // nChannels words in HBM
  float2* outActuator = nullptr;      // or nullptr: per actuator (the rest its constraint holds after the call, value)
  uint32_t* tileRecords = nullptr;    // or nullptr: per (tile, channel) kActuatorTileWords words, every record written
};

// One lane per actuator, one workgroup per tile.  A live actuator stores its constraint's rest word; with tileRecords the workgroup
// then adds, per channel, the values and rests of the tile's live actuators in ascending index from 0.0f and counts them.
void launch_actuator_drive(hipStream_t st, const ActuatorPass& P);
// outSums[2 c], outSums[2 c + 1]: the tile records of channel c added in ascending tile index from 0.0f; outLive[c]: the counts
// added.  Either may be nullptr.
void launch_actuator_fold(hipStream_t st, const uint32_t* tileRecords, uint32_t nTiles, uint32_t nChannels, float* outSums, uint32_t* outLive);

}  // namespace pies
