// Anchors (pies_add_anchors / pies_apply_anchors, extensions): the device side.  The rule for one node and its anchors is stated in
// pies_hip.h and lives in anchor_rule.h.  Unlike the record lists of the other node edits (at most 64, staged whole in LDS) a set
// is as long as a rim or a seam: it is a persistent asset in HBM, sorted by node, and a lane owns one ANCHORED node - it walks
// that node's records and nothing about the edit depends on an order between lanes.  The reaction sums do: they are taken in the
// fixed two-level order of the header - per tile of kPropTile consecutive ANCHOR indices of the set's own order in ascending index,
// then the tile sums in ascending tile index (k_prop_fold) - without atomics, a function of the set alone.  Launch wrappers like
// kernels.h: no allocation, no synchronisation, everything on the caller's stream.
#pragma once
#include "prop_kernels.h"

namespace pies {

struct AnchorRecord {  // one anchor in the sorted list: pies_anchor_t with the node (the list's row) replaced by the index
  uint32_t frame;
  float local[3];
  float stiffness, damping;
  uint32_t flags;
  uint32_t index;  // in the set's own order
};
static_assert(sizeof(AnchorRecord) == 32 && sizeof(pies_anchor_t) == 32, "eight words without padding");
static_assert(sizeof(pies_anchor_frame_t) == 88, "pies_anchor_frame_t is 22 words without padding");
static_assert(PIES_ANCHOR_FRAME_MAX <= PIES_PROP_MAX, "the fold's buffers and the 64-bit tile word are the props'");

constexpr uint32_t kAnchorLiveBit = 0x80000000u;  // of the word beside an anchor's torque: the anchor was live; below it the frame

inline uint32_t anchor_tiles(uint32_t n) { return (n + kPropTile - 1) / kPropTile; }

struct AnchorPass {
  PropPass base;  // nd, inv, nProps = the frame count, tileMask / tileSums per tile of ANCHOR indices (props and nodeProp unused)
  const pies_anchor_frame_t* frames = nullptr;  // base.nProps records in HBM
  float dt = 0.0f;
  // the set
  uint32_t nAnchors = 0, nNodes = 0;
  const uint32_t* nodes = nullptr;      // nNodes anchored host ids, ascending
  const uint32_t* offsets = nullptr;    // nNodes + 1
  const AnchorRecord* records = nullptr;
  // the second walk's output in the set's own order, or nullptr (both or neither): (j, stretch) and (torque, frame | live bit)
  float4* impulse = nullptr;
  float4* torque = nullptr;
};

// One lane per anchored node, one workgroup per kPropTile of them: the frames staged in LDS once, the node's position read, its
// velocity at the first live anchor; the velocity (a pin: position and previous position too) stored for a node with a live anchor
// only.  With P.impulse set every lane walks its records a second time and writes every anchor's entry.
void launch_anchor_evaluate(hipStream_t st, const AnchorPass& P);
// One workgroup per tile of kPropTile anchor indices: base.tileMask[tile] = the frames present, and per present frame the record of
// kPropSumWords words k_prop_fold reads (impulse, torque, the live count's bits).  Needs P.impulse and base.tileMask.
void launch_anchor_sums(hipStream_t st, const AnchorPass& P);

}  // namespace pies
