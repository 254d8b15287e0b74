// Ties (pies_add_ties / pies_apply_ties, extensions): the device side.  The rule is stated in pies_hip.h and lives in tie_rule.h.  A
// tie couples four nodes - the tied node a and the three carriers of the point q - and a node may carry many ties, so a call is an
// iteration of two launches: k_tie_evaluate, one lane per TIE, reads the velocities the previous iteration left and writes the
// tie's impulse change; k_tie_scatter, one lane per TIED NODE, walks the node's row of the set's CSR in ascending tie index and
// stores the velocity in place.  No lane writes what another lane of the same launch reads, nothing is summed with atomics, and the
// order of every sum is a function of the set alone.  The reaction sums are the anchors': k_anchor_sums over tiles of kPropTile tie
// indices, then k_prop_fold.  Launch wrappers like kernels.h: no allocation, no synchronisation, everything on the caller's stream.
#pragma once
#include "anchor_kernels.h"

namespace pies {

struct TieRecord {  // one tie as the device reads it: pies_tie_t with the set's counts (pies_hip.h: cnt_v) as floats, four uint4
  uint32_t node, to[3];  // HOST ids (P.inv gives the device index under renumbering)
  float weight[3], stiffness;
  float damping;
  uint32_t group;
  float cntNode, cntTo[3];  // cnt of node and of to[j], whether weight[j] is 0 or not (a zero weight wipes its term)
  uint32_t spare[2];
};
static_assert(sizeof(TieRecord) == 64 && sizeof(pies_tie_t) == 40, "sixteen and ten words without padding");
static_assert(sizeof(pies_tie_group_t) == 20, "pies_tie_group_t is 5 words without padding");
static_assert(PIES_TIE_GROUP_MAX <= PIES_ANCHOR_FRAME_MAX, "the sums and the fold are the anchors': a group's index is six bits");

struct TieEntry {  // one (tie, slot) entry of a node's row: the coefficient is +1 for slot a, -weight_j for to[j]
  uint32_t tie;
  float coefficient;
};

struct TiePass {
  PropPass base;  // nd, inv, nProps = the group count, tileMask / tileSums per tile of TIE indices (props and nodeProp unused)
  const pies_tie_group_t* groups = nullptr;  // base.nProps records in HBM
  float dt = 0.0f;
  // the set
  uint32_t nTies = 0, nNodes = 0;
  const TieRecord* records = nullptr;
  uint8_t* broken = nullptr;           // per tie: 1 once it broke
  const uint32_t* nodes = nullptr;     // nNodes tied host ids, ascending
  const uint32_t* offsets = nullptr;   // nNodes + 1
  const TieEntry* entries = nullptr;   // a node's row: ascending tie index
  // the call, per tie in the set's own order
  float4* delta = nullptr;    // (the iteration's change of J, 1u when the tie is live else 0u)
  float4* impulse = nullptr;  // (J, stretch)
  float4* scratch = nullptr;  // 2 per tie, written by the first iteration: (x, den) and (q - pivot, group | live bit)
  float4* torque = nullptr;   // or nullptr: (cross(q - pivot, J), group | live bit), written by the last iteration
};

// Iteration `first` .. `last` flags: the first reads the positions and decides broken and live, the last writes P.torque.  With
// P.dt == 0 the tie's J stays 0 (the host launches no scatter then).
void launch_tie_evaluate(hipStream_t st, const TiePass& P, bool first, bool last);
// v = v + (sum of the live entries' delta * coefficient) * w for every tied node with w != 0 and a live entry
void launch_tie_scatter(hipStream_t st, const TiePass& P);
// the anchors' tile sums over P.impulse / P.torque (needs base.tileMask and base.tileSums)
void launch_tie_sums(hipStream_t st, const TiePass& P);

}  // namespace pies
