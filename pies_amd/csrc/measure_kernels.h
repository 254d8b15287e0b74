// Strain, volume and momentum measures (pies_measure_elements, pies_measure_nodes: extensions): the device side.  Both rules are
// stated in pies_hip.h.  Read-only: nothing here writes node state.  An element is one lane's work - the gather, F = P Qinv and
// svd3 of the tetrahedral projection (dev_math.h: the shared functions, not copies) - and the only thing that depends on an order
// between lanes is the summary: tiles of kMeasureTile consecutive element indices of the container reduced through LDS in
// ascending index, then the tiles in ascending index by a fold launch, without atomics.  The node sums take the props' tiling
// (prop_kernels.h: kPropTile consecutive HOST node ids) with records of their own width.  Launch wrappers like kernels.h: no
// allocation, no synchronisation, everything on the caller's stream.
#pragma once
#include "prop_kernels.h"

namespace pies {

constexpr uint32_t kMeasureTile = 256;       // element indices per workgroup and per first-level reduction (fixed: the order of the summary)
// one tile's record of the summary: volume, max stretch, min stretch, min j, max j, max green; the counts inverted, over, under,
// nonfinite; the elements that count (0: the five extremes are not set); one spare
constexpr uint32_t kMeasureTileWords = 12;
constexpr uint32_t kNodeSumWords = 16;       // one (tile, range) record and one folded range: pies_node_sums_t's 13 words, 3 spare
static_assert(sizeof(pies_node_sums_t) == 13 * sizeof(uint32_t), "pies_node_sums_t is 13 words without padding");
static_assert(sizeof(pies_element_measure_t) == 32, "an element's record is two 16-byte words");
static_assert(sizeof(pies_element_summary_t) == 10 * sizeof(uint32_t), "pies_element_summary_t is 10 words without padding");

inline uint32_t measure_tiles(uint32_t first, uint32_t n) {  // tiles of the container that [first, first + n) meets, n > 0
  return (first + (n - 1)) / kMeasureTile - first / kMeasureTile + 1;
}

struct ElementPass {
  const float4* pos = nullptr;  // the node positions the device holds
  // the container staged in HOST order with node ids in DEVICE numbering: upload_tets' layout (Qinv, lo, hi, w in three float4)
  const uint4* ids = nullptr;
  const float4 *q0 = nullptr, *q1 = nullptr, *q2 = nullptr;
  uint32_t first = 0, n = 0;    // the range, inside the container
  bool volume = false;          // PIES_VOLUME's limits (on the product of the stretches), else PIES_TET's
  pies_element_measure_t* out = nullptr;  // n records, or nullptr
  uint32_t* tileRecords = nullptr;        // measure_tiles(first, n) x kMeasureTileWords, or nullptr: no summary
};

// One lane per element index, one workgroup per tile of the container that the range meets.
void launch_measure_elements(hipStream_t st, const ElementPass& E);
// out[0 .. kMeasureTileWords): the tile records folded in ascending tile index (words 0-5 floats, 6-9 the counts, 10 the elements that count)
void launch_measure_elements_fold(hipStream_t st, const ElementPass& E, uint32_t* out);

struct MeasureRange {  // one range of pies_measure_nodes as the kernels read it
  uint32_t first, count;
  float about[3];
  uint32_t spare[3];
};
static_assert(sizeof(MeasureRange) == 32, "eight words");

struct NodeSumPass {
  NodeArrays nd;
  const uint32_t* inv = nullptr;         // host id -> device index of a renumbered scene (nullptr: identity)
  const MeasureRange* ranges = nullptr;  // nRanges records in HBM
  uint32_t nRanges = 0;
  float* tileSums = nullptr;             // per (tile, range) with a node of the range in the tile: kNodeSumWords words at (tile * nRanges + r)
};

// One lane per host node id, one workgroup per tile: the ranges staged in LDS once, position and velocity read once.
void launch_measure_nodes(hipStream_t st, const NodeSumPass& P);
// out[r * kNodeSumWords + c]: the records of range r's tiles folded in ascending tile index
void launch_measure_nodes_fold(hipStream_t st, const NodeSumPass& P, float* out);

}  // namespace pies
