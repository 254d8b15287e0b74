// The reaction of a tile of kPropTile host node ids, shared by k_prop_collide (prop_kernels.hip) and k_field_collide
// (field_kernels.hip): from the props each lane's node was touched by, the tile's set of props (one 64-bit word per tile) and, for
// every prop of that set, the touches' impulses and torques summed in ascending node id - the first level of the order pies_hip.h
// states; k_prop_fold takes the second.  Included by .hip files only.
#pragma once
#include "prop_kernels.h"
#include "prop_rule.h"

namespace pies {

constexpr uint32_t kPropWaves = kPropTile / 64;

struct PropTileLds {
  uint64_t waveSet[kPropWaves];     // props that touched a node of the wave
  uint64_t waveBallot[kPropWaves];  // the wave's lanes the current prop touched
  float stage[6][kPropTile];        // ... and their impulse and torque
};

// Called by every lane of the workgroup (barriers inside) after the edit.  touchedBy: bit k set when prop k touched this lane's
// node.  retouch(k, T): the lane's touch by prop k once more, from the state the lane loaded - called for the props of touchedBy
// in ascending index, each on the state the previous call left; the same functions on the same operands as the edit, the same
// bits.  For every prop that touched the tile the impulses and torques go through LDS to six lanes, each of which adds one
// component in ascending node id (the touched lanes from the waves' ballots: an untouched node would add 0, which changes no bit
// of a sum that started at +0).  No atomics.
template <class Retouch>
PIES_DEV void prop_tile_sums(PropTileLds& lds, uint64_t* __restrict__ tileMask, float* __restrict__ tileSums, uint32_t nProps,
                             uint64_t touchedBy, Retouch&& retouch) {
  const uint32_t tid = threadIdx.x, wave = tid >> 6, tile = blockIdx.x;
  // ---- the tile's set of props ----
  uint64_t set = touchedBy;
  for (int offset = 32; offset > 0; offset >>= 1) set |= __shfl_xor(set, offset);
  if ((tid & 63u) == 0) lds.waveSet[wave] = set;
  __syncthreads();
  set = 0;
  for (uint32_t w = 0; w < kPropWaves; ++w) set |= lds.waveSet[w];
  if (tid == 0) tileMask[tile] = set;
  if (!set) return;  // (uniform: every lane read the same words)

  // ---- the tile's sums, prop after prop in the set ----
  for (uint32_t k = 0; k < nProps; ++k) {
    if (!((set >> k) & 1ull)) continue;  // (uniform)
    const bool touched = (touchedBy >> k) & 1ull;
    if (touched) {
      PropTouch T;
      retouch(k, T);
      lds.stage[0][tid] = T.impulse.x, lds.stage[1][tid] = T.impulse.y, lds.stage[2][tid] = T.impulse.z;
      lds.stage[3][tid] = T.torque.x, lds.stage[4][tid] = T.torque.y, lds.stage[5][tid] = T.torque.z;
    }
    const uint64_t ballot = __builtin_amdgcn_ballot_w64(touched);
    if ((tid & 63u) == 0) lds.waveBallot[wave] = ballot;
    __syncthreads();
    float* record = tileSums + (static_cast<size_t>(tile) * nProps + k) * kPropSumWords;
    if (tid < 6) {
      float sum = 0.0f;
      for (uint32_t w = 0; w < kPropWaves; ++w)
        for (uint64_t m = lds.waveBallot[w]; m; m &= m - 1) sum = sum + lds.stage[tid][w * 64 + __builtin_ctzll(m)];
      record[tid] = sum;
    } else if (tid == 6) {
      uint32_t hits = 0;
      for (uint32_t w = 0; w < kPropWaves; ++w) hits += __builtin_popcountll(lds.waveBallot[w]);
      reinterpret_cast<uint32_t*>(record)[6] = hits;
    }
    __syncthreads();  // the stage and the ballots are free for the next prop
  }
}

}  // namespace pies
