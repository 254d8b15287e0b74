// Kinematic props (prop_kernels.h; the rule is stated in pies_hip.h, lives in prop_rule.h and is restated in numpy by
// tests/test_props.py).
//  k_prop_collide  a collide edit (node_edit_device.h: collide_pass) of at most 64 x 120 bytes of records: position and radius
//                  are all an untouched node costs.
//  k_prop_fold     one workgroup per prop: the tile records, 256 tiles at a time through LDS, added in ascending tile index by six
//                  lanes (a tile outside a prop's set adds 0; 256 tiles without one are passed over); a seventh adds the hit counts.
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written in prop_rule.h.
#include "prop_kernels.h"

#include "node_edit_device.h"

namespace pies {
namespace {

static_assert(sizeof(pies_prop_t) == 120, "pies_prop_t is 30 words without padding");

__global__ void __launch_bounds__(kPropTile) k_prop_collide(PropPass P) {
  __shared__ pies_prop_t props[PIES_PROP_MAX];
  __shared__ PropTileLds lds;  // second pass
  stage_records(props, P.props, P.nProps);
  __syncthreads();
  collide_pass(
      P, props, lds, [](const pies_prop_t& r, V3 p, float rad, V3& n, V3& q) { return prop_contact(r, p, rad, n, q); },
      [](const pies_prop_t& r) -> const pies_prop_t& { return r; });
}

__global__ void __launch_bounds__(kPropTile) k_prop_fold(const uint64_t* __restrict__ tileMask, const float* __restrict__ tileSums,
                                                         uint32_t nTiles, uint32_t nProps, float* __restrict__ out) {
  __shared__ uint32_t chunk[7][kPropTile];  // bits: six floats and the hit count of 256 tiles
  const uint32_t tid = threadIdx.x, k = blockIdx.x;
  float sum = 0.0f;
  uint32_t hits = 0;
  for (uint32_t base = 0; base < nTiles; base += kPropTile) {
    const uint32_t t = base + tid;
    const bool has = t < nTiles && ((tileMask[t] >> k) & 1ull);
    if (!__syncthreads_or(has)) continue;  // (uniform) 256 tiles the prop did not touch: they would add 0
    const uint32_t* record = reinterpret_cast<const uint32_t*>(tileSums) + (static_cast<size_t>(t) * nProps + k) * kPropSumWords;
#pragma unroll
    for (uint32_t c = 0; c < 7; ++c) chunk[c][tid] = has ? record[c] : 0u;  // (a tile outside the set: +0.0f and no hits)
    __syncthreads();
    const uint32_t count = min(kPropTile, nTiles - base);
    if (tid < 6)
#pragma unroll 8
      for (uint32_t j = 0; j < count; ++j) sum = sum + __uint_as_float(chunk[tid][j]);  // (the reads do not wait for the sum)
    else if (tid == 6)
      for (uint32_t j = 0; j < count; ++j) hits += chunk[6][j];
    __syncthreads();  // the chunk is free for the next 256 tiles
  }
  if (tid < 6) out[k * kPropSumWords + tid] = sum;
  else if (tid == 6) reinterpret_cast<uint32_t*>(out)[k * kPropSumWords + 6] = hits;
}

}  // namespace

void launch_prop_collide(hipStream_t st, const PropPass& P) {
  if (!P.nd.n || !P.nProps || P.nProps > PIES_PROP_MAX) return;
  hipLaunchKernelGGL(k_prop_collide, dim3(prop_tiles(P.nd.n)), dim3(kPropTile), 0, st, P);
}

void launch_prop_fold(hipStream_t st, const PropPass& P, float* out) {
  if (!P.nd.n) return;
  launch_prop_fold_tiles(st, P.tileMask, P.tileSums, prop_tiles(P.nd.n), P.nProps, out);
}

void launch_prop_fold_tiles(hipStream_t st, const uint64_t* tileMask, const float* tileSums, uint32_t nTiles, uint32_t nRecords, float* out) {
  if (!nTiles || !nRecords || nRecords > PIES_PROP_MAX || !tileMask) return;
  hipLaunchKernelGGL(k_prop_fold, dim3(nRecords), dim3(kPropTile), 0, st, tileMask, tileSums, nTiles, nRecords, out);
}

}  // namespace pies
