// Actuators (actuator_kernels.h; the rule is stated in pies_hip.h, lives in actuator_rule.h and is restated in numpy by
// tests/test_actuators.py).
//  k_actuator_drive  one lane per actuator in the set's own order: the record (32 bytes, consecutive), the channel's activation, the
//                    constraint's id record at the record's slot (8 or 16 bytes) and its two or four positions gathered from HBM;
//                    r and the value through actuator_rule.h; a live lane stores r in the .x of its constraint's rest record - no
//                    two lanes of a set share a slot - and every lane writes its entry of outActuator.  With tileRecords the
//                    tile's (value, r, channel | live bit) go to LDS and one lane per (channel, word) walks the 256 entries in
//                    ascending index - every lane of a wave reads the same entry, a broadcast - adding another channel's or a
//                    non-live actuator's entry as 0, which changes no bit of a sum that started at +0.
//  k_actuator_fold   one workgroup per channel: the tile records, 256 tiles at a time through LDS, added in ascending tile index
//                    by one lane per word.
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written in actuator_rule.h.
#include "actuator_kernels.h"

#include "actuator_rule.h"

namespace pies {
namespace {

constexpr uint32_t kLiveBit = 0x80000000u;  // of an entry's channel word: the actuator was live
constexpr uint32_t kNoEntry = 0xFFFFFFFFu;  // ... of a lane beyond the set

__global__ void __launch_bounds__(kActuatorTile) k_actuator_drive(ActuatorPass P) {
  __shared__ float stage[2][kActuatorTile];    // value, rest
  __shared__ uint32_t word[kActuatorTile];     // channel | live bit
  const uint32_t tid = threadIdx.x, tile = blockIdx.x, a = tile * kActuatorTile + tid;
  float value = 0.0f, rest = 0.0f;
  uint32_t entry = kNoEntry;
  if (a < P.nActuators) {
    const ActuatorRecord R = P.records[a];
    const float u = P.activation[R.channel];
    const bool live = actuator_live(u);
    float* word0 = nullptr;  // the constraint's rest word
    if (R.type == PIES_DISTANCE) {
      const uint2 id = P.dcIds[R.slot];
      const float4 pa = P.pos[id.x], pb = P.pos[id.y];
      const float xa[3] = {pa.x, pa.y, pa.z}, xb[3] = {pb.x, pb.y, pb.z};
      value = actuator_length(xa, xb);
      word0 = &P.dcRw[R.slot].x;
    } else {
      const uint4 id = P.bcIds[R.slot];
      const float4 q1 = P.pos[id.x], q2 = P.pos[id.y], q3 = P.pos[id.z], q4 = P.pos[id.w];
      const float x1[3] = {q1.x, q1.y, q1.z}, x2[3] = {q2.x, q2.y, q2.z}, x3[3] = {q3.x, q3.y, q3.z}, x4[3] = {q4.x, q4.y, q4.z};
      value = actuator_cosine(x1, x2, x3, x4);
      word0 = &P.bcAw[R.slot].x;
    }
    if (live) {
      rest = actuator_rest(R.base, R.gain, R.lo, R.hi, R.flags, u);
      *word0 = rest;
    } else {
      rest = *word0;  // the rest the constraint keeps
    }
    if (P.outActuator) P.outActuator[a] = make_float2(rest, value);
    entry = R.channel | (live ? kLiveBit : 0u);
  }
  if (!P.tileRecords) return;  // (uniform: a kernel argument)
  stage[0][tid] = value;
  stage[1][tid] = rest;
  word[tid] = entry;
  __syncthreads();
  const uint32_t count = min(kActuatorTile, P.nActuators - tile * kActuatorTile);
  for (uint32_t item = tid; item < kActuatorTileWords * P.nChannels; item += kActuatorTile) {
    const uint32_t c = item / kActuatorTileWords, w = item % kActuatorTileWords, want = c | kLiveBit;
    uint32_t* record = P.tileRecords + (static_cast<size_t>(tile) * P.nChannels + c) * kActuatorTileWords;
    if (w < 2) {
      float sum = 0.0f;
#pragma unroll 8
      for (uint32_t j = 0; j < count; ++j) sum = sum + (word[j] == want ? stage[w][j] : 0.0f);
      record[w] = __float_as_uint(sum);
    } else {
      uint32_t live = 0;
#pragma unroll 8
      for (uint32_t j = 0; j < count; ++j) live += word[j] == want;
      record[2] = live;
    }
  }
}

__global__ void __launch_bounds__(kActuatorTile) k_actuator_fold(const uint32_t* __restrict__ tileRecords, uint32_t nTiles, uint32_t nChannels,
                                                                 float* __restrict__ outSums, uint32_t* __restrict__ outLive) {
  __shared__ uint32_t chunk[kActuatorTileWords][kActuatorTile];
  const uint32_t tid = threadIdx.x, c = blockIdx.x;
  float sum = 0.0f;
  uint32_t live = 0;
  for (uint32_t base = 0; base < nTiles; base += kActuatorTile) {
    const uint32_t t = base + tid;
    if (t < nTiles) {
      const uint32_t* record = tileRecords + (static_cast<size_t>(t) * nChannels + c) * kActuatorTileWords;
#pragma unroll
      for (uint32_t w = 0; w < kActuatorTileWords; ++w) chunk[w][tid] = record[w];
    }
    __syncthreads();
    const uint32_t count = min(kActuatorTile, nTiles - base);
    if (tid < 2)
#pragma unroll 8
      for (uint32_t j = 0; j < count; ++j) sum = sum + __uint_as_float(chunk[tid][j]);
    else if (tid == 2)
      for (uint32_t j = 0; j < count; ++j) live += chunk[2][j];
    __syncthreads();  // the chunk is free for the next 256 tiles
  }
  if (tid < 2 && outSums) outSums[2 * c + tid] = sum;
  else if (tid == 2 && outLive) outLive[c] = live;
}

}  // namespace

void launch_actuator_drive(hipStream_t st, const ActuatorPass& P) {
  if (!P.nActuators || !P.nChannels || P.nChannels > PIES_ACTUATOR_CHANNEL_MAX || !P.records || !P.activation || !P.pos) return;
  hipLaunchKernelGGL(k_actuator_drive, dim3(actuator_tiles(P.nActuators)), dim3(kActuatorTile), 0, st, P);
}

void launch_actuator_fold(hipStream_t st, const uint32_t* tileRecords, uint32_t nTiles, uint32_t nChannels, float* outSums, uint32_t* outLive) {
  if (!nTiles || !nChannels || nChannels > PIES_ACTUATOR_CHANNEL_MAX || !tileRecords || (!outSums && !outLive)) return;
  hipLaunchKernelGGL(k_actuator_fold, dim3(nChannels), dim3(kActuatorTile), 0, st, tileRecords, nTiles, nChannels, outSums, outLive);
}

}  // namespace pies
