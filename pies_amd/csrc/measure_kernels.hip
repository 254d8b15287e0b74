// Strain, volume and momentum measures (measure_kernels.h; the rules are stated in pies_hip.h and restated in numpy by
// tests/test_measure.py).  Read-only kernels: none of them stores to a node array.
//  k_measure_elements       one lane per element index of the container, one workgroup per tile of kMeasureTile indices that the
//                           range meets (xcd_block: neighbouring elements' nodes meet in one L2).  16-byte loads of the staged ids
//                           and of the three rest words, four float4 gathers, F = P Qinv (mat3_mul_cm) and svd3 exactly as
//                           tet_core hands them over; the record leaves as two 16-byte stores.  A lane outside the range works on
//                           the range's first element and stores nothing: no lane leaves before the barriers, and svd3's
//                           wave-uniform branches see whole wavefronts.  With a summary: the five values go through LDS and one
//                           lane per word walks the tile's counting elements in ascending index (the ballots of the four
//                           waves); the counts are population counts of ballots.
//  k_measure_elements_fold  one workgroup: the tile records in ascending tile index, kMeasureTile tiles at a time through LDS; the
//                           tiles that hold an element that counts from the waves' ballots.
//  k_measure_nodes          k_prop_collide's shape: one lane per HOST node id, one workgroup per tile of kPropTile ids, the
//                           ranges staged in LDS once.  Per range that meets the tile (a uniform test) the lanes of the range with
//                           w != 0 put their eleven terms into LDS and eleven lanes add one word each in ascending node id.
//  k_measure_nodes_fold     one workgroup per range: the records of the range's tiles in ascending tile index.
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written here.
#include "measure_kernels.h"

#include "dev_math.h"

namespace pies {
namespace {

constexpr uint32_t kWaves = kMeasureTile / 64;
static_assert(kMeasureTile == kPropTile, "both reductions use workgroups of 256 lanes");

// The held value of a walk: a sum from 0.0f, or the first value met, replaced iff the next one is smaller (larger).  A maximum is
// walked as the minimum of the negated values (x > held iff -x < -held, NaNs and signed zeros included: negation is exact), so one
// loop of selects serves the six lanes of a summary whatever their words are.
enum WalkMode : uint32_t { kWalkSum = 0, kWalkMin = 1, kWalkMax = 2 };
struct Walk {
  float held = 0.0f;
  bool have = false;
  PIES_DEV void take(uint32_t mode, float x) {
    const float y = mode == kWalkMax ? -x : x;
    const bool replace = !have || y < held;
    held = mode == kWalkSum ? held + x : (replace ? y : held);
    have = true;
  }
  PIES_DEV float result(uint32_t mode) const { return mode == kWalkMax ? -held : held; }
};
// take(x) for the lanes of `mask` in ascending lane, x = column[lane] (16-byte aligned).  Sixteen values are in registers before
// the first take of a block and the next block's reads are issued beside it: the chain of takes does not wait for LDS.
template <class Take> PIES_DEV void walk_wave(const float* column, uint64_t mask, Take&& take) {
  if (!mask) return;
#pragma unroll 2
  for (uint32_t k = 0; k < 64; k += 16) {
    const float4* q = reinterpret_cast<const float4*>(column + k);
    const float4 a = q[0], b = q[1], c = q[2], d = q[3];
    const float x[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
    const uint32_t m = static_cast<uint32_t>(mask >> k) & 0xFFFFu;
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i)
      if ((m >> i) & 1u) take(x[i]);
  }
}
// the summary's float words: which staged value a word walks, and how (volume, max stretch, min stretch, min j, max j, max green)
PIES_DEV uint32_t summary_source(uint32_t word) { return word == 0 ? 0u : word == 1 ? 1u : word == 2 ? 2u : word <= 4 ? 3u : 4u; }
PIES_DEV uint32_t summary_mode(uint32_t word) { return word == 0 ? kWalkSum : (word == 2 || word == 3) ? kWalkMin : kWalkMax; }

struct ElementTileLds {
  __attribute__((aligned(16))) float stage[5][kMeasureTile];  // volume, s[0], |s[2]|, j, green
  uint64_t ballot[5][kWaves];    // the lanes that count; inverted, over, under, nonfinite
};

__global__ void __launch_bounds__(kMeasureTile) k_measure_elements(ElementPass E) {
  __shared__ ElementTileLds lds;
  const uint32_t tid = threadIdx.x, wave = tid >> 6;
  const uint32_t tile = xcd_block(blockIdx.x, gridDim.x);  // of the range's tiles
  const uint32_t e = (E.first / kMeasureTile + tile) * kMeasureTile + tid;
  const bool live = e >= E.first && e - E.first < E.n;
  const uint32_t ec = live ? e : E.first;  // (always inside the container)
  const uint4 id = E.ids[ec];
  const float4 a0 = E.q0[ec], a1 = E.q1[ec], a2 = E.q2[ec];
  const float4 x1 = E.pos[id.x], x2 = E.pos[id.y], x3 = E.pos[id.z], x4 = E.pos[id.w];
  const float qi[3][3] = {{a0.x, a0.y, a0.z}, {a0.w, a1.x, a1.y}, {a1.z, a1.w, a2.x}};  // [col][row], tet_core's
  const float lo = a2.y, hi = a2.z;
  const float P[3][3] = {{x2.x - x1.x, x2.y - x1.y, x2.z - x1.z},
                         {x3.x - x1.x, x3.y - x1.y, x3.z - x1.z},
                         {x4.x - x1.x, x4.y - x1.y, x4.z - x1.z}};
  float F[3][3];
  mat3_mul_cm(P, qi, F);
  const float j = det3_cm(F);
  const float volume = det3_cm(P) / 6.0f;
  float i1 = F[0][0] * F[0][0];
  bool finite = true;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      if (c || r) i1 = i1 + F[c][r] * F[c][r];
      finite = finite && fabsf(F[c][r]) < INFINITY;
    }
  Svd3 d;
  svd3(F, d);
  float s0 = d.s[0], s1 = d.s[1], s2 = d.s[2];
  if (s0 < s1) { const float t = s0; s0 = s1; s1 = t; }
  if (s1 < s2) { const float t = s1; s1 = s2; s2 = t; }
  if (s0 < s1) { const float t = s0; s0 = s1; s1 = t; }
  const bool inverted = j < 0.0f;
  bool over, under;
  if (E.volume) {
    const float prod = (s0 * s1) * s2;
    over = prod > hi;
    under = prod < lo;
  } else {
    over = s0 > hi;
    under = s2 < lo;  // (s2 is still unsigned: fabsf of the signed one)
  }
  const float low = s2;
  if (inverted) s2 = -s2;
  const float g0 = s0 * s0 - 1.0f, g1 = s1 * s1 - 1.0f, g2 = s2 * s2 - 1.0f;
  const float green = 0.5f * sqrtf((g0 * g0 + g1 * g1) + g2 * g2);
  const uint32_t flags = finite ? (inverted ? PIES_ELEMENT_INVERTED : 0u) | (over ? PIES_ELEMENT_OVER : 0u) | (under ? PIES_ELEMENT_UNDER : 0u)
                                : static_cast<uint32_t>(PIES_ELEMENT_NONFINITE);
  if (E.out && live) {
    float4* record = reinterpret_cast<float4*>(E.out + (e - E.first));
    record[0] = make_float4(s0, s1, s2, j);
    record[1] = make_float4(volume, i1, green, __uint_as_float(flags));
  }
  if (!E.tileRecords) return;  // (uniform: a kernel argument)

  // ---- the tile's record of the summary ----
  const bool counts = live && finite;
  lds.stage[0][tid] = volume, lds.stage[1][tid] = s0, lds.stage[2][tid] = low, lds.stage[3][tid] = j, lds.stage[4][tid] = green;
  const uint64_t b0 = __builtin_amdgcn_ballot_w64(counts), b1 = __builtin_amdgcn_ballot_w64(counts && inverted);
  const uint64_t b2 = __builtin_amdgcn_ballot_w64(counts && over), b3 = __builtin_amdgcn_ballot_w64(counts && under);
  const uint64_t b4 = __builtin_amdgcn_ballot_w64(live && !finite);
  if ((tid & 63u) == 0) lds.ballot[0][wave] = b0, lds.ballot[1][wave] = b1, lds.ballot[2][wave] = b2, lds.ballot[3][wave] = b3, lds.ballot[4][wave] = b4;
  __syncthreads();
  uint32_t* record = E.tileRecords + static_cast<size_t>(tile) * kMeasureTileWords;
  if (tid < 6) {
    const uint32_t source = summary_source(tid), mode = summary_mode(tid);
    Walk walk;
    for (uint32_t w = 0; w < kWaves; ++w) walk_wave(&lds.stage[source][w * 64], lds.ballot[0][w], [&](float x) { walk.take(mode, x); });
    record[tid] = __float_as_uint(walk.result(mode));
  } else if (tid < 11) {  // words 6-9: inverted, over, under, nonfinite; word 10: the elements that count
    const uint32_t which = tid == 10 ? 0u : tid - 5;
    uint32_t count = 0;
    for (uint32_t w = 0; w < kWaves; ++w) count += __builtin_popcountll(lds.ballot[which][w]);
    record[tid] = count;
  } else if (tid == 11) {
    record[11] = 0u;
  }
}

__global__ void __launch_bounds__(kMeasureTile) k_measure_elements_fold(const uint32_t* __restrict__ tileRecords, uint32_t nTiles,
                                                                        uint32_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t chunk[kMeasureTileWords][kMeasureTile];  // the records of 256 tiles, word by word
  __shared__ uint64_t counts[kWaves];  // per wave of tiles: those that hold an element that counts
  const uint32_t tid = threadIdx.x;
  const uint32_t mode = summary_mode(tid);
  Walk walk;
  uint32_t count = 0;
  for (uint32_t base = 0; base < nTiles; base += kMeasureTile) {
    const uint32_t t = base + tid;
    bool counted = false;
    if (t < nTiles) {
      const uint4* record = reinterpret_cast<const uint4*>(tileRecords + static_cast<size_t>(t) * kMeasureTileWords);
      const uint4 r0 = record[0], r1 = record[1], r2 = record[2];
      chunk[0][tid] = r0.x, chunk[1][tid] = r0.y, chunk[2][tid] = r0.z, chunk[3][tid] = r0.w;
      chunk[4][tid] = r1.x, chunk[5][tid] = r1.y, chunk[6][tid] = r1.z, chunk[7][tid] = r1.w;
      chunk[8][tid] = r2.x, chunk[9][tid] = r2.y, chunk[10][tid] = r2.z, chunk[11][tid] = r2.w;
      counted = r2.z != 0u;  // (a tile without an element that counts holds +0.0f and no extremes)
    } else {
      chunk[6][tid] = chunk[7][tid] = chunk[8][tid] = chunk[9][tid] = chunk[10][tid] = 0u;  // (past the last tile: nothing to count)
    }
    const uint64_t ballot = __builtin_amdgcn_ballot_w64(counted);
    if ((tid & 63u) == 0) counts[tid >> 6] = ballot;
    __syncthreads();
    if (tid < 6) {
      for (uint32_t w = 0; w < kWaves; ++w)
        walk_wave(reinterpret_cast<const float*>(&chunk[tid][w * 64]), counts[w], [&](float x) { walk.take(mode, x); });
    } else if (tid < 11) {
#pragma unroll 8
      for (uint32_t k = 0; k < kMeasureTile; ++k) count += chunk[tid][k];  // (the reads do not wait for the sum)
    }
    __syncthreads();  // the chunk is free for the next 256 tiles
  }
  if (tid < 6) out[tid] = __float_as_uint(walk.result(mode));
  else if (tid < 11) out[tid] = count;
  else if (tid == 11) out[11] = 0u;
}

struct NodeTileLds {
  MeasureRange ranges[PIES_MEASURE_RANGE_MAX];
  __attribute__((aligned(16))) float stage[11][kPropTile];
  uint64_t ballot[2][kWaves];  // the range's lanes with w != 0, with w == 0
};

__global__ void __launch_bounds__(kPropTile) k_measure_nodes(NodeSumPass P) {
  __shared__ NodeTileLds lds;
  const uint32_t tid = threadIdx.x, wave = tid >> 6, tile = blockIdx.x;
  const uint32_t h = tile * kPropTile + tid;  // host id
  stage_records(lds.ranges, P.ranges, P.nRanges);
  __syncthreads();
  const bool live = h < P.nd.n;  // (no early return: every lane meets the barriers)
  float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v = p;
  if (live) {
    const uint32_t i = P.inv ? P.inv[h] : h;
    p = P.nd.pos[i];
    v = P.nd.vel[i];
  }
  const float w = p.w;
  const bool fixed = w == 0.0f;
  const float m = 1.0f / w;
  const float vmx = v.x * m, vmy = v.y * m, vmz = v.z * m;
  const float kinetic = 0.5f * (m * (v.x * v.x + v.y * v.y + v.z * v.z));
  const uint32_t tileFirst = tile * kPropTile;
  for (uint32_t r = 0; r < P.nRanges; ++r) {
    const MeasureRange& R = lds.ranges[r];
    // (uniform) a range without a node in this tile writes no record here: the fold reads the range's own tiles only
    if (R.count == 0 || R.first + (R.count - 1) < tileFirst || (R.first > tileFirst && R.first - tileFirst >= kPropTile)) continue;
    const bool in = live && h >= R.first && h - R.first < R.count;
    const bool dynamic = in && !fixed;
    if (dynamic) {
      const float dx = p.x - R.about[0], dy = p.y - R.about[1], dz = p.z - R.about[2];
      lds.stage[0][tid] = m;
      lds.stage[1][tid] = vmx, lds.stage[2][tid] = vmy, lds.stage[3][tid] = vmz;
      lds.stage[4][tid] = dy * vmz - dz * vmy, lds.stage[5][tid] = dz * vmx - dx * vmz, lds.stage[6][tid] = dx * vmy - dy * vmx;
      lds.stage[7][tid] = p.x * m, lds.stage[8][tid] = p.y * m, lds.stage[9][tid] = p.z * m;
      lds.stage[10][tid] = kinetic;
    }
    const uint64_t bd = __builtin_amdgcn_ballot_w64(dynamic), bf = __builtin_amdgcn_ballot_w64(in && fixed);
    if ((tid & 63u) == 0) lds.ballot[0][wave] = bd, lds.ballot[1][wave] = bf;
    __syncthreads();
    float* record = P.tileSums + (static_cast<size_t>(tile) * P.nRanges + r) * kNodeSumWords;
    if (tid < 11) {
      float sum = 0.0f;
      for (uint32_t k = 0; k < kWaves; ++k) walk_wave(&lds.stage[tid][k * 64], lds.ballot[0][k], [&](float x) { sum = sum + x; });
      record[tid] = sum;
    } else if (tid < 13) {
      uint32_t count = 0;
      for (uint32_t k = 0; k < kWaves; ++k) count += __builtin_popcountll(lds.ballot[tid - 11][k]);
      reinterpret_cast<uint32_t*>(record)[tid] = count;
    }
    __syncthreads();  // the stage and the ballots are free for the next range
  }
}

__global__ void __launch_bounds__(kPropTile) k_measure_nodes_fold(const MeasureRange* __restrict__ ranges, const float* __restrict__ tileSums,
                                                                  uint32_t nRanges, float* __restrict__ out) {
  __shared__ uint32_t chunk[13][kPropTile];  // bits: the eleven floats and the two counts of 256 tiles
  const uint32_t tid = threadIdx.x, r = blockIdx.x;
  const uint32_t first = ranges[r].first, n = ranges[r].count;
  float sum = 0.0f;
  uint32_t count = 0;
  if (n) {  // (uniform)
    const uint32_t t0 = first / kPropTile, nTiles = (first + (n - 1)) / kPropTile - t0 + 1;
    for (uint32_t base = 0; base < nTiles; base += kPropTile) {
      const uint32_t t = base + tid;
      if (t < nTiles) {
        const uint32_t* record = reinterpret_cast<const uint32_t*>(tileSums) + (static_cast<size_t>(t0 + t) * nRanges + r) * kNodeSumWords;
#pragma unroll
        for (uint32_t c = 0; c < 13; ++c) chunk[c][tid] = record[c];
      }
      __syncthreads();
      const uint32_t have = min(kPropTile, nTiles - base);
      if (tid < 11)
#pragma unroll 8
        for (uint32_t k = 0; k < have; ++k) sum = sum + __uint_as_float(chunk[tid][k]);  // (the reads do not wait for the sum)
      else if (tid < 13)
        for (uint32_t k = 0; k < have; ++k) count += chunk[tid][k];
      __syncthreads();  // the chunk is free for the next 256 tiles
    }
  }
  if (tid < 11) out[r * kNodeSumWords + tid] = sum;
  else if (tid < 13) reinterpret_cast<uint32_t*>(out)[r * kNodeSumWords + tid] = count;
  else if (tid < kNodeSumWords) out[r * kNodeSumWords + tid] = 0.0f;
}

}  // namespace

void launch_measure_elements(hipStream_t st, const ElementPass& E) {
  if (!E.n || (!E.out && !E.tileRecords)) return;
  hipLaunchKernelGGL(k_measure_elements, dim3(measure_tiles(E.first, E.n)), dim3(kMeasureTile), 0, st, E);
}

void launch_measure_elements_fold(hipStream_t st, const ElementPass& E, uint32_t* out) {
  if (!E.n || !E.tileRecords) return;
  hipLaunchKernelGGL(k_measure_elements_fold, dim3(1), dim3(kMeasureTile), 0, st, E.tileRecords, measure_tiles(E.first, E.n), out);
}

void launch_measure_nodes(hipStream_t st, const NodeSumPass& P) {
  if (!P.nd.n || !P.nRanges || P.nRanges > PIES_MEASURE_RANGE_MAX) return;
  hipLaunchKernelGGL(k_measure_nodes, dim3(prop_tiles(P.nd.n)), dim3(kPropTile), 0, st, P);
}

void launch_measure_nodes_fold(hipStream_t st, const NodeSumPass& P, float* out) {
  if (!P.nRanges || P.nRanges > PIES_MEASURE_RANGE_MAX) return;
  hipLaunchKernelGGL(k_measure_nodes_fold, dim3(P.nRanges), dim3(kPropTile), 0, st, P.ranges, P.tileSums, P.nRanges, out);
}

}  // namespace pies
