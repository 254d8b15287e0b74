// Closest points and winding numbers against the deforming surface (near_kernels.h; the pair rule is stated in pies_hip.h and
// restated in numpy by tests/test_nearest.py).  Brute force: every point meets every triangle.
//  k_near_wide     one point per lane.  A workgroup copies the staged records (k_ray_stage: a, e1, e2 and the triangle's own three
//                  dot products, 48 bytes) of a tile into LDS with coalesced 16-byte loads and every lane walks the tile; all
//                  lanes of a wavefront read the same LDS address at the same time (a broadcast: no bank conflicts), three
//                  ds_read_b128 per pair.  The region walk is one chain that picks a numerator and a denominator, so a pair
//                  costs one division whatever its region; the compiler turns the chain into exec-mask branches, which
//                  neighbouring points mostly take alike (DESIGN.md 8d counts the instructions).  12 KB of LDS: the 8 waves
//                  per SIMD are the limit, as for k_ray_cast.
//  k_near_narrow   one lane per triangle, corners gathered directly, the dot products computed by the same expressions as the
//                  staging kernel's; the workgroup's points (up to 64) are wave-uniform.  Per point a wave-level minimum of the
//                  key, one LDS slot per wave, and after one barrier lane k takes the minimum over the four waves for point k.
//  k_near_resolve  one lane per point: its partial keys, the winning pair once more for (u, v), q and dd.
//  k_near_winding_tiles / _sum   the winding number in its fixed two-level order: a workgroup stages one tile's corners (nine
//                  floats per triangle, as k_winding does), every lane sums the tile for its point in ascending index and
//                  stores the tile sum; the second kernel adds a point's tile sums in ascending tile index.  The dependent
//                  chain of a lane is 256 pairs however many triangles there are; a single probe spreads over the tiles.
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written here.
#include "near_kernels.h"

#include <cfloat>

#include "../../include/pies_hip.h"
#include "surface_device.h"

namespace pies {
namespace {

// The rule for one (point, triangle) pair: point p, triangle corner a, edges e1 = b - a, e2 = c - a and their dot products.
// Ericson's region walk; every test in the positive form, so a NaN anywhere ends in the last branch and in a NaN dd, which is
// no candidate.
__device__ __forceinline__ bool near_pair(V3 p, V3 a, V3 e1, V3 e2, float e11, float e12, float e22, float maxDistance2, float& dd,
                                          float& u, float& v, V3& q) {
  const V3 ap = sub(p, a);
  const float d1 = dot(e1, ap), d2 = dot(e2, ap);
  const float d3 = d1 - e11, d4 = d2 - e12, d5 = d1 - e12, d6 = d2 - e22;
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float d43 = d4 - d3, d56 = d5 - d6;
  int region;
  float num = 0.0f, den = 1.0f;
  if (d1 <= 0.0f && d2 <= 0.0f) region = 0;                  // corner a
  else if (d3 >= 0.0f && d4 <= d3) region = 1;               // corner b
  else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {         // edge a b
    region = 2;
    num = d1;
    den = d1 - d3;
  } else if (d6 >= 0.0f && d5 <= d6) region = 3;             // corner c
  else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {         // edge a c
    region = 4;
    num = d2;
    den = d2 - d6;
  } else if (va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f) {     // edge b c
    region = 5;
    num = d43;
    den = d43 + d56;
  } else {                                                   // the interior
    region = 6;
    num = 1.0f;
    den = (va + vb) + vc;
  }
  const float w = num / den;  // (the one division of a pair; 0 / 1 at a corner)
  u = region == 1 ? 1.0f : region == 2 ? w : region == 5 ? 1.0f - w : region == 6 ? vb * w : 0.0f;
  v = region == 3 ? 1.0f : region == 4 || region == 5 ? w : region == 6 ? vc * w : 0.0f;
  q = V3{(a.x + e1.x * u) + e2.x * v, (a.y + e1.y * u) + e2.y * v, (a.z + e1.z * u) + e2.z * v};
  const V3 r = sub(p, q);
  dd = dot(r, r);
  return dd <= FLT_MAX && dd <= maxDistance2;
}

__global__ void __launch_bounds__(kNearBlock) k_near_wide(const float4* __restrict__ records, uint32_t nTris, NearBatch P,
                                                          uint32_t tilesPerChunk, uint64_t* __restrict__ partial) {
  __shared__ float4 tile[3 * kNearTile];
  const uint32_t i = blockIdx.x * kNearBlock + threadIdx.x;
  const bool live = i < P.n;  // (no early return: every lane stages records and meets the barriers)
  V3 p{0.0f, 0.0f, 0.0f};
  if (live) p = load3(P.points + 3ull * i);
  const uint32_t nTiles = (nTris + kNearTile - 1) / kNearTile;
  const uint64_t first64 = static_cast<uint64_t>(blockIdx.y) * tilesPerChunk;
  const uint32_t first = static_cast<uint32_t>(first64 < nTiles ? first64 : nTiles);
  const uint32_t last = static_cast<uint32_t>(first64 + tilesPerChunk < nTiles ? first64 + tilesPerChunk : nTiles);
  uint64_t best = kRayMissKey;
  for (uint32_t tileIndex = first; tileIndex < last; ++tileIndex) {
    const uint32_t base = tileIndex * kNearTile;
    const uint32_t count = min(kNearTile, nTris - base);
    __syncthreads();  // the previous tile has been read by every lane
    for (uint32_t k = threadIdx.x; k < 3 * count; k += kNearBlock) tile[k] = records[3ull * base + k];
    __syncthreads();
    if (!live) continue;
    for (uint32_t k = 0; k < count; ++k) {
      const float4 r0 = tile[3 * k], r1 = tile[3 * k + 1], r2 = tile[3 * k + 2];
      float dd, u, v;
      V3 q;
      if (near_pair(p, V3{r0.x, r0.y, r0.z}, V3{r0.w, r1.x, r1.y}, V3{r1.z, r1.w, r2.x}, r2.y, r2.z, r2.w, P.maxDistance2, dd, u, v, q))
        best = min(best, surface_key(dd, base + k));
    }
  }
  if (live) partial[static_cast<size_t>(blockIdx.y) * P.n + i] = best;
}

// blockIdx.x = group * parts + block: points [group * kNearNarrowGroup, ...) against triangles [block * kNearBlock, ...)
__global__ void __launch_bounds__(kNearBlock) k_near_narrow(RayTarget T, NearBatch P, uint32_t parts, uint64_t* __restrict__ partial) {
  __shared__ uint64_t slot[kNearNarrowGroup][kNearBlock / 64];
  const uint32_t group = blockIdx.x / parts, block = blockIdx.x - group * parts;
  const uint32_t tri = block * kNearBlock + threadIdx.x;
  const bool live = tri < T.nTris;
  V3 a{0.0f, 0.0f, 0.0f}, e1 = a, e2 = a;
  if (live) gather_triangle(T, tri, a, e1, e2);
  const float e11 = dot(e1, e1), e12 = dot(e1, e2), e22 = dot(e2, e2);
  const uint32_t firstPoint = group * kNearNarrowGroup;
  const uint32_t points = min(kNearNarrowGroup, P.n - firstPoint);
  for (uint32_t k = 0; k < points; ++k) {
    const V3 p = load3(P.points + 3ull * (firstPoint + k));
    uint64_t key = kRayMissKey;
    float dd, u, v;
    V3 q;
    if (live && near_pair(p, a, e1, e2, e11, e12, e22, P.maxDistance2, dd, u, v, q)) key = surface_key(dd, tri);
    for (int offset = 32; offset > 0; offset >>= 1) key = min(key, __shfl_xor(key, offset));
    if ((threadIdx.x & 63u) == 0) slot[k][threadIdx.x >> 6] = key;
  }
  __syncthreads();
  if (threadIdx.x < points) {
    uint64_t key = slot[threadIdx.x][0];
    for (uint32_t w = 1; w < kNearBlock / 64; ++w) key = min(key, slot[threadIdx.x][w]);
    partial[static_cast<size_t>(block) * P.n + firstPoint + threadIdx.x] = key;
  }
}

__global__ void __launch_bounds__(kNearBlock) k_near_resolve(RayTarget T, NearBatch P, const uint64_t* __restrict__ partial, uint32_t parts,
                                                             uint32_t* __restrict__ outTriangle, float* __restrict__ outDistance,
                                                             float* __restrict__ outUv, float* __restrict__ outPoint) {
  const uint32_t i = blockIdx.x * kNearBlock + threadIdx.x;
  if (i >= P.n) return;
  uint64_t key = kRayMissKey;
  for (uint32_t part = 0; part < parts; ++part) key = min(key, partial[static_cast<size_t>(part) * P.n + i]);
  const V3 p = load3(P.points + 3ull * i);
  uint32_t triangle = PIES_NEAR_NONE;
  float distance = __uint_as_float(0x7F800000u), u = 0.0f, v = 0.0f;  // +inf
  V3 q = p;
  if (key != kRayMissKey && static_cast<uint32_t>(key) < T.nTris) {
    triangle = static_cast<uint32_t>(key);
    V3 a, e1, e2;
    gather_triangle(T, triangle, a, e1, e2);
    // the pair that won, once more: the same function on the same operands gives the same bits
    float dd;
    (void)near_pair(p, a, e1, e2, dot(e1, e1), dot(e1, e2), dot(e2, e2), P.maxDistance2, dd, u, v, q);
    distance = sqrtf(__uint_as_float(static_cast<uint32_t>(key >> 32)));
  }
  if (outTriangle) outTriangle[i] = triangle;
  if (outDistance) outDistance[i] = distance;
  if (outUv) {
    outUv[2ull * i] = u;
    outUv[2ull * i + 1] = v;
  }
  if (outPoint) {
    outPoint[3ull * i] = q.x;
    outPoint[3ull * i + 1] = q.y;
    outPoint[3ull * i + 2] = q.z;
  }
}

__global__ void __launch_bounds__(kNearBlock) k_near_winding_tiles(RayTarget T, NearBatch P, float* __restrict__ tileSums) {
  __shared__ float tile[9 * kNearTile];
  const uint32_t i = blockIdx.x * kNearBlock + threadIdx.x;
  const bool live = i < P.n;  // (no early return: every lane stages triangles and meets the barriers)
  V3 p{0.0f, 0.0f, 0.0f};
  if (live) p = load3(P.points + 3ull * i);
  const uint32_t nTiles = (T.nTris + kNearTile - 1) / kNearTile;
  for (uint32_t tileIndex = blockIdx.y; tileIndex < nTiles; tileIndex += gridDim.y) {
    const uint32_t base = tileIndex * kNearTile;
    const uint32_t count = min(kNearTile, T.nTris - base);
    __syncthreads();  // the previous tile has been read by every lane
    for (uint32_t t = threadIdx.x; t < count; t += kNearBlock) {
      V3 a, b, c;
      gather_corners(T, base + t, a, b, c);
      float* q = tile + 9 * t;
      q[0] = a.x, q[1] = a.y, q[2] = a.z;
      q[3] = b.x, q[4] = b.y, q[5] = b.z;
      q[6] = c.x, q[7] = c.y, q[8] = c.z;
    }
    __syncthreads();
    if (!live) continue;
    float sum = 0.0f;
    for (uint32_t t = 0; t < count; ++t) {
      const float* q = tile + 9 * t;
      sum = sum + solid_angle(q[0] - p.x, q[1] - p.y, q[2] - p.z, q[3] - p.x, q[4] - p.y, q[5] - p.z, q[6] - p.x, q[7] - p.y, q[8] - p.z);
    }
    tileSums[static_cast<size_t>(tileIndex) * P.n + i] = sum;
  }
}

__global__ void __launch_bounds__(kNearBlock) k_near_winding_sum(const float* __restrict__ tileSums, uint32_t nTiles, uint32_t n,
                                                                 float* __restrict__ winding) {
  const uint32_t i = blockIdx.x * kNearBlock + threadIdx.x;
  if (i >= n) return;
  float sum = 0.0f;
  for (uint32_t t = 0; t < nTiles; ++t) sum = sum + tileSums[static_cast<size_t>(t) * n + i];
  winding[i] = sum / 12.566370614359172f;  // 4 pi
}

}  // namespace

void launch_near_wide(hipStream_t st, const float4* records, uint32_t nTris, const NearBatch& P, uint32_t chunks, uint64_t* partial) {
  if (!P.n || !nTris || !chunks || chunks > kNearMaxChunks) return;
  const uint32_t nTiles = near_tiles(nTris);
  const uint32_t tilesPerChunk = (nTiles + chunks - 1) / chunks;
  hipLaunchKernelGGL(k_near_wide, dim3((P.n + kNearBlock - 1) / kNearBlock, chunks), dim3(kNearBlock), 0, st, records, nTris, P,
                     tilesPerChunk, partial);
}

void launch_near_narrow(hipStream_t st, const RayTarget& T, const NearBatch& P, uint64_t* partial) {
  if (!P.n || !T.nTris) return;
  const uint32_t parts = ray_narrow_parts(T.nTris);
  const uint64_t blocks = static_cast<uint64_t>((P.n + kNearNarrowGroup - 1) / kNearNarrowGroup) * parts;
  if (blocks > 0x7FFFFFFFull) return;
  hipLaunchKernelGGL(k_near_narrow, dim3(static_cast<uint32_t>(blocks)), dim3(kNearBlock), 0, st, T, P, parts, partial);
}

void launch_near_resolve(hipStream_t st, const RayTarget& T, const NearBatch& P, const uint64_t* partial, uint32_t parts,
                         uint32_t* outTriangle, float* outDistance, float* outUv, float* outPoint) {
  if (!P.n) return;
  hipLaunchKernelGGL(k_near_resolve, dim3((P.n + kNearBlock - 1) / kNearBlock), dim3(kNearBlock), 0, st, T, P, partial, parts, outTriangle,
                     outDistance, outUv, outPoint);
}

void launch_near_winding(hipStream_t st, const RayTarget& T, const NearBatch& P, float* tileSums, float* winding) {
  if (!P.n) return;
  const uint32_t nTiles = near_tiles(T.nTris), blocks = (P.n + kNearBlock - 1) / kNearBlock;
  if (nTiles)
    hipLaunchKernelGGL(k_near_winding_tiles, dim3(blocks, nTiles < kNearMaxTileRows ? nTiles : kNearMaxTileRows), dim3(kNearBlock), 0, st, T, P,
                       tileSums);
  hipLaunchKernelGGL(k_near_winding_sum, dim3(blocks), dim3(kNearBlock), 0, st, tileSums, nTiles, P.n, winding);
}

}  // namespace pies
