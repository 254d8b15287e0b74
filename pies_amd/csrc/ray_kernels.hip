// Ray casts against the deforming surface (ray_kernels.h; the pair rule is stated in pies_hip.h and restated in numpy by
// tests/test_raycast.py).  Brute force: every ray meets every triangle.  Per pair ~45 plain VALU operations and one division.
//  k_ray_stage   one lane per triangle: three gathers of a corner (12 B each, through the id list) and one 48-byte record
//                (a, e1, e2) out.  A bandwidth kernel, run once per call of the wide variant.
//  k_ray_cast    wide variant, one ray per lane.  A workgroup copies the records of a tile into LDS with coalesced 16-byte
//                loads and every lane walks the tile; all lanes of a wavefront read the same LDS address at the same time (a
//                broadcast: no bank conflicts), three ds_read_b128 per pair, so the kernel sits at its arithmetic.  The 12 KB tile
//                leaves 13 workgroups' worth of LDS per CU; the 8 waves per SIMD (8 workgroups of 4 waves per CU) are the limit.
//  k_ray_narrow  one lane per triangle, corners gathered directly and kept in registers; the workgroup's rays (up to 64) are
//                wave-uniform, their origins and directions come through the scalar cache.  Per ray a wave-level minimum of the
//                key (six shuffle steps of two words), one LDS word pair per wave, and after one barrier lane k takes the minimum
//                over the four waves for ray k.  Few rays against many triangles fill the device with triangle blocks.
//  k_ray_resolve one lane per ray: coalesced reads of its partial keys, the winning pair once more for (u, v).
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written here.
#include "ray_kernels.h"

#include <cfloat>

#include "../../include/pies_hip.h"
#include "surface_device.h"

namespace pies {
namespace {

// The rule for one (ray, triangle) pair: ray (o, d), triangle corner a and edges e1 = b - a, e2 = c - a.  Every test in the
// positive form: a NaN anywhere is a miss.
__device__ __forceinline__ bool ray_pair(V3 o, V3 d, V3 a, V3 e1, V3 e2, float tMax, bool cullBack, float& t, float& u, float& v) {
  const V3 p = cross(d, e2);
  const float det = dot(e1, p);
  if (!((cullBack ? det : fabsf(det)) >= FLT_MIN)) return false;
  const float inv = 1.0f / det;
  if (!(fabsf(inv) <= FLT_MAX)) return false;
  const V3 s = sub(o, a);
  u = dot(s, p) * inv;
  if (!(u >= 0.0f && u <= 1.0f)) return false;
  const V3 q = cross(s, e1);
  v = dot(d, q) * inv;
  if (!(v >= 0.0f && u + v <= 1.0f)) return false;
  t = dot(e2, q) * inv + 0.0f;  // (-0 becomes +0: the key below orders by bit pattern)
  return t >= 0.0f && t <= tMax;
}

__device__ __forceinline__ uint64_t ray_key(float t, uint32_t triangle) { return surface_key(t, triangle); }

// The last three words are the triangle's own dot products e1.e1, e1.e2, e2.e2: pies_closest_points reads them (near_kernels.hip),
// a ray cast does not.
__global__ void __launch_bounds__(kRayBlock) k_ray_stage(RayTarget T, float4* __restrict__ records) {
  const uint32_t t = blockIdx.x * kRayBlock + threadIdx.x;
  if (t >= T.nTris) return;
  V3 a, e1, e2;
  gather_triangle(T, t, a, e1, e2);
  float4* r = records + 3ull * t;
  r[0] = make_float4(a.x, a.y, a.z, e1.x);
  r[1] = make_float4(e1.y, e1.z, e2.x, e2.y);
  r[2] = make_float4(e2.z, dot(e1, e1), dot(e1, e2), dot(e2, e2));
}

__global__ void __launch_bounds__(kRayBlock) k_ray_cast(const float4* __restrict__ records, uint32_t nTris, RayBatch R,
                                                        uint32_t tilesPerChunk, uint64_t* __restrict__ partial) {
  __shared__ float4 tile[3 * kRayTile];
  const uint32_t r = blockIdx.x * kRayBlock + threadIdx.x;
  const bool live = r < R.n;  // (no early return: every lane stages records and meets the barriers)
  V3 o{0.0f, 0.0f, 0.0f}, d{0.0f, 0.0f, 0.0f};
  if (live) {
    o = load3(R.origins + 3ull * r);
    d = load3(R.directions + 3ull * r);
  }
  const bool cull = (R.flags & PIES_RAY_CULL_BACK) != 0;
  const uint32_t nTiles = (nTris + kRayTile - 1) / kRayTile;
  const uint64_t first64 = static_cast<uint64_t>(blockIdx.y) * tilesPerChunk;
  const uint32_t first = static_cast<uint32_t>(first64 < nTiles ? first64 : nTiles);
  const uint32_t last = static_cast<uint32_t>(first64 + tilesPerChunk < nTiles ? first64 + tilesPerChunk : nTiles);
  uint64_t best = kRayMissKey;
  for (uint32_t tileIndex = first; tileIndex < last; ++tileIndex) {
    const uint32_t base = tileIndex * kRayTile;
    const uint32_t count = min(kRayTile, nTris - base);
    __syncthreads();  // the previous tile has been read by every lane
    for (uint32_t k = threadIdx.x; k < 3 * count; k += kRayBlock) tile[k] = records[3ull * base + k];
    __syncthreads();
    if (!live) continue;
    for (uint32_t k = 0; k < count; ++k) {
      const float4 r0 = tile[3 * k], r1 = tile[3 * k + 1], r2 = tile[3 * k + 2];
      float t, u, v;
      if (ray_pair(o, d, V3{r0.x, r0.y, r0.z}, V3{r0.w, r1.x, r1.y}, V3{r1.z, r1.w, r2.x}, R.tMax, cull, t, u, v))
        best = min(best, ray_key(t, base + k));
    }
  }
  if (live) partial[static_cast<size_t>(blockIdx.y) * R.n + r] = best;
}

// blockIdx.x = group * parts + block: rays [group * kRayNarrowGroup, ...) against triangles [block * kRayBlock, ...)
__global__ void __launch_bounds__(kRayBlock) k_ray_narrow(RayTarget T, RayBatch R, uint32_t parts, uint64_t* __restrict__ partial) {
  __shared__ uint64_t slot[kRayNarrowGroup][kRayBlock / 64];
  const uint32_t group = blockIdx.x / parts, block = blockIdx.x - group * parts;
  const uint32_t tri = block * kRayBlock + threadIdx.x;
  const bool live = tri < T.nTris;
  V3 a{0.0f, 0.0f, 0.0f}, e1 = a, e2 = a;
  if (live) gather_triangle(T, tri, a, e1, e2);
  const bool cull = (R.flags & PIES_RAY_CULL_BACK) != 0;
  const uint32_t firstRay = group * kRayNarrowGroup;
  const uint32_t rays = min(kRayNarrowGroup, R.n - firstRay);
  for (uint32_t k = 0; k < rays; ++k) {
    const V3 o = load3(R.origins + 3ull * (firstRay + k)), d = load3(R.directions + 3ull * (firstRay + k));
    uint64_t key = kRayMissKey;
    float t, u, v;
    if (live && ray_pair(o, d, a, e1, e2, R.tMax, cull, t, u, v)) key = ray_key(t, tri);
    for (int offset = 32; offset > 0; offset >>= 1) key = min(key, __shfl_xor(key, offset));
    if ((threadIdx.x & 63u) == 0) slot[k][threadIdx.x >> 6] = key;
  }
  __syncthreads();
  if (threadIdx.x < rays) {
    uint64_t key = slot[threadIdx.x][0];
    for (uint32_t w = 1; w < kRayBlock / 64; ++w) key = min(key, slot[threadIdx.x][w]);
    partial[static_cast<size_t>(block) * R.n + firstRay + threadIdx.x] = key;
  }
}

__global__ void __launch_bounds__(kRayBlock) k_ray_resolve(RayTarget T, RayBatch R, const uint64_t* __restrict__ partial, uint32_t parts,
                                                           uint32_t* __restrict__ hitTriangle, float* __restrict__ hitT,
                                                           float* __restrict__ hitUv) {
  const uint32_t r = blockIdx.x * kRayBlock + threadIdx.x;
  if (r >= R.n) return;
  uint64_t key = kRayMissKey;
  for (uint32_t p = 0; p < parts; ++p) key = min(key, partial[static_cast<size_t>(p) * R.n + r]);
  uint32_t triangle = PIES_RAY_MISS;
  float t = __uint_as_float(0x7F800000u), u = 0.0f, v = 0.0f;  // +inf
  if (key != kRayMissKey && static_cast<uint32_t>(key) < T.nTris) {
    triangle = static_cast<uint32_t>(key);
    V3 a, e1, e2;
    gather_triangle(T, triangle, a, e1, e2);
    // the pair that won, once more: the same function on the same operands gives the same bits
    (void)ray_pair(load3(R.origins + 3ull * r), load3(R.directions + 3ull * r), a, e1, e2, R.tMax, (R.flags & PIES_RAY_CULL_BACK) != 0, t, u, v);
    t = __uint_as_float(static_cast<uint32_t>(key >> 32));
  }
  if (hitTriangle) hitTriangle[r] = triangle;
  if (hitT) hitT[r] = t;
  if (hitUv) {
    hitUv[2ull * r] = u;
    hitUv[2ull * r + 1] = v;
  }
}

}  // namespace

void launch_ray_stage(hipStream_t st, const RayTarget& T, float4* records) {
  if (!T.nTris) return;
  hipLaunchKernelGGL(k_ray_stage, dim3((T.nTris + kRayBlock - 1) / kRayBlock), dim3(kRayBlock), 0, st, T, records);
}

void launch_ray_cast_wide(hipStream_t st, const float4* records, uint32_t nTris, const RayBatch& R, uint32_t chunks, uint64_t* partial) {
  if (!R.n || !nTris || !chunks || chunks > kRayMaxChunks) return;
  const uint32_t nTiles = (nTris + kRayTile - 1) / kRayTile;
  const uint32_t tilesPerChunk = (nTiles + chunks - 1) / chunks;
  hipLaunchKernelGGL(k_ray_cast, dim3((R.n + kRayBlock - 1) / kRayBlock, chunks), dim3(kRayBlock), 0, st, records, nTris, R, tilesPerChunk,
                     partial);
}

void launch_ray_cast_narrow(hipStream_t st, const RayTarget& T, const RayBatch& R, uint64_t* partial) {
  if (!R.n || !T.nTris) return;
  const uint32_t parts = ray_narrow_parts(T.nTris);
  const uint64_t blocks = static_cast<uint64_t>((R.n + kRayNarrowGroup - 1) / kRayNarrowGroup) * parts;
  if (blocks > 0x7FFFFFFFull) return;
  hipLaunchKernelGGL(k_ray_narrow, dim3(static_cast<uint32_t>(blocks)), dim3(kRayBlock), 0, st, T, R, parts, partial);
}

void launch_ray_resolve(hipStream_t st, const RayTarget& T, const RayBatch& R, const uint64_t* partial, uint32_t parts,
                        uint32_t* hitTriangle, float* hitT, float* hitUv) {
  if (!R.n) return;
  hipLaunchKernelGGL(k_ray_resolve, dim3((R.n + kRayBlock - 1) / kRayBlock), dim3(kRayBlock), 0, st, T, R, partial, parts, hitTriangle, hitT,
                     hitUv);
}

}  // namespace pies
