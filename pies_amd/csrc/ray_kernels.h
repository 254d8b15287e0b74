// Ray casts against a triangle list whose corners live in HBM (pies_raycast, an extension): the device side.  The rule for one
// (ray, triangle) pair is stated in pies_hip.h; a ray's hit is the minimum of the 64-bit key float_as_uint(t) << 32 | triangle
// over its pairs (t >= +0, so the bit patterns order like the values; equal t: the lowest triangle), a miss is kRayMissKey.  A
// minimum does not depend on the order it is taken in: every split of the triangles gives the same bits.  No atomics - a cast
// kernel writes one partial key per (part, ray), k_ray_resolve takes the minimum over a ray's parts.
// Launch wrappers like kernels.h: no allocation, no synchronisation, everything on the caller's stream.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pies {

constexpr uint32_t kRayBlock = 256;        // lanes per workgroup of every kernel here
constexpr uint32_t kRayTile = 256;         // wide variant: triangle records per LDS tile (3 float4 = 48 B each: 12 KB)
constexpr uint32_t kRayNarrowGroup = 64;   // narrow variant: rays one workgroup casts against its 256 triangles
constexpr uint32_t kRayMaxRays = 1u << 26;
constexpr uint32_t kRayMaxChunks = 1024;
constexpr uint64_t kRayMissKey = ~0ull;

// The triangles of a target: corner c of triangle t is the three floats at pos + stride * tri[3 t + c] (stride 4: the node
// positions, ids in DEVICE numbering; stride 3: a skin's packed vertices).
struct RayTarget {
  const float* pos = nullptr;
  uint32_t stride = 0;
  const uint32_t* tri = nullptr;
  uint32_t nTris = 0;
};
struct RayBatch {  // rays [0, n): origins and directions 3 floats each
  const float* origins = nullptr;
  const float* directions = nullptr;
  uint32_t n = 0;
  float tMax = 0.0f;
  uint32_t flags = 0;  // PIES_RAY_CULL_BACK
};

// Wide variant.  Staging: one lane per triangle gathers the corners once and stores the record (a, e1, e2) as 3 float4; the three
// words left over hold e1.e1, e1.e2, e2.e2 for pies_closest_points (near_kernels.h), which stages with this kernel too.
void launch_ray_stage(hipStream_t st, const RayTarget& T, float4* records);
// One ray per lane; the records go through LDS in tiles and are read as wave-wide broadcasts.  grid.y = chunks splits the
// tiles; partial[chunk * R.n + ray] receives the chunk's key.
void launch_ray_cast_wide(hipStream_t st, const float4* records, uint32_t nTris, const RayBatch& R, uint32_t chunks, uint64_t* partial);
// Narrow variant: one lane per triangle (corners gathered directly), the ray wave-uniform; wave-level minimum, then LDS across
// the workgroup.  partial[block * R.n + ray] for block < ray_narrow_parts(nTris).
inline uint32_t ray_narrow_parts(uint32_t nTris) { return (nTris + kRayBlock - 1) / kRayBlock; }
void launch_ray_cast_narrow(hipStream_t st, const RayTarget& T, const RayBatch& R, uint64_t* partial);
// Minimum over a ray's `parts` partial keys, the winning pair evaluated again for u and v (the same bits), the three outputs
// (each may be nullptr): triangle (PIES_RAY_MISS), t (+inf), uv (0, 0).
void launch_ray_resolve(hipStream_t st, const RayTarget& T, const RayBatch& R, const uint64_t* partial, uint32_t parts,
                        uint32_t* hitTriangle, float* hitT, float* hitUv);

}  // namespace pies
