// Closest points on, and winding numbers of, a triangle list whose corners live in HBM (pies_closest_points, an extension): the
// device side.  The rule for one (point, triangle) pair is stated in pies_hip.h; a point's answer is the minimum of the 64-bit key
// float_as_uint(dd) << 32 | triangle over its pairs (dd a sum of squares: >= +0, so the bit patterns order like the values; equal
// dd: the lowest triangle), no candidate is kRayMissKey.  A minimum does not depend on the order it is taken in: every split of
// the triangles gives the same bits.  No atomics - a distance kernel writes one partial key per (part, point), k_near_resolve
// takes the minimum over a point's parts.  The winding number is a sum, so its order is fixed instead: per tile of kNearTile
// triangles in ascending index, then the tile sums in ascending tile index - a function of the triangle count alone.
// Targets are RayTargets, records are launch_ray_stage's (ray_kernels.h).  Launch wrappers like kernels.h: no allocation, no
// synchronisation, everything on the caller's stream.
#pragma once
#include "ray_kernels.h"

namespace pies {

constexpr uint32_t kNearBlock = kRayBlock;   // lanes per workgroup of every kernel here
constexpr uint32_t kNearTile = kRayTile;     // triangles per LDS tile of the wide variant and per winding tile (fixed: the order of the sum)
constexpr uint32_t kNearNarrowGroup = 64;    // narrow variant: points one workgroup holds against its 256 triangles
constexpr uint32_t kNearMaxPoints = 1u << 26;
constexpr uint32_t kNearMaxChunks = 1024;
constexpr uint32_t kNearMaxTileRows = 32768;  // winding: tiles one launch spreads over grid.y (more tiles: a lane walks several)

struct NearBatch {  // points [0, n): 3 floats each
  const float* points = nullptr;
  uint32_t n = 0;
  float maxDistance2 = 0.0f;  // max_distance * max_distance, rounded once on the host
};

// Wide variant: one point per lane; the staged records go through LDS in tiles and are read as wave-wide broadcasts.  grid.y =
// chunks splits the tiles; partial[chunk * P.n + point] receives the chunk's key.
void launch_near_wide(hipStream_t st, const float4* records, uint32_t nTris, const NearBatch& P, uint32_t chunks, uint64_t* partial);
// Narrow variant: one lane per triangle (corners gathered directly), the point wave-uniform; wave-level minimum, one LDS slot per
// wave.  partial[block * P.n + point] for block < ray_narrow_parts(nTris).
void launch_near_narrow(hipStream_t st, const RayTarget& T, const NearBatch& P, uint64_t* partial);
// Minimum over a point's `parts` partial keys, the winning pair evaluated again (the same bits), the outputs (each may be nullptr):
// triangle (PIES_NEAR_NONE), distance (+inf), uv (0, 0), point (p itself).
void launch_near_resolve(hipStream_t st, const RayTarget& T, const NearBatch& P, const uint64_t* partial, uint32_t parts,
                         uint32_t* outTriangle, float* outDistance, float* outUv, float* outPoint);
// Winding numbers.  First tileSums[tile * P.n + point] = the solid angles of the tile's triangles summed in ascending index, one
// point per lane, one tile per (workgroup, grid.y step); then winding[point] = (tile sums in ascending tile index) / 4 pi.
inline uint32_t near_tiles(uint32_t nTris) { return (nTris + kNearTile - 1) / kNearTile; }
void launch_near_winding(hipStream_t st, const RayTarget& T, const NearBatch& P, float* tileSums, float* winding);

}  // namespace pies
