// Generalised winding number of a triangle mesh at the cell centres of a lattice (pies_voxelize_tri_mesh, the cell classifier of
// pies_add_tri_mesh_volume): the device side.  A launch wrapper like skin_kernels.h: no allocation, no synchronisation, on the
// caller's stream.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pies {

constexpr uint32_t kVoxelBlock = 256;        // lanes = samples per workgroup
constexpr uint32_t kVoxelTile = 256;         // triangles staged in LDS at a time, nine floats each (9 KB)
constexpr uint32_t kVoxelMaxSamples = 1u << 26;
constexpr uint32_t kVoxelMaxTriangles = 1u << 24;

struct VoxelLattice {
  float origin[3];
  float cell;
  uint32_t dims[3];  // (nx, ny, nz); sample (i, j, k) has index (i * ny + j) * nz + k and lies at origin + ((i, j, k) + 0.5) * cell
};

// winding[s] = w(sample s) by the rule of pies_hip.h, inside[s] = |w| > 0.5, for the nx * ny * nz (<= kVoxelMaxSamples) samples.
// positions: nVertices x 3, tri: nTriangles x 3 indices that the caller has checked against nVertices.
void launch_winding(hipStream_t st, const float* positions, const uint32_t* tri, uint32_t nTriangles, const VoxelLattice& L,
                    float* winding, uint8_t* inside);

}  // namespace pies
