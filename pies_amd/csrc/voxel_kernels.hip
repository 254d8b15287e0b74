// k_winding (voxel_kernels.h): points x triangles solid angles, the classifier of pies_add_tri_mesh_volume.  One lane owns one
// sample (a cell centre) and sums the solid angles of ALL triangles itself, in ascending triangle index: no atomics, no
// cross-lane combination, two runs agree bit for bit.  A workgroup of kVoxelBlock lanes stages the triangles through LDS in
// tiles of kVoxelTile triangles, nine floats each (corner a, b, d; gathered through the index list once per workgroup and
// tile), and every lane walks every tile in order.  All lanes of a wavefront read the same LDS address at the same time
// (a broadcast: no bank conflicts), so the 9 KB tile costs nothing in occupancy (17 workgroups' worth fit the 160 KB of a CU,
// the 8 waves per SIMD are the limit) and the kernel is bound by its arithmetic: per pair ~60 plain VALU operations, three
// square roots and one atan2f (a division and a polynomial).
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written here, which
// tests/test_trimesh.py restates in numpy.
#include "voxel_kernels.h"

#include "surface_device.h"

namespace pies {
namespace {

__global__ void __launch_bounds__(kVoxelBlock) k_winding(const float* __restrict__ positions, const uint32_t* __restrict__ tri,
                                                         uint32_t nTriangles, VoxelLattice L, uint32_t nSamples,
                                                         float* __restrict__ winding, uint8_t* __restrict__ inside) {
  __shared__ float tile[9 * kVoxelTile];
  const uint32_t s = blockIdx.x * kVoxelBlock + threadIdx.x;
  const bool live = s < nSamples;  // (no early return: every lane stages triangles and meets the barriers)
  const uint32_t plane = L.dims[1] * L.dims[2];
  const uint32_t i = live ? s / plane : 0u, r = live ? s - i * plane : 0u;
  const uint32_t j = r / L.dims[2], k = r - j * L.dims[2];
  const float cx = L.origin[0] + (static_cast<float>(i) + 0.5f) * L.cell;
  const float cy = L.origin[1] + (static_cast<float>(j) + 0.5f) * L.cell;
  const float cz = L.origin[2] + (static_cast<float>(k) + 0.5f) * L.cell;
  float sum = 0.0f;
  for (uint32_t base = 0; base < nTriangles; base += kVoxelTile) {
    const uint32_t count = min(kVoxelTile, nTriangles - base);
    __syncthreads();  // the previous tile has been read by every lane
    for (uint32_t t = threadIdx.x; t < count; t += kVoxelBlock) {
      const uint32_t* id = tri + 3ull * (base + t);
      for (int c = 0; c < 3; ++c) {
        const float* p = positions + 3ull * id[c];
        tile[9 * t + 3 * c] = p[0];
        tile[9 * t + 3 * c + 1] = p[1];
        tile[9 * t + 3 * c + 2] = p[2];
      }
    }
    __syncthreads();
    if (!live) continue;
    for (uint32_t t = 0; t < count; ++t) {
      const float* q = tile + 9 * t;
      const float ax = q[0] - cx, ay = q[1] - cy, az = q[2] - cz;
      const float bx = q[3] - cx, by = q[4] - cy, bz = q[5] - cz;
      const float dx = q[6] - cx, dy = q[7] - cy, dz = q[8] - cz;
      sum = sum + solid_angle(ax, ay, az, bx, by, bz, dx, dy, dz);  // (surface_device.h: shared with pies_closest_points)
    }
  }
  if (live) {
    const float w = sum / 12.566370614359172f;  // 4 pi
    winding[s] = w;
    inside[s] = fabsf(w) > 0.5f ? 1 : 0;
  }
}

}  // namespace

void launch_winding(hipStream_t st, const float* positions, const uint32_t* tri, uint32_t nTriangles, const VoxelLattice& L,
                    float* winding, uint8_t* inside) {
  const uint64_t n = static_cast<uint64_t>(L.dims[0]) * L.dims[1] * L.dims[2];
  if (n == 0 || n > kVoxelMaxSamples || nTriangles > kVoxelMaxTriangles) return;
  const uint32_t nSamples = static_cast<uint32_t>(n);
  hipLaunchKernelGGL(k_winding, dim3((nSamples + kVoxelBlock - 1) / kVoxelBlock), dim3(kVoxelBlock), 0, st, positions, tri, nTriangles, L,
                     nSamples, winding, inside);
}

}  // namespace pies
