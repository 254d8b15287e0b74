// Skinning kernels of the embedded surface meshes (skin_kernels.h).  Plain bandwidth kernels: one lane per vertex, no LDS, no
// atomics (every sum has a fixed order, so two runs agree bit for bit).  Per vertex k_skin_positions moves 32 B of record (two
// coalesced 16-byte loads), four 16-byte gathers from the node positions and one 12-byte store; k_skin_normals 8 B of row
// pointers, 4 B + 12 B per incident triangle of indices, 36 B per incident triangle of skinned positions and a 12-byte store.
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written here.
#include "skin_kernels.h"

namespace pies {
namespace {

constexpr uint32_t kSkinBlock = 256;

__global__ void __launch_bounds__(kSkinBlock) k_skin_positions(const uint4* __restrict__ ids, const float4* __restrict__ w,
                                                               const float4* __restrict__ nodePos, float* __restrict__ out,
                                                               uint32_t first, uint32_t count) {
  const uint32_t k = blockIdx.x * kSkinBlock + threadIdx.x;
  if (k >= count) return;
  const uint32_t v = first + k;
  const uint4 id = ids[v];
  const float4 wt = w[v];
  const float4 p0 = nodePos[id.x], p1 = nodePos[id.y], p2 = nodePos[id.z], p3 = nodePos[id.w];
  float x = p0.x + wt.x * (p1.x - p0.x);
  float y = p0.y + wt.x * (p1.y - p0.y);
  float z = p0.z + wt.x * (p1.z - p0.z);
  x = x + wt.y * (p2.x - p0.x);
  y = y + wt.y * (p2.y - p0.y);
  z = z + wt.y * (p2.z - p0.z);
  x = x + wt.z * (p3.x - p0.x);
  y = y + wt.z * (p3.y - p0.y);
  z = z + wt.z * (p3.z - p0.z);
  float* o = out + 3ull * v;
  o[0] = x;
  o[1] = y;
  o[2] = z;
}

__global__ void __launch_bounds__(kSkinBlock) k_skin_normals(const uint32_t* __restrict__ incPtr, const uint32_t* __restrict__ inc,
                                                             const uint32_t* __restrict__ tri, const float* __restrict__ x,
                                                             float* __restrict__ out, uint32_t first, uint32_t count) {
  const uint32_t k = blockIdx.x * kSkinBlock + threadIdx.x;
  if (k >= count) return;
  const uint32_t v = first + k;
  const uint32_t begin = incPtr[v], end = incPtr[v + 1];
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  for (uint32_t e = begin; e < end; ++e) {
    const uint32_t* t = tri + 3ull * inc[e];
    const float *a = x + 3ull * t[0], *b = x + 3ull * t[1], *c = x + 3ull * t[2];
    const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const float vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    sx = sx + (uy * vz - uz * vy);
    sy = sy + (uz * vx - ux * vz);
    sz = sz + (ux * vy - uy * vx);
  }
  const float len2 = sx * sx + sy * sy + sz * sz;
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (len2 > 0.0f && len2 <= 3.402823466e+38f) {  // (false for NaN as well)
    const float len = sqrtf(len2);
    nx = sx / len;
    ny = sy / len;
    nz = sz / len;
  }
  float* o = out + 3ull * v;
  o[0] = nx;
  o[1] = ny;
  o[2] = nz;
}

}  // namespace

void launch_skin_positions(hipStream_t st, const SkinArrays& S, const float4* nodePos, float* out, uint32_t first, uint32_t count) {
  if (!count || first + static_cast<uint64_t>(count) > S.nVerts) return;
  hipLaunchKernelGGL(k_skin_positions, dim3((count + kSkinBlock - 1) / kSkinBlock), dim3(kSkinBlock), 0, st, S.ids, S.w, nodePos, out,
                     first, count);
}

void launch_skin_normals(hipStream_t st, const SkinArrays& S, const float* x, float* out, uint32_t first, uint32_t count) {
  if (!count || first + static_cast<uint64_t>(count) > S.nVerts) return;
  hipLaunchKernelGGL(k_skin_normals, dim3((count + kSkinBlock - 1) / kSkinBlock), dim3(kSkinBlock), 0, st, S.incPtr, S.inc, S.tri, x, out,
                     first, count);
}

}  // namespace pies
