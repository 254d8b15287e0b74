// Embedded surface meshes (pies_add_skin): the device side.  Every skin of a handle lives in one set of arrays, skin after
// skin, so that a frame's export is two launches whatever the number of skins; vertex and triangle indices are global to
// that concatenation.  Launch wrappers like kernels.h: no allocation, no synchronisation, everything on the caller's stream.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pies {

struct SkinArrays {
  uint32_t nVerts = 0;              // over all skins
  uint32_t nTris = 0;
  const uint4* ids = nullptr;       // per vertex: the four nodes of its tetrahedron, DEVICE numbering
  const float4* w = nullptr;        // per vertex: (w1, w2, w3, unused); w0 = 1 - (w1 + w2 + w3) is implied
  const uint32_t* tri = nullptr;    // 3 per triangle: vertex indices (global)
  const uint32_t* incPtr = nullptr; // nVerts + 1: the triangles that name a vertex are inc[incPtr[v] .. incPtr[v + 1]), ascending
  const uint32_t* inc = nullptr;
};

// x[v] = p0 + w1 (p1 - p0) + w2 (p2 - p0) + w3 (p3 - p0) for v in [first, first + count), packed 3 floats per vertex at out[3 v]
void launch_skin_positions(hipStream_t st, const SkinArrays& S, const float4* nodePos, float* out, uint32_t first, uint32_t count);
// normal[v] = normalize(sum of cross(x_b - x_a, x_c - x_a) over v's triangles, ascending) from the skinned positions x (the
// array launch_skin_positions filled); (0, 0, 0) when the sum's squared length is 0 or not finite
void launch_skin_normals(hipStream_t st, const SkinArrays& S, const float* x, float* out, uint32_t first, uint32_t count);

}  // namespace pies
