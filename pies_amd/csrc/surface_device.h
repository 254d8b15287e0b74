// Device functions shared by the kernels that meet points or rays with a triangle list (ray_kernels.hip, near_kernels.hip,
// voxel_kernels.hip): small vectors, the gather of a triangle through a RayTarget, the 64-bit key whose minimum picks a winner,
// and the solid angle of one (point, triangle) pair.  Included by .hip files only.  Everything here is the IEEE sequence written
// (-ffp-contract=off): a kernel that calls one of these functions gets the bits every other caller gets.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "ray_kernels.h"

namespace pies {

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 load3(const float* p) { return {p[0], p[1], p[2]}; }

// bits of a value >= +0 above the triangle index: the minimum is the smallest value, the lowest triangle on equal values
__device__ __forceinline__ uint64_t surface_key(float value, uint32_t triangle) {
  return static_cast<uint64_t>(__float_as_uint(value)) << 32 | triangle;
}

__device__ __forceinline__ void gather_corners(const RayTarget& T, uint32_t t, V3& a, V3& b, V3& c) {
  const uint32_t* id = T.tri + 3ull * t;
  a = load3(T.pos + static_cast<size_t>(T.stride) * id[0]);
  b = load3(T.pos + static_cast<size_t>(T.stride) * id[1]);
  c = load3(T.pos + static_cast<size_t>(T.stride) * id[2]);
}
__device__ __forceinline__ void gather_triangle(const RayTarget& T, uint32_t t, V3& a, V3& e1, V3& e2) {
  V3 b, c;
  gather_corners(T, t, a, b, c);
  e1 = sub(b, a);
  e2 = sub(c, a);
}

// The solid angle of the triangle whose corners, seen from the point, are A, B, D (van Oosterom and Strackee; the rule of
// pies_voxelize_tri_mesh in pies_hip.h, restated by tests/test_trimesh.py: _terms).  0 where it is undefined (the point on a
// corner or an edge line: num = den = 0) or not finite.
__device__ __forceinline__ float solid_angle(float ax, float ay, float az, float bx, float by, float bz, float dx, float dy, float dz) {
  const float la = sqrtf(ax * ax + ay * ay + az * az);
  const float lb = sqrtf(bx * bx + by * by + bz * bz);
  const float ld = sqrtf(dx * dx + dy * dy + dz * dz);
  // det [A, B, D] (columns), the expansion det3 of skin.cpp
  const float num = ax * (by * dz - dy * bz) - bx * (ay * dz - dy * az) + dx * (ay * bz - by * az);
  const float ab = ax * bx + ay * by + az * bz;
  const float bd = bx * dx + by * dy + bz * dz;
  const float da = dx * ax + dy * ay + dz * az;
  const float den = la * lb * ld + ab * ld + bd * la + da * lb;
  float omega = 2.0f * atan2f(num, den);
  if ((num == 0.0f && den == 0.0f) || !(fabsf(omega) <= 3.402823466e+38f)) omega = 0.0f;  // (NaN too)
  return omega;
}

}  // namespace pies
