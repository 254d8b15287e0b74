// Device code shared by the files of the point-triangle pipeline (tri_detect.hip: grid, pair search, CCD; tri_lists.hip: contact
// list, per-node incidence, merged rows, dependency levels; tri_passes.hip: local step and sequential passes) and by the local-step
// kernels of pd_kernels.hip: the 3-vector, ranges of world cells, the reference's merge order, the contact local step, the levels
// of a 64-contact window and the constants both the level kernel and the passes are sized by.
#pragma once
#include <cstdint>

#include "cell_table.h"
#include "tri_kernels.h"

namespace pies {

struct F3 {
  float x, y, z;
};
PIES_DEV F3 f3(float x, float y, float z) { return {x, y, z}; }
PIES_DEV F3 operator+(F3 a, F3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
PIES_DEV F3 operator-(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
PIES_DEV F3 operator*(F3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
PIES_DEV F3 operator*(float s, F3 a) { return {s * a.x, s * a.y, s * a.z}; }
PIES_DEV F3 operator/(F3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
PIES_DEV F3 neg(F3 a) { return {-a.x, -a.y, -a.z}; }
PIES_DEV float dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PIES_DEV F3 cross(F3 a, F3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
PIES_DEV F3 normalize(F3 a) { return a * (1.0f / sqrtf(dot(a, a))); }
PIES_DEV F3 xyz(const float4& v) { return {v.x, v.y, v.z}; }

constexpr uint32_t kNil = kTriNil;

// Position of triangle t in the reference's merge order: thread (t mod T) owns triangles t, t + T, ... and the
// per-thread lists are concatenated thread after thread (Solver.cpp:714, 852).  cntTri / offTri are indexed by it.
PIES_DEV uint32_t merge_rank(uint32_t t, uint32_t nt, uint32_t threads) {
  const uint32_t th = t % threads, q = nt / threads, rem = nt % threads;
  return th * q + min(th, rem) + t / threads;
}

struct CellBox {  // a range of world cells [lo, hi) per axis
  int x0, y0, z0, x1, y1, z1;
};
PIES_DEV CellBox range_box(const int4& r, uint32_t lx, uint32_t ly, uint32_t lz) {
  return {r.x, r.y, r.z, r.x + static_cast<int>(lx), r.y + static_cast<int>(ly), r.z + static_cast<int>(lz)};
}
PIES_DEV int4 ent_range(const float4& e) { return make_int4(__float_as_int(e.x), __float_as_int(e.y), __float_as_int(e.z), __float_as_int(e.w)); }
PIES_DEV CellBox insert_box(const int4& r) { return range_box(r, r.w & 0xff, (r.w >> 8) & 0xff, (r.w >> 16) & 0xff); }
PIES_DEV CellBox meet(const CellBox& a, const CellBox& b) {
  return {max(a.x0, b.x0), max(a.y0, b.y0), max(a.z0, b.z0), min(a.x1, b.x1), min(a.y1, b.y1), min(a.z1, b.z1)};
}
PIES_DEV bool empty(const CellBox& b) { return b.x1 <= b.x0 || b.y1 <= b.y0 || b.z1 <= b.z0; }
PIES_DEV uint32_t volume(const CellBox& b) { return static_cast<uint32_t>((b.x1 - b.x0) * (b.y1 - b.y0) * (b.z1 - b.z0)); }
PIES_DEV bool holds(const CellBox& b, int x, int y, int z) { return x >= b.x0 && x < b.x1 && y >= b.y0 && y < b.y1 && z >= b.z0 && z < b.z1; }
// cells of the (non-empty) box b that come before cell (x, y, z) when a range is walked x-major (dx, dy, dz: Solver.cpp:722-724)
PIES_DEV uint32_t cells_before(const CellBox& b, int x, int y, int z) {
  const int nx = b.x1 - b.x0, ny = b.y1 - b.y0, nz = b.z1 - b.z0;
  int n = min(max(x - b.x0, 0), nx) * ny * nz;
  if (x >= b.x0 && x < b.x1) {
    n += min(max(y - b.y0, 0), ny) * nz;
    if (y >= b.y0 && y < b.y1) n += min(max(z - b.z0, 0), nz);
  }
  return static_cast<uint32_t>(n);
}

// ---- local step (CollisionConstraint.cpp:86-124) and w * (AtA p)_i (:176-194) of the contacts first, first + stride, ... -------
// (k_pd_local_tri sweeps the list with a grid of its own; in the fused launches of the strain + volume elements, k_pd_local_tet_pair
// and k_pd_local_tiles, a few extra workgroups do, so that a substep without contacts does not pay a launch boundary per
// local/global iteration for it)
PIES_DEV void tri_local_contacts(const TriArrays& T, const float4* __restrict__ pos, float thickness, uint32_t first, uint32_t stride) {
  const uint32_t M = T.counters[kTriCtrContacts];
  for (uint32_t c = first; c < M; c += stride) {
    const uint4 id = T.ids[c];
    F3 p[4] = {xyz(pos[id.x]), xyz(pos[id.y]), xyz(pos[id.z]), xyz(pos[id.w])};
    const F3 rel = p[0] - p[1];
    const F3 n = normalize(cross(p[2] - p[1], p[3] - p[1]));
    const float nDotP = dot(n, rel);
    if (nDotP < thickness) p[0] = p[0] + (thickness - nDotP) * n;
    // AtA = [[3,-1,-1,-1],[-1,1,0,0],[-1,0,1,0],[-1,0,0,1]], products accumulated from 0 in column order
    const float AtA[4][4] = {{3.f, -1.f, -1.f, -1.f}, {-1.f, 1.f, 0.f, 0.f}, {-1.f, 0.f, 1.f, 0.f}, {-1.f, 0.f, 0.f, 1.f}};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ax += AtA[i][k] * p[k].x;
        ay += AtA[i][k] * p[k].y;
        az += AtA[i][k] * p[k].z;
      }
      T.contrib[4 * c + i] = make_float4(kTriContactW * ax, kTriContactW * ay, kTriContactW * az, 0.f);
    }
  }
}

// ---- what the level kernel and the sequential passes share ------------------------------------------------------------------
constexpr int kSeqBlock = 1024;            // the workgroup of k_tri_levels, k_tri_tail_levels and k_tri_sequential
constexpr uint32_t kSeqLdsNodes = 4096;    // touched nodes the LDS copy of the sequential passes holds
// workgroup barrier that waits for this wavefront's LDS traffic only (requests to global memory stay in flight)
PIES_DEV void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// dependency level of every contact of a 64-contact window (contacts that share a node keep their list order)
PIES_DEV int window_levels(bool valid, const uint4& id, int lane, int& maxLevel, int base = 0) {
  int level = base;
  for (int m = 0; m < 63; ++m) {
    const int lm = __builtin_amdgcn_readlane(level, m);
    const uint32_t mx = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(id.x), m));
    const uint32_t my = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(id.y), m));
    const uint32_t mz = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(id.z), m));
    const uint32_t mw = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(id.w), m));
    const uint32_t mine[4] = {id.x, id.y, id.z, id.w};
    bool share = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) share = share || mine[k] == mx || mine[k] == my || mine[k] == mz || mine[k] == mw;
    if (valid && lane > m && share && mx != 0xffffffffu) level = max(level, lm + 1);
  }
  int mxl = valid ? level : 0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mxl = max(mxl, __shfl_xor(mxl, off, 64));
  maxLevel = mxl;
  return level;
}

}  // namespace pies
