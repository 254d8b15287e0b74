// Point-triangle collisions of the Projective-Dynamics substep, first stage: detection.
//
//   detection  Src/Solver.cpp:680-875: the reference inserts every surface triangle into a world-unit cell grid over the
//              AABB of its nodes' current and previous positions (TriCompRange :942-979, sweptTriRange :639-677);
//              for every triangle, every triangle without a common node found in the cells of its swept range
//              is tested with three point-triangle CCDs (CollisionDetection.cpp:227-302).  Contacts are listed
//              in the reference's order: thread by thread (triangle id modulo threadCount), triangle by
//              triangle, cell by cell (dx,dy,dz), bucket entry by entry (ascending triangle id), point by
//              point -- including the duplicates a pair produces when it shares several cells.  The device finds the
//              same pairs from a grid that holds every triangle once (tri_kernels.h) and writes the same list.
//   This file: the CCD, the triangle grid, the pair search and the hit records.  The list, the per-node incidence, the merged rows
//   and the dependency levels are tri_lists.hip; the constraint's local step and the sequential passes tri_passes.hip.
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "tri_device.h"

namespace pies {

constexpr int kBlock = 256;
constexpr int kTriTeam = 16;  // lanes sharing one triangle's candidate list in the counting pass
static inline dim3 grid_for(uint32_t n) { return dim3((n + kBlock - 1) / kBlock); }

// inverse(mat3(c0, c1, c2)) * v with glm's cofactor formula (columns c0, c1, c2)
PIES_DEV F3 solve_columns(F3 c0, F3 c1, F3 c2, F3 v) {
  const float m00 = c0.x, m01 = c0.y, m02 = c0.z, m10 = c1.x, m11 = c1.y, m12 = c1.z, m20 = c2.x, m21 = c2.y, m22 = c2.z;
  const float det = +m00 * (m11 * m22 - m21 * m12) - m10 * (m01 * m22 - m21 * m02) + m20 * (m01 * m12 - m11 * m02);
  const float ood = 1.0f / det;
  const float i00 = +(m11 * m22 - m21 * m12) * ood, i10 = -(m10 * m22 - m20 * m12) * ood, i20 = +(m10 * m21 - m20 * m11) * ood;
  const float i01 = -(m01 * m22 - m21 * m02) * ood, i11 = +(m00 * m22 - m20 * m02) * ood, i21 = -(m00 * m21 - m20 * m01) * ood;
  const float i02 = +(m01 * m12 - m11 * m02) * ood, i12 = -(m00 * m12 - m10 * m02) * ood, i22 = +(m00 * m11 - m10 * m01) * ood;
  return {i00 * v.x + i10 * v.y + i20 * v.z, i01 * v.x + i11 * v.y + i21 * v.z, i02 * v.x + i12 * v.y + i22 * v.z};
}
PIES_DEV bool bary_outside(F3 b) { return (0.0f > b.x) || (b.x > 1.0f) || (0.0f > b.y) || (b.y > 1.0f) || (b.x + b.y > 1.0f); }

struct Cubic {
  float c3, c2, c1, c0;
};
PIES_DEV float eval(const Cubic& c, float t) {
  const float t2 = t * t;
  return c.c3 * t2 * t + c.c2 * t2 + c.c1 * t + c.c0;
}
PIES_DEV void expand_term(float a0, float b0, float c0, float ad, float bd, float cd, Cubic& e) {  // CollisionDetection.cpp:209-221
  e.c3 += ad * bd * cd;
  e.c2 += ad * bd * c0 + a0 * bd * cd + ad * b0 * cd;
  e.c1 += ad * b0 * c0 + a0 * bd * c0 + a0 * b0 * cd;
  e.c0 += a0 * b0 * c0;
}
// smallest real root of a genuine cubic in [0,1]: monotone pieces between the critical points, first sign
// change bisected 32 times (stands in for the companion-matrix eigenvalues of CollisionDetection.cpp:189-204)
PIES_DEV bool cubic_smallest_root01(const Cubic& c, float& root) {
  float cuts[4];
  int nc = 0;
  cuts[nc++] = 0.0f;
  const float a = 3.0f * c.c3, b = 2.0f * c.c2, cc = c.c1;
  const float disc = b * b - 4.0f * a * cc;
  if (disc > 0.0f) {
    const float sq = sqrtf(disc);
    float t0 = (-b - sq) / (2.0f * a), t1 = (-b + sq) / (2.0f * a);
    if (t0 > t1) { const float tmp = t0; t0 = t1; t1 = tmp; }
    if (t0 > 0.0f && t0 < 1.0f) cuts[nc++] = t0;
    if (t1 > 0.0f && t1 < 1.0f) cuts[nc++] = t1;
  }
  cuts[nc++] = 1.0f;
  for (int k = 0; k + 1 < nc; ++k) {
    float lo = cuts[k], hi = cuts[k + 1];
    float flo = eval(c, lo), fhi = eval(c, hi);
    if (flo == 0.0f) { root = lo; return true; }
    if (flo * fhi > 0.0f) continue;
    for (int it = 0; it < 32; ++it) {
      const float mid = 0.5f * (lo + hi);
      const float fm = eval(c, mid);
      if ((flo < 0.0f) == (fm < 0.0f) && fm != 0.0f) { lo = mid; flo = fm; } else { hi = mid; fhi = fm; }
    }
    root = hi;
    return true;
  }
  return false;
}
PIES_DEV bool find_root(const Cubic& c, float& t) {  // CollisionDetection.cpp:143-205
  if (c.c3 == 0.0f) {
    if (c.c2 == 0.0f) {
      if (c.c1 == 0.0f) {
        if (c.c0 == 0.0f) { t = 0.0f; return true; }
        return false;
      }
      t = -c.c0 / c.c1;
      return t >= 0.0f && t <= 1.0f;
    }
    const float disc = c.c1 * c.c1 - 4.0f * c.c2 * c.c0;
    if (disc < 0.0f) return false;
    const float sq = sqrtf(disc);
    t = (-c.c1 - sq) / (2.0f * c.c2);
    if (t > 1.0f) return false;
    if (t < 0.0f) t = (-c.c1 + sq) / (2.0f * c.c2);
    return t >= 0.0f && t <= 1.0f;
  }
  return cubic_smallest_root01(c, t);
}
// CollisionDetection.cpp:227-302
PIES_DEV bool point_triangle_ccd(F3 ap0, F3 ab0, F3 ac0, F3 ap1, F3 ab1, F3 ac1, float threshold) {
  const F3 n0 = normalize(cross(ab0, ac0)), n1 = normalize(cross(ab1, ac1));
  const float d0 = dot(n0, ap0), d1 = dot(n1, ap1);
  if (d0 * d1 >= 0.0f) {
    if (d1 >= 0.0f && d1 < threshold) return !bary_outside(solve_columns(ab1, ac1, n1, ap1));
    return false;
  }
  const F3 apd = ap1 - ap0, abd = ab1 - ab0, acd = ac1 - ac0;
  Cubic e{0.f, 0.f, 0.f, 0.f};
  expand_term(ap0.x, ab0.y, ac0.z, apd.x, abd.y, acd.z, e);
  expand_term(-ap0.x, ac0.y, ab0.z, -apd.x, acd.y, abd.z, e);
  expand_term(-ab0.x, ap0.y, ac0.z, -abd.x, apd.y, acd.z, e);
  expand_term(ab0.x, ac0.y, ap0.z, abd.x, acd.y, apd.z, e);
  expand_term(ac0.x, ap0.y, ab0.z, acd.x, apd.y, abd.z, e);
  expand_term(-ac0.x, ab0.y, ap0.z, -acd.x, abd.y, apd.z, e);
  float t;
  if (!find_root(e, t)) return false;
  const F3 apt = ap0 + t * apd, abt = ab0 + t * abd, act = ac0 + t * acd;
  const F3 n = normalize(cross(abt, act));
  return !bary_outside(solve_columns(abt, act, n, apt));
}

// ---- triangle grid (tri_kernels.h: every triangle once, in the cell of its range's minimum corner) ----------------------
PIES_DEV uint32_t grid_slot(const TriGridLevel& L, int x, int y, int z) {  // cell coordinates of the level -> slot (modulo the table)
  const uint32_t ux = static_cast<uint32_t>(x) & ((1u << L.lx) - 1u), uy = static_cast<uint32_t>(y) & ((1u << L.ly) - 1u),
                 uz = static_cast<uint32_t>(z) & ((1u << L.lz) - 1u);
  return L.base + ((((ux << L.ly) | uy) << L.lz) | uz);
}
// cells of the level a range of `len` world cells from `m` spans
PIES_DEV uint32_t level_extent(int m, uint32_t len, uint32_t shift) { return static_cast<uint32_t>(((m + static_cast<int>(len) - 1) >> shift) - (m >> shift)) + 1u; }

// TriCompRange / sweptTriRange: floor(min), ceil(max) - floor(min) over position and prevPosition, world units; the triangle's
// record for the detection (box of its six corner positions, "both normals are non-zero"); its size class and slot.
__global__ void __launch_bounds__(kBlock) k_tri_box(TriArrays T, const float4* __restrict__ pos, const float4* __restrict__ prev) {
  __shared__ uint32_t sExt[kTriLevels], sCnt[kTriLevels];
  if (threadIdx.x < kTriLevels) { sExt[threadIdx.x] = 0; sCnt[threadIdx.x] = 0; }
  __syncthreads();
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  uint32_t slot = kNil;
  int cls = -1;
  uint32_t ext = 0;
  if (t < T.nt) {
    const uint32_t i0 = T.tris[3 * t], i1 = T.tris[3 * t + 1], i2 = T.tris[3 * t + 2];
    const F3 b1 = xyz(pos[i0]), c1 = xyz(pos[i1]), d1 = xyz(pos[i2]);
    const F3 b0 = xyz(prev[i0]), c0 = xyz(prev[i1]), d0 = xyz(prev[i2]);
    const float pv[3][3] = {{b1.x, b1.y, b1.z}, {c1.x, c1.y, c1.z}, {d1.x, d1.y, d1.z}};
    const float qv[3][3] = {{b0.x, b0.y, b0.z}, {c0.x, c0.y, c0.z}, {d0.x, d0.y, d0.z}};
    float mn[3], mx[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (i == 0) { mx[k] = pv[i][k]; mn[k] = pv[i][k]; }
        mx[k] = fmaxf(pv[i][k], mx[k]); mx[k] = fmaxf(qv[i][k], mx[k]);
        mn[k] = fminf(pv[i][k], mn[k]); mn[k] = fminf(qv[i][k], mn[k]);
      }
    }
    int m[3];
    uint32_t len[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float f = floorf(mn[k]);
      ok = ok && (fabsf(f) < 1.0e6f) && (fabsf(mx[k]) < 1.0e6f);
      m[k] = ok ? static_cast<int>(f) : 0;
      len[k] = ok ? static_cast<uint32_t>(ceilf(mx[k]) - static_cast<float>(static_cast<long long>(f))) : 0u;
    }
    if (!ok) atomicOr(&T.counters[kTriCtrFailure], kTriFailNonFinite);
    if (!ok || len[0] > kTriInsertMaxCells || len[1] > kTriInsertMaxCells || len[2] > kTriInsertMaxCells)
      len[0] = len[1] = len[2] = 0;  // the reference returns an empty range (Solver.cpp:974-976)
    T.rng[t] = make_int4(m[0], m[1], m[2], static_cast<int>(len[0] | (len[1] << 8) | (len[2] << 16)));
    const F3 nn0 = cross(c0 - b0, d0 - b0), nn1 = cross(c1 - b1, d1 - b1);
    const bool regular = dot(nn0, nn0) > 0.0f && dot(nn1, nn1) > 0.0f;
    T.boxOf[4 * t] = make_float4(mn[0], mn[1], mn[2], __uint_as_float(t));
    T.boxOf[4 * t + 1] = make_float4(mx[0], mx[1], mx[2], regular ? 1.0f : 0.0f);
    T.boxOf[4 * t + 2] = make_float4(__int_as_float(m[0]), __int_as_float(m[1]), __int_as_float(m[2]), __uint_as_float(len[0] | (len[1] << 8) | (len[2] << 16)));
    T.boxOf[4 * t + 3] = make_float4(__uint_as_float(i0), __uint_as_float(i1), __uint_as_float(i2), 0.0f);
    T.head[t] = kNil;
    if (len[0] * len[1] * len[2] != 0u) {
      int k = 0;
#pragma unroll
      for (int l = kTriLevels - 1; l >= 0; --l) {  // the finest class whose cells the range spans at most kTriLevelExt of per axis
        const uint32_t sh = T.level[l].shift;
        const uint32_t e = max(max(level_extent(m[0], len[0], sh), level_extent(m[1], len[1], sh)), level_extent(m[2], len[2], sh));
        if (l == kTriLevels - 1 || e <= kTriLevelExt) { k = l; ext = e; }
      }
      cls = k;
      const uint32_t sh = T.level[k].shift;
      slot = grid_slot(T.level[k], m[0] >> sh, m[1] >> sh, m[2] >> sh);
      T.posIn[t] = atomicAdd(&T.cellCnt[slot], 1u);
    }
    T.cellOf[t] = slot;
  }
  // (word 0 and the words from the used nodes to the row entries: tri_reset leaves them to this kernel)
  if (blockIdx.x == 0 && (threadIdx.x == 0 || (threadIdx.x >= kTriCtrUsedNodes && threadIdx.x <= kTriCtrRowEntries))) T.counters[threadIdx.x] = 0;
  // the tiles' sums for the prefix sum over the slots: the triangles of a wavefront are neighbours, so their slots lie in a few
  // tiles - one atomic per wavefront and tile
  for (unsigned long long todo = __ballot(slot != kNil); todo;) {
    const uint32_t tile = __shfl(slot, __builtin_ctzll(todo), 64) / kGridTile;
    const unsigned long long same = __ballot(slot != kNil && slot / kGridTile == tile);
    if ((threadIdx.x & 63u) == static_cast<uint32_t>(__builtin_ctzll(same))) atomicAdd(&T.tileSum[tile], static_cast<uint32_t>(__popcll(same)));
    todo &= ~same;
  }
  // the classes' statistics: per wavefront a count per class and - only while it still raises it - the longest range
#pragma unroll
  for (int k = 0; k < kTriLevels; ++k) {
    const unsigned long long in = __ballot(cls == k);
    if (in == 0ull) continue;
    if ((threadIdx.x & 63u) == static_cast<uint32_t>(__builtin_ctzll(in))) atomicAdd(&sCnt[k], static_cast<uint32_t>(__popcll(in)));
    if (cls == k && sExt[k] < ext) atomicMax(&sExt[k], ext);
  }
  __syncthreads();
  if (threadIdx.x < kTriLevels && sCnt[threadIdx.x]) {
    atomicMax(&T.counters[kTriCtrLongest + threadIdx.x], sExt[threadIdx.x]);
    atomicAdd(&T.counters[kTriCtrListed + threadIdx.x], sCnt[threadIdx.x]);
  }
}
// first entry of every slot = the exclusive prefix sum of the slots' counts, in slot order, so that the slots of a row of cells
// (consecutive z) have their entries in one stretch.  The sums of tiles of kGridTile slots come from k_tri_box; every tile adds up
// the sums before it and scans its own slots.
__global__ void __launch_bounds__(kBlock) k_tri_starts(TriArrays T) {
  __shared__ uint32_t red[kBlock / 64], wsum[kBlock / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t before = 0;
  for (uint32_t b = threadIdx.x; b < blockIdx.x; b += kBlock) before += T.tileSum[b];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) before += __shfl_xor(before, off, 64);
  if (lane == 0u) red[wave] = before;
  // this thread's 8 consecutive slots
  const size_t first = static_cast<size_t>(kGridTile) * blockIdx.x + 8u * threadIdx.x;
  const uint4 a = *reinterpret_cast<const uint4*>(T.cellCnt + first), b = *reinterpret_cast<const uint4*>(T.cellCnt + first + 4);
  const uint32_t mine = (a.x + a.y) + (a.z + a.w) + (b.x + b.y) + (b.z + b.w);
  uint32_t incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t v = __shfl_up(incl, off, 64);
    if (lane >= static_cast<uint32_t>(off)) incl += v;
  }
  if (lane == 63u) wsum[wave] = incl;
  __syncthreads();
  uint32_t run = (red[0] + red[1]) + (red[2] + red[3]);
  for (uint32_t w = 0; w < wave; ++w) run += wsum[w];
  run += incl - mine;
  uint4 oa, ob;
  oa.x = run; oa.y = oa.x + a.x; oa.z = oa.y + a.y; oa.w = oa.z + a.z;
  ob.x = oa.w + a.w; ob.y = ob.x + b.x; ob.z = ob.y + b.y; ob.w = ob.z + b.z;
  *reinterpret_cast<uint4*>(T.cellStart + first) = oa;
  *reinterpret_cast<uint4*>(T.cellStart + first + 4) = ob;
  if (blockIdx.x == gridDim.x - 1u && threadIdx.x == kBlock - 1u) T.cellStart[T.slots] = ob.w + b.w;
}
__global__ void __launch_bounds__(kBlock) k_tri_fill(TriArrays T) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= T.nt) return;
  const uint32_t s = T.cellOf[t];
  if (s == kNil) return;
  const uint32_t at = T.cellStart[s] + T.posIn[t];
#pragma unroll
  for (int i = 0; i < 4; ++i) T.ent[4 * at + i] = T.boxOf[4 * t + i];
}

// the window of class L a partner of a triangle with range box S can be listed in: its minimum corner lies in S grown downwards
// by (the longest range listed in the class - 1) cells of the class
struct Window {
  int x0, y0, z0;
  uint32_t wx, wy, wz;
};
PIES_DEV Window window_of(const CellBox& S, uint32_t shift, uint32_t longest) {
  Window w;
  const int grow = static_cast<int>(longest) - 1;
  w.x0 = (S.x0 >> shift) - grow; w.y0 = (S.y0 >> shift) - grow; w.z0 = (S.z0 >> shift) - grow;
  w.wx = static_cast<uint32_t>(((S.x1 - 1) >> shift) - w.x0 + 1);
  w.wy = static_cast<uint32_t>(((S.y1 - 1) >> shift) - w.y0 + 1);
  w.wz = static_cast<uint32_t>(((S.z1 - 1) >> shift) - w.z0 + 1);
  return w;
}

// The entries of one row of a window - the cells (x, y, z0 .. z0 + wz) of a class - are one stretch of the entry list, or two
// when the row runs past the end of the table's z axis and goes on at its start.
struct RowRun {
  uint32_t s1, c1, s2, c2;
};
PIES_DEV RowRun row_run(const TriArrays& T, const TriGridLevel& L, int x, int y, int z0, uint32_t wz) {
  const uint32_t ux = static_cast<uint32_t>(x) & ((1u << L.lx) - 1u), uy = static_cast<uint32_t>(y) & ((1u << L.ly) - 1u);
  const uint32_t nz = 1u << L.lz, uz = static_cast<uint32_t>(z0) & (nz - 1u);
  const uint32_t row = L.base + (((ux << L.ly) | uy) << L.lz);
  RowRun r;
  r.s1 = T.cellStart[row + uz];
  if (uz + wz <= nz) {
    r.c1 = T.cellStart[row + uz + wz] - r.s1;
    r.s2 = 0; r.c2 = 0;
  } else {
    r.c1 = T.cellStart[row + nz] - r.s1;
    r.s2 = T.cellStart[row];
    r.c2 = T.cellStart[row + (uz + wz - nz)] - r.s2;
  }
  return r;
}

// Solver.cpp:751-755 - a bucket of more than 1000 triangles fails the sim - for a triangle whose windows list more than 1000
// triangles (otherwise no cell of its range can be in that many ranges): the exact number of ranges every cell of its range lies
// in.  Rare (a collapsed mesh) and slow: per cell of the range, every listed triangle of the windows.
template <int TEAM>
PIES_DEV bool crowded_cell(const TriArrays& T, const CellBox& S, uint32_t member) {
  for (int x = S.x0; x < S.x1; ++x)
    for (int y = S.y0; y < S.y1; ++y)
      for (int z = S.z0; z < S.z1; ++z) {
        uint32_t cover = 0;
        for (int k = 0; k < kTriLevels; ++k) {
          if (T.counters[kTriCtrListed + k] == 0u) continue;
          const Window W = window_of(S, T.level[k].shift, T.counters[kTriCtrLongest + k]);
          const uint32_t rows = W.wx * W.wy;
          for (uint32_t w = member; w < rows; w += TEAM) {
            const uint32_t dx = w / W.wy, dy = w - dx * W.wy;
            const RowRun r = row_run(T, T.level[k], W.x0 + (int)dx, W.y0 + (int)dy, W.z0, W.wz);
            for (uint32_t e = 0; e < r.c1 + r.c2; ++e) {
              const uint32_t at = e < r.c1 ? r.s1 + e : r.s2 + (e - r.c1);
              if (holds(insert_box(ent_range(T.ent[4 * at + 2])), x, y, z)) ++cover;
            }
          }
        }
#pragma unroll
        for (int off = TEAM / 2; off >= 1; off >>= 1) cover += __shfl_xor(cover, off, TEAM);
        if (cover > 1000u) return true;
        if (T.counters[kTriCtrFailure]) return false;  // somebody else has failed the sim already
      }
  return false;
}

// ---- detection (Solver.cpp:714-797).  The reference walks the cells of a triangle's range and tests every triangle listed
// there without a common node, corner by corner; a pair that shares c cells is tested c times with the same result.  Two launches:
//
// k_tri_pairs  TEAM lanes share a triangle.  The team walks the windows of the three size classes row by row, TEAM rows at a time
//              (a lane per row: where its entries are and how many), forms the running offsets and walks the rows' entries as ONE
//              list, TEAM at a time; a partner is met once: its box - in the entry - against the box of the triangle's three
//              swept corners first (most partners of a window end here), then the ranges' intersection (none: the reference
//              never pairs them), the common nodes, the corners one by one.  What is left - a pair and the corners to test - goes
//              into the work list.  Nothing here is heavy (with the CCD inlined the kernel held 192 registers - two wavefronts per
//              SIMD - and took 43 us of a 470 us substep; 20 us now, the CCD's launch 8 on top of its floor).
// k_tri_ccd    one lane per entry of the work list: the CCD of the listed corners (Solver.cpp:775-797); a pair with hits goes
//              into the pool of hit records {triangle, partner, corners}, chained per triangle, and adds (hits x shared cells)
//              to the triangle's contacts (cntTri).  k_tri_emit writes the list from the records.
constexpr uint32_t kPairStage = 1024;  // pairs a workgroup (16 triangles) collects in LDS; a triangle of a moving lattice leaves ~15
// The work list is kWorkShards lists with a counter each, 64 bytes apart (workCnt[16 s]): atomics on ONE word take their turns at
// ~9 ns each on this chip (measured: 29 000 of them made a 10 us kernel a 260 us one), and so do the loads of its neighbours in
// the line; a workgroup appends to the list of its index modulo kWorkShards.
PIES_DEV uint32_t shard_capacity(const TriArrays& T) { return T.maxWork / kWorkShards; }
PIES_DEV void work_append(const TriArrays& T, uint32_t shard, uint2 item) {
  for (uint32_t tries = 0; tries < kWorkShards; ++tries, shard = (shard + 1u) % kWorkShards) {  // (a full list passes the item on)
    const uint32_t at = atomicAdd(&T.workCnt[16u * shard], 1u);
    if (at < shard_capacity(T)) { T.work[shard * shard_capacity(T) + at] = item; return; }
  }
  atomicOr(&T.counters[kTriCtrFailure], kTriFailOverflow);
}
template <int TEAM>
__global__ void __launch_bounds__(kBlock) k_tri_pairs(TriArrays T, const float4* __restrict__ pos, const float4* __restrict__ prev, float threshold) {
  // the workgroup's part of the work list is collected in LDS and appended at the end: one atomic per workgroup on the list's
  // counter (an append per wavefront and round of candidates put 200 000 atomics on that one word: 370 us)
  __shared__ uint2 sWork[kPairStage];
  __shared__ uint32_t sCount, sBase;
  if (threadIdx.x == 0) sCount = 0;
  __syncthreads();
  const uint32_t t = (blockIdx.x * kBlock + threadIdx.x) / TEAM, member = threadIdx.x % TEAM;
  bool search = t < T.nt && T.counters[kTriCtrFailure] == 0u;  // a team lies inside one wavefront and stays together
  int4 rg = make_int4(0, 0, 0, 0);
  uint32_t lx = 0, ly = 0, lz = 0;
  if (search) {
    if (member == 0) T.cntTri[merge_rank(t, T.nt, T.threadCount)] = 0;
    rg = T.rng[t];
    lx = rg.w & 0xff; ly = (rg.w >> 8) & 0xff; lz = (rg.w >> 16) & 0xff;
    if (lx > kTriSearchMaxCells || ly > kTriSearchMaxCells || lz > kTriSearchMaxCells) lx = ly = lz = 0;  // sweptTriRange: empty (Solver.cpp:672-674)
    const uint32_t ncell = lx * ly * lz;
    if (ncell == 0u || ncell > 1000u) {
      // Solver.cpp:741-745: more than 1000 buckets in a range fails the sim - every cell of a searching triangle's range has a
      // bucket, the triangle's own entry
      if (ncell && member == 0) atomicOr(&T.counters[kTriCtrFailure], kTriFailBucket);
      search = false;
    }
  }
  if (search) {
  const CellBox S = range_box(rg, lx, ly, lz);
  const uint32_t ia[3] = {T.tris[3 * t], T.tris[3 * t + 1], T.tris[3 * t + 2]};
  F3 slo[3], shi[3];  // the corners' swept segments as boxes
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const F3 p1 = xyz(pos[ia[i]]), p0 = xyz(prev[ia[i]]);
    slo[i] = {fminf(p0.x, p1.x), fminf(p0.y, p1.y), fminf(p0.z, p1.z)};
    shi[i] = {fmaxf(p0.x, p1.x), fmaxf(p0.y, p1.y), fmaxf(p0.z, p1.z)};
  }
  const F3 tlo = {fminf(fminf(slo[0].x, slo[1].x), slo[2].x), fminf(fminf(slo[0].y, slo[1].y), slo[2].y), fminf(fminf(slo[0].z, slo[1].z), slo[2].z)};
  const F3 thi = {fmaxf(fmaxf(shi[0].x, shi[1].x), shi[2].x), fmaxf(fmaxf(shi[0].y, shi[1].y), shi[2].y), fmaxf(fmaxf(shi[0].z, shi[1].z), shi[2].z)};
  uint32_t listed = 0;
  for (int k = 0; k < kTriLevels; ++k) {
    if (T.counters[kTriCtrListed + k] == 0u) continue;
    const TriGridLevel L = T.level[k];
    const Window W = window_of(S, L.shift, T.counters[kTriCtrLongest + k]);
    const uint32_t rows = W.wx * W.wy;
    const float invWy = 1.0f / static_cast<float>(W.wy);
    for (uint32_t w0 = 0; w0 < rows; w0 += TEAM) {
      // this lane's row of the round
      const uint32_t w = w0 + member;
      RowRun run = {0u, 0u, 0u, 0u};
      if (w < rows) {
        const uint32_t dx = static_cast<uint32_t>((static_cast<float>(w) + 0.5f) * invWy), dy = w - dx * W.wy;  // (rows < 2^10: exact)
        run = row_run(T, L, W.x0 + (int)dx, W.y0 + (int)dy, W.z0, W.wz);
      }
      const uint32_t bc = run.c1 + run.c2;
      // offsets of the round's rows in the round's candidate list
      uint32_t incl = bc;
#pragma unroll
      for (int off = 1; off < TEAM; off <<= 1) {
        const uint32_t below = __shfl_up(incl, off, TEAM);
        if (static_cast<int>(member) >= off) incl += below;
      }
      const uint32_t pre = incl - bc, total = __shfl(incl, TEAM - 1, TEAM);
      listed += total;
      for (uint32_t k0 = 0; k0 < total; k0 += TEAM) {  // (total is the team's: its lanes stay together)
        const uint32_t kk = k0 + member;
        // where candidate kk sits: its row is the last one of the round whose offset is <= kk (empty rows share their
        // offset with the next one, so "the last" is never one of them): a binary search over the team's lanes (every
        // lane takes part in every shuffle - a lane past the end of the list searches too and drops the result)
        uint32_t l = 0;
#pragma unroll
        for (int step = TEAM / 2; step >= 1; step >>= 1) {
          const uint32_t pm = __shfl(pre, static_cast<int>(l) + step, TEAM);
          if (pm <= kk) l += static_cast<uint32_t>(step);
        }
        const uint32_t pl = __shfl(pre, static_cast<int>(l), TEAM);
        const uint32_t rs1 = __shfl(run.s1, static_cast<int>(l), TEAM), rc1 = __shfl(run.c1, static_cast<int>(l), TEAM), rs2 = __shfl(run.s2, static_cast<int>(l), TEAM);
        uint32_t o = 0, tests = 0;
        if (kk < total) {
          const uint32_t at = kk - pl < rc1 ? rs1 + (kk - pl) : rs2 + (kk - pl - rc1);
          const float4 e0 = T.ent[4 * at], e1 = T.ent[4 * at + 1], e2 = T.ent[4 * at + 2], e3 = T.ent[4 * at + 3];  // (all four at once: no load waits for another)
          // Conservative reject before anything else.  A hit puts a corner, at some time in [0,1], within `threshold` of a
          // point of the moving partner (proximity branch: at t = 1; crossing branch: on it at the root), so the corner's
          // swept segment must meet the box of the partner's six corner positions grown by the threshold; the margin adds 5 %
          // and 1e-3 of the box on top of that, orders of magnitude above the rounding of the barycentric test.  First all
          // three segments at once (their common box), then one by one.  A partner with a vanishing normal (NaN inside the
          // CCD, which then cannot say "outside") is never rejected here, nor is anything non-finite: every comparison below
          // is false for NaN.
          const bool regular = e1.w != 0.0f;
          const F3 lo = {e0.x, e0.y, e0.z}, hi = {e1.x, e1.y, e1.z};
          const float margin = 1.05f * threshold + 1.0e-3f * fmaxf(fmaxf(hi.x - lo.x, hi.y - lo.y), hi.z - lo.z);
          const bool apartAll = (thi.x < lo.x - margin) || (tlo.x > hi.x + margin) || (thi.y < lo.y - margin) || (tlo.y > hi.y + margin) ||
                                (thi.z < lo.z - margin) || (tlo.z > hi.z + margin);
          if (!(regular && apartAll)) {
            o = __float_as_uint(e0.w);
            if (!empty(meet(S, insert_box(ent_range(e2))))) {  // (no cell lists both: the reference never sees the pair)
              const uint32_t ib = __float_as_uint(e3.x), ic = __float_as_uint(e3.y), idd = __float_as_uint(e3.z);
              bool common = false;
#pragma unroll
              for (int i = 0; i < 3; ++i) common = common || ia[i] == ib || ia[i] == ic || ia[i] == idd;
              if (!common) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                  const bool apart = (shi[i].x < lo.x - margin) || (slo[i].x > hi.x + margin) || (shi[i].y < lo.y - margin) || (slo[i].y > hi.y + margin) ||
                                     (shi[i].z < lo.z - margin) || (slo[i].z > hi.z + margin);
                  if (!(regular && apart)) tests |= 1u << i;
                }
              }
            }
          }
        }
        // the pairs that are left: one LDS append per wavefront for those of its lanes
        const unsigned long long keep = __ballot(tests != 0u);
        if (keep) {
          const int leader = __builtin_ctzll(keep);
          uint32_t base = 0;
          if (static_cast<int>(threadIdx.x & 63u) == leader) base = atomicAdd(&sCount, static_cast<uint32_t>(__popcll(keep)));
          base = __shfl(base, leader, 64);
          if (tests) {
            const uint32_t at = base + static_cast<uint32_t>(__popcll(keep & ((1ull << (threadIdx.x & 63u)) - 1ull)));
            const uint2 item = make_uint2(t, o | (tests << 29));
            if (at < kPairStage) sWork[at] = item;
            else work_append(T, blockIdx.x % kWorkShards, item);  // (more than the stage holds: straight to the list)
          }
        }
      }
    }
  }
  // Solver.cpp:751-755 (a bucket of more than 1000 triangles): the triangles whose ranges hold a cell are all listed in the windows
  if (listed > 1000u && crowded_cell<TEAM>(T, S, member) && member == 0) atomicOr(&T.counters[kTriCtrFailure], kTriFailBucket);
  }
  __syncthreads();
  const uint32_t staged = min(sCount, kPairStage);
  // The workgroup's list, and - when that one is full (a mesh folded locally fills ONE list while the others are nearly empty:
  // ADVICE r4) - the lists behind it, each taking what it has room for; only when every list is full is the work list as a whole
  // (128 pairs per triangle) exhausted, which is as fatal as the contact list it would overflow.  (A list's counter may run past its
  // capacity: k_tri_ccd reads min(counter, capacity) entries, and exactly those were written.)
  const uint32_t cap = shard_capacity(T);
  uint32_t done = 0;
  for (uint32_t tries = 0; tries < kWorkShards && done < staged; ++tries) {  // (workgroup uniform)
    const uint32_t shard = (blockIdx.x + tries) % kWorkShards;
    __syncthreads();
    if (threadIdx.x == 0) sBase = atomicAdd(&T.workCnt[16u * shard], staged - done);
    __syncthreads();
    const uint32_t base = min(sBase, cap), fit = min(staged - done, cap - base);
    for (uint32_t i = threadIdx.x; i < fit; i += kBlock) T.work[shard * cap + base + i] = sWork[done + i];
    done += fit;
  }
  if (done < staged && threadIdx.x == 0) atomicOr(&T.counters[kTriCtrFailure], kTriFailOverflow);
}

__global__ void __launch_bounds__(kBlock) k_tri_ccd(TriArrays T, const float4* __restrict__ pos, const float4* __restrict__ prev, float threshold) {
  if (T.counters[kTriCtrFailure]) return;
  // workgroup b works on list b % kWorkShards, with the other workgroups of that list
  const uint32_t shard = blockIdx.x % kWorkShards, cap = shard_capacity(T);
  const uint32_t n = min(T.workCnt[16u * shard], cap);
  for (uint32_t w = (blockIdx.x / kWorkShards) * kBlock + threadIdx.x; w < n; w += (gridDim.x / kWorkShards) * kBlock) {
    const uint2 item = T.work[shard * cap + w];
    const uint32_t t = item.x, o = item.y & 0x1fffffffu, tests = item.y >> 29;
    const uint32_t ia[3] = {T.tris[3 * t], T.tris[3 * t + 1], T.tris[3 * t + 2]};
    const uint32_t ib = T.tris[3 * o], ic = T.tris[3 * o + 1], idd = T.tris[3 * o + 2];
    const F3 b1 = xyz(pos[ib]), c1 = xyz(pos[ic]), d1 = xyz(pos[idd]);
    const F3 b0 = xyz(prev[ib]), c0 = xyz(prev[ic]), d0 = xyz(prev[idd]);
    uint32_t hits = 0;
    for (int i = 0; i < 3; ++i) {  // (not unrolled: one copy of the CCD)
      if (!(tests >> i & 1u)) continue;
      const F3 p1 = xyz(pos[ia[i]]), p0 = xyz(prev[ia[i]]);
      if (point_triangle_ccd(p0 - b0, c0 - b0, d0 - b0, p1 - b1, c1 - b1, d1 - b1, threshold)) hits |= 1u << i;
    }
    // the hit records: one append per wavefront
    const unsigned long long hot = __ballot(hits != 0u);
    if (hot == 0ull) continue;
    const int leader = __builtin_ctzll(hot);
    uint32_t base = 0;
    if (static_cast<int>(threadIdx.x & 63u) == leader) base = atomicAdd(&T.counters[kTriCtrHitRecords], static_cast<uint32_t>(__popcll(hot)));
    base = __shfl(base, leader, 64);
    if (hits == 0u) continue;
    const int4 rg = T.rng[t];
    const uint32_t shared = volume(meet(insert_box(rg), insert_box(T.rng[o])));  // (a triangle on the work list searched: its range is the listed one)
    atomicAdd(&T.cntTri[merge_rank(t, T.nt, T.threadCount)], static_cast<uint32_t>(__popc(hits)) * shared);
    const uint32_t rec = base + static_cast<uint32_t>(__popcll(hot & ((1ull << (threadIdx.x & 63u)) - 1ull)));
    if (rec < T.maxContacts) T.pool[rec] = make_uint4(t, o, hits, atomicExch(&T.head[t], rec));
    else atomicOr(&T.counters[kTriCtrFailure], kTriFailOverflow);  // more records than contacts fit the list: the list overflows as well
  }
}

void launch_tri_detect(hipStream_t st_, const TriArrays& T, const NodeArrays& nd, const float* kdiag, float* cdiag, float* dinv, float threshold,
                       bool mergedRows, bool levelsInLine) {
  if (T.nt == 0) return;
  const dim3 blk(kBlock);
  hipLaunchKernelGGL(k_tri_box, grid_for(T.nt), blk, 0, st_, T, nd.pos, nd.prev);
  hipLaunchKernelGGL(k_tri_starts, dim3(T.slots / kGridTile), blk, 0, st_, T);
  hipLaunchKernelGGL(k_tri_fill, grid_for(T.nt), blk, 0, st_, T);
  int team = kTriTeam;  // PIES_TRI_TEAM: lanes per triangle in k_tri_pairs (8, 16, 32; speed only)
  if (const char* e = tuning_env("PIES_TRI_TEAM")) team = std::atoi(e);
  if (team == 8) hipLaunchKernelGGL((k_tri_pairs<8>), grid_for(T.nt * 8), blk, 0, st_, T, nd.pos, nd.prev, threshold);
  else if (team == 32) hipLaunchKernelGGL((k_tri_pairs<32>), grid_for(T.nt * 32), blk, 0, st_, T, nd.pos, nd.prev, threshold);
  else hipLaunchKernelGGL((k_tri_pairs<kTriTeam>), grid_for(T.nt * kTriTeam), blk, 0, st_, T, nd.pos, nd.prev, threshold);
  hipLaunchKernelGGL(k_tri_ccd, dim3(1024), blk, 0, st_, T, nd.pos, nd.prev, threshold);  // (a multiple of kWorkShards)
  launch_tri_lists(st_, T, nd, kdiag, cdiag, dinv, mergedRows, levelsInLine);
}

}  // namespace pies
