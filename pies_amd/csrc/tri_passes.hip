// Point-triangle contacts of the Projective-Dynamics substep, third stage: what runs over the finished contact list
// (tri_lists.hip).  The contacts' local step (CollisionConstraint.cpp:86-124, 176-194) and the sequential parts - stabilisation
// (Solver.cpp:367-383 via CollisionConstraint.cpp:126-162) and friction (Solver.cpp:431-471) - which are order dependent
// Gauss-Seidel passes over the list.  They run level by level of the list's dependency DAG (two contacts conflict when they share
// a node; k_tri_levels) - the sequential result - on an LDS copy of the touched nodes when these fit, through L2 otherwise; lists
// with more than kTriMaxLevels levels are walked by one wavefront, 64 contacts at a time.
#include <algorithm>
#include <cstdint>

#include "floor_friction.h"
#include "tri_device.h"

namespace pies {

constexpr int kBlock = 256;

__global__ void __launch_bounds__(kBlock) k_pd_local_tri(TriArrays T, const float4* __restrict__ pos, float thickness) {
  tri_local_contacts(T, pos, thickness, blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock);
}

// ---- sequential passes over the contact list ---------------------------------------------------------------
PIES_DEV float ld(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
PIES_DEV void st(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
PIES_DEV F3 ld3(const float* base, uint32_t node) { return {ld(base + 4 * node), ld(base + 4 * node + 1), ld(base + 4 * node + 2)}; }
PIES_DEV void st3(float* base, uint32_t node, F3 v) { st(base + 4 * node, v.x); st(base + 4 * node + 1, v.y); st(base + 4 * node + 2, v.z); }

// The node state of a pass is reached through an accessor (L2 or the workgroup's LDS copy): im(k), pos(k), set_pos(k, v),
// second(k) / set_second(k, v) = the previous position (stabilisation) or the velocity (friction) of the node with key k;
// key(u, n) = the key of the list's u-th node n.
// node state in L2 (agent-scope loads and stores), by node index
struct GlobalNodes {
  float *p, *q;
  static PIES_DEV uint32_t key(uint32_t, uint32_t n) { return n; }
  PIES_DEV float im(uint32_t k) const { return ld(p + 4 * k + 3); }
  PIES_DEV F3 pos(uint32_t k) const { return ld3(p, k); }
  PIES_DEV void set_pos(uint32_t k, F3 v) const { st3(p, k, v); }
  PIES_DEV F3 second(uint32_t k) const { return ld3(q, k); }
  PIES_DEV void set_second(uint32_t k, F3 v) const { st3(q, k, v); }
};
// node state in the workgroup's LDS copy (records of four floats; the fourth of P is the inverse mass), by place in usedNodes
struct LdsNodes {
  float4 *P, *Q;
  static PIES_DEV uint32_t key(uint32_t u, uint32_t) { return u; }
  PIES_DEV float im(uint32_t k) const { return P[k].w; }
  PIES_DEV F3 pos(uint32_t k) const { const float4 v = P[k]; return {v.x, v.y, v.z}; }
  PIES_DEV void set_pos(uint32_t k, F3 v) const { float4& d = P[k]; d.x = v.x; d.y = v.y; d.z = v.z; }
  PIES_DEV F3 second(uint32_t k) const { const float4 v = Q[k]; return {v.x, v.y, v.z}; }
  PIES_DEV void set_second(uint32_t k, F3 v) const { float4& d = Q[k]; d.x = v.x; d.y = v.y; d.z = v.z; }
};
struct PassConstants { float thickness, friction, staticThreshold; };

// One contact of a sequential pass.  MODE 0: PointTriangleCollisionConstraint::stabilizeCollisions
// (CollisionConstraint.cpp:126-162); MODE 1: point-triangle friction (Solver.cpp:431-471).  k: the keys of the contact's
// point and of the three nodes of its triangle.
template <int MODE, class IO>
PIES_DEV void tri_contact_step(const IO& io, const uint4 k, const PassConstants& c) {
  const float imA = io.im(k.x), imB = io.im(k.y), imC = io.im(k.z), imD = io.im(k.w);
  const F3 pa = io.pos(k.x), pb = io.pos(k.y), pc = io.pos(k.z), pd = io.pos(k.w);
  const F3 n = normalize(cross(pc - pb, pd - pb));
  const float wTri = imB + imC + imD, wSum = imA + wTri;
  if (MODE == 0) {
    const float nDotP = dot(n, pa - pb);
    if (nDotP < c.thickness) {
      const F3 disp = (c.thickness - nDotP) * n;
      const F3 da = disp * imA / wSum, dt = disp * wTri / wSum;
      io.set_pos(k.x, pa + da); io.set_pos(k.y, pb - dt); io.set_pos(k.z, pc - dt); io.set_pos(k.w, pd - dt);
      io.set_second(k.x, io.second(k.x) + da); io.set_second(k.y, io.second(k.y) - dt);
      io.set_second(k.z, io.second(k.z) - dt); io.set_second(k.w, io.second(k.w) - dt);
    }
  } else {
    const F3 va = io.second(k.x), vb = io.second(k.y), vc = io.second(k.z), vd = io.second(k.w);
    const F3 avg = (vb + vc + vd) / 3.0f;
    const F3 rel = va - avg;
    const float vDotN = dot(rel, n);
    const F3 perp = rel - vDotN * n;
    float fr = c.friction;
    if (sqrtf(dot(perp, perp)) < c.staticThreshold) fr = 1.0f;
    const F3 dv = (-fr) * perp - (1.1f * fminf(vDotN, 0.0f)) * n;
    const F3 ndv = neg(dv);
    io.set_second(k.x, va + dv * imA / wSum);
    io.set_second(k.y, vb + ndv * wTri / wSum);
    io.set_second(k.z, vc + ndv * wTri / wSum);
    io.set_second(k.w, vd + ndv * wTri / wSum);
  }
}
// The three things a pass is made of, each over an accessor, the lanes' stride and - what ends a level - close().
// The contacts first, first + stride, ... of a level (they share no node); keys(q) = the keys of the level's q-th contact.
template <int MODE, class IO, class Keys, class Close>
PIES_DEV void level_contacts(const IO& io, uint32_t first, uint32_t end, uint32_t stride, Keys keys, Close close, const PassConstants& c) {
  for (uint32_t q = first; q < end; q += stride) tri_contact_step<MODE>(io, keys(q), c);
  close();
}
// Between two stabilisation iterations: the floor snap of the list's nodes (to where the right-hand side kernel left their target).
template <class IO, class Close>
PIES_DEV void snap_list_nodes(const TriArrays& T, const IO& io, uint32_t used, uint32_t first, uint32_t stride, const uint32_t* __restrict__ nstatic,
                              const float4* __restrict__ statp, Close close) {
  for (uint32_t u = first; u < used; u += stride) {
    const uint32_t n = T.usedNodes[u];
    if (nstatic[n]) io.set_pos(IO::key(u, n), xyz(statp[n]));
  }
  close();
}
// After the contacts' friction: the floor friction of the list's nodes.
template <class IO>
PIES_DEV void list_floor_friction(const TriArrays& T, const IO& io, uint32_t used, uint32_t first, uint32_t stride, const uint32_t* __restrict__ nstatic,
                                  const PassConstants& c) {
  for (uint32_t u = first; u < used; u += stride) {
    const uint32_t n = T.usedNodes[u];
    const uint32_t ns = nstatic[n];
    if (ns == 0u) continue;
    F3 v = io.second(IO::key(u, n));
    floor_friction(v.x, v.y, v.z, ns, c.friction, c.staticThreshold);
    io.set_second(IO::key(u, n), v);
  }
}

// A sequential pass over the contact list (stabilisation or friction), level by level: the contacts of a level share no
// node.  Three forms, chosen by k_tri_levels (counters[kTriCtrPassForm]):
//  kTriPassLds   the touched nodes (at most kSeqLdsNodes) are copied into LDS, the levels run on the copy with a barrier that waits
//     for LDS traffic only, the copy is written back at the end.  A level costs its arithmetic and one LDS round trip
//     (0.43 us: the dependent chain cross product - square root - division - dot product - divisions of one contact)
//     instead of one or two L2 round trips on top of it (0.75 us stabilisation, 2.0 us friction on a 29k-contact patch);
//     four wavefronts work (levels are 20-110 contacts wide), the other twelve help with the copy and leave.  The
//     contacts' node slots are staged through LDS kSeqChunk at a time.  (Measured and dropped: four lanes per contact,
//     one vector component each over DPP quad permutes - bit-identical, less than half the instructions, the same
//     270 us per pass: a level waits for latencies, not for issue slots; one working wavefront without barriers: slower,
//     levels wider than 64 contacts take two rounds.)
//  kTriPassL2    node state through agent-scope (L2) loads and stores, a level ends with the stores drained and a workgroup barrier.
//  kTriPassWalk  more levels than kTriMaxLevels: one wavefront walks the list window by window; a level of a window ends with
//     the stores drained.
#ifndef PIES_SEQ_WORKERS
#define PIES_SEQ_WORKERS 256
#endif
constexpr int kSeqWorkers = PIES_SEQ_WORKERS;
constexpr uint32_t kSeqChunk = 2048;
// between two levels: with one working wavefront its LDS operations are already in order; with several, a barrier
PIES_DEV void level_barrier() {
  if (kSeqWorkers > 64) lds_barrier();
  else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// The passes through L2: WALK = false level by level with the whole workgroup, WALK = true window by window with one wavefront.
// The two differ in how a level's contacts are found and in what ends a level.
template <int MODE, bool WALK>
PIES_DEV void passes_through_l2(const TriArrays& T, const GlobalNodes& io, uint32_t M, uint32_t used, uint32_t tid, const uint32_t* __restrict__ nstatic,
                                const float4* __restrict__ statp, uint32_t iterations, bool snap, bool floorFr, const PassConstants& c) {
  constexpr uint32_t stride = WALK ? 64u : static_cast<uint32_t>(kSeqBlock);
  if (WALK && tid >= stride) return;
  auto close = [] {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!WALK) __syncthreads();
  };
  for (uint32_t it = 0; it < iterations; ++it) {
    if (WALK) {
      for (uint32_t base = 0; base < M; base += 64) {
        const bool valid = base + tid < M;
        const uint4 id = valid ? T.ids[base + tid] : make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
        int maxLevel;
        const int level = window_levels(valid, id, static_cast<int>(tid), maxLevel);
        for (int lv = 0; lv <= maxLevel; ++lv)  // (this lane's contact, when it is of the level)
          level_contacts<MODE>(io, valid && level == lv ? 0u : 1u, 1u, 1u, [&](uint32_t) { return id; }, close, c);
      }
    } else {
      const uint32_t levels = T.counters[kTriCtrLevels];
      for (uint32_t lv = 0; lv < levels; ++lv)
        level_contacts<MODE>(io, T.lvStart[lv] + tid, T.lvStart[lv + 1], stride, [&](uint32_t q) { return T.ids[T.lvOrder[q]]; }, close, c);
    }
    if (snap) snap_list_nodes(T, io, used, tid, stride, nstatic, statp, close);
  }
  if (floorFr) list_floor_friction(T, io, used, tid, stride, nstatic, c);
}
// MODE 0 runs ALL the stabilisation iterations of the substep (Solver.cpp:367-383: every iteration is a pass over the contacts
// followed by the floor snap of every node with a floor contact): the snap of a node puts it where the right-hand side kernel
// left its target (statp) and is idempotent, and a pass only touches the nodes of the list (usedNodes) - so the snap of those
// nodes runs here, between the passes, and the snap of all the others once, in k_pd_stabilize behind this kernel.  (Until
// round 3 the host launched pass and snap `iterations` times: eight launches of ~4.7 us in a substep without a single contact.)
// MODE 1 (friction) ends with the floor friction of the list's nodes, which the reference applies after the contacts' friction;
// k_pd_velocity, before this kernel, has applied it to every node that is in no contact (usedBits).
template <int MODE>
__global__ void __launch_bounds__(kSeqBlock) k_tri_sequential(TriArrays T, float4* pos4, float4* prev4, float4* vel4, float thickness,
                                                              float friction, float staticThreshold, const uint32_t* __restrict__ nstatic,
                                                              const float4* __restrict__ statp, uint32_t iterations) {
  __shared__ float4 P[kSeqLdsNodes], Q[kSeqLdsNodes];
  __shared__ uint2 sSlots[kSeqChunk];
  __shared__ uint32_t sLv[kTriMaxLevels + 1];
  const uint32_t tid = threadIdx.x;
  const uint32_t M = T.counters[kTriCtrContacts];
  if (M == 0) return;
  const uint32_t form = T.counters[kTriCtrPassForm], used = T.counters[kTriCtrUsedNodes];
  const bool snap = MODE == 0 && nstatic != nullptr, floorFr = MODE == 1 && nstatic != nullptr;
  const PassConstants c = {thickness, friction, staticThreshold};
  float4* second4 = MODE == 0 ? prev4 : vel4;
  if (form != kTriPassLds) {
    const GlobalNodes io = {reinterpret_cast<float*>(pos4), reinterpret_cast<float*>(second4)};
    if (form == kTriPassWalk) passes_through_l2<MODE, true>(T, io, M, used, tid, nstatic, statp, iterations, snap, floorFr, c);
    else passes_through_l2<MODE, false>(T, io, M, used, tid, nstatic, statp, iterations, snap, floorFr, c);
    return;
  }
  const uint32_t levels = T.counters[kTriCtrLevels];
  for (uint32_t u = tid; u < used; u += kSeqBlock) {
    const uint32_t n = T.usedNodes[u];
    P[u] = pos4[n];
    Q[u] = second4[n];
  }
  for (uint32_t l = tid; l <= levels; l += kSeqBlock) sLv[l] = T.lvStart[l];
  __syncthreads();
  if (tid >= kSeqWorkers) return;  // (a wavefront that has ended no longer counts at the barrier)
  const LdsNodes io = {P, Q};
  auto close = [] { level_barrier(); };
  uint32_t k0 = 0, kEnd = 0;
  for (uint32_t it = 0; it < iterations; ++it) {
    if (M > kSeqChunk) k0 = kEnd = 0;  // (a list that fits one chunk stays staged)
    for (uint32_t lv = 0; lv < levels; ++lv) {
      const uint32_t lo = sLv[lv], hi = sLv[lv + 1];
      uint32_t seg = lo;
      while (seg < hi) {
        if (min(hi, seg + kSeqChunk) > kEnd) {  // stage the node slots of the next kSeqChunk contacts
          k0 = seg;
          kEnd = min(M, seg + kSeqChunk);
          for (uint32_t q = k0 + tid; q < kEnd; q += kSeqWorkers) sSlots[q - k0] = T.lvSlots[q];
          level_barrier();
        }
        const uint32_t segEnd = min(hi, kEnd);
        level_contacts<MODE>(io, seg + tid, segEnd, kSeqWorkers, [&](uint32_t q) {
          const uint2 sl = sSlots[q - k0];
          return make_uint4(sl.x & 0xffffu, sl.x >> 16, sl.y & 0xffffu, sl.y >> 16);
        }, close, c);
        seg = segEnd;
      }
    }
    if (snap) snap_list_nodes(T, io, used, tid, kSeqWorkers, nstatic, statp, close);
  }
  if (floorFr) list_floor_friction(T, io, used, tid, kSeqWorkers, nstatic, c);  // (a lane's own nodes: no barrier before the copy leaves)
  for (uint32_t u = tid; u < used; u += kSeqWorkers) {
    const uint32_t n = T.usedNodes[u];
    if (MODE == 0) pos4[n] = P[u];
    second4[n] = Q[u];
  }
}

void launch_pd_local_tri(hipStream_t st_, const TriArrays& T, const float4* pos, float thickness) {
  if (T.nt == 0) return;
  const dim3 cgrid(std::min<uint32_t>(256u, (T.maxContacts + kBlock - 1) / kBlock));
  hipLaunchKernelGGL(k_pd_local_tri, cgrid, dim3(kBlock), 0, st_, T, pos, thickness);
}
void launch_tri_stabilize(hipStream_t st_, const TriArrays& T, const NodeArrays& nd, float thickness, const uint32_t* nstatic, const float4* statp,
                          uint32_t iterations) {
  if (T.nt == 0 || iterations == 0) return;
  hipLaunchKernelGGL(k_tri_sequential<0>, dim3(1), dim3(kSeqBlock), 0, st_, T, nd.pos, nd.prev, nd.vel, thickness, 0.0f, 0.0f, nstatic, statp, iterations);
}
void launch_tri_friction(hipStream_t st_, const TriArrays& T, const NodeArrays& nd, float friction, float staticThreshold, const uint32_t* nstatic) {
  if (T.nt == 0) return;
  hipLaunchKernelGGL(k_tri_sequential<1>, dim3(1), dim3(kSeqBlock), 0, st_, T, nd.pos, nd.prev, nd.vel, 0.0f, friction, staticThreshold, nstatic,
                     static_cast<const float4*>(nullptr), 1u);
}

}  // namespace pies
