// Node-node resolve on the node grid (grid_build.hip) in the two orders that walk the grid's buckets cell by cell (reference:
// Src/Solver.cpp:81-130, Include/Pies/SpatialHash.h:101-127).  The orders by dependency levels (pair_*.hip) fall back on them.
//  * k_collide_reference - the reference's loop as it stands (Solver.cpp:85-130): nodes 0..N-1 in ascending index, each
//    querying the cell range of its CURRENT position (SpatialHash.h:101-127), buckets in dx,dy,dz order, every overlapping
//    pair resolved at once (positions and velocities of both nodes, the self pair included).  The loop is one dependent
//    chain, so it runs on one wavefront: 64 candidates are tested at a time and hits are resolved one by one in bucket
//    order, re-testing the rest after each resolve because the visiting node has moved.  Bit-identical to the loop; slow.
//  * k_collide_flow / k_collide - a documented order that exposes parallelism (DESIGN.md "Node-node collisions"): nodes are
//    grouped by the minimum cell of their range; groups whose minimum cells agree modulo 3 on every axis touch disjoint node
//    sets (needs ranges of at most 2 cells per axis), so the 27 residue classes are 27 passes; inside a pass one
//    wavefront owns one group and visits its nodes in ascending index, each with the range it was inserted with.
// Each step exists once: the walk over one bucket (walk_bucket, over an accessor that says where the candidates' state lives),
// a node's load and store per storage (global memory, the LDS table of a staged group), the kernels' prologue and their
// statistics.  The per-pair arithmetic is the reference's, operation for operation: visit_wide (pair_rule.h).
#include <climits>
#include <cstdint>
#include <cstdlib>

#include "cell_table.h"
#include "hash_kernels.h"
#include "hash_device.h"
#include "pair_rule.h"

namespace pies {

// ---- node state in global memory ------------------------------------------------------------------------------------
// The unstaged path reads and writes node state through agent-scope relaxed atomics (L2-served, write-through): within a
// pass exactly one wavefront touches a given node, and that wavefront must see its own earlier writes.  (The staged path
// moves whole records with ordinary 16-byte loads and stores between the acquire fence behind the wait and the release
// store of the completion stamp, group_resolve.)
PIES_DEV float ld(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
PIES_DEV void st(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
struct GlobalNodes {
  float *pos, *vel;  // four words per node
  const float* __restrict__ radius;
};
PIES_DEV NodeState load_node(const GlobalNodes& G, uint32_t j) {
  return NodeState{ld(G.pos + 4 * j), ld(G.pos + 4 * j + 1), ld(G.pos + 4 * j + 2), ld(G.pos + 4 * j + 3),
                   ld(G.vel + 4 * j), ld(G.vel + 4 * j + 1), ld(G.vel + 4 * j + 2), G.radius[j]};
}
PIES_DEV void store_node(const GlobalNodes& G, uint32_t j, const NodeState& s) {  // (a resolve moves position and velocity only)
  st(G.pos + 4 * j, s.px); st(G.pos + 4 * j + 1, s.py); st(G.pos + 4 * j + 2, s.pz);
  st(G.vel + 4 * j, s.vx); st(G.vel + 4 * j + 1, s.vy); st(G.vel + 4 * j + 2, s.vz);
}
PIES_DEV void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }  // this wave's stores are in L2 before its next loads

// ---- node state in the LDS table of a staged group ---------------------------------------------------------------------
// All nodes of a group share their minimum cell, so everything they can touch lies in the 2x2x2 cells above it: the distinct
// nodes of those buckets (typically ~100) are fetched ONCE into a wave-private LDS table (open addressing on the node index),
// the visiting order of collide_group_global is replayed on the LDS copies, and the touched nodes are written back at the end.
// Same arithmetic, same order.
#ifndef PIES_COL_BLOCK
#define PIES_COL_BLOCK 128
#endif
constexpr int kColBlock = PIES_COL_BLOCK;            // wavefronts of a block, each with its own table
#ifndef PIES_COL_SLOTS
#define PIES_COL_SLOTS 512
#endif
constexpr uint32_t kColSlots = PIES_COL_SLOTS;       // table capacity per wavefront (power of two)
#ifndef PIES_COL_MAX_UNIQUE
#define PIES_COL_MAX_UNIQUE 384
#endif
constexpr uint32_t kColMaxUnique = PIES_COL_MAX_UNIQUE;   // live entries allowed: an interior group of BASELINE config 4 (spacing 0.9, cells of 2.0) sees 216-343 distinct nodes
constexpr uint32_t kColMaxEntries = 1024; // bucket entries of the 8 cells
constexpr uint32_t kColEmpty = 0xffffffffu, kColDirty = 0x80000000u;
constexpr uint32_t kColMaxSpins = 1u << 22;  // default polls of one completion stamp before the wait is declared dead (~5 s);
                                             // PIES_COLLIDE_SPIN_LIMIT overrides it (0 = wait for ever; PIES_PROFILER_SAFE=1 implies 0:
                                             // counter collection serialises and slows the launch)
struct ColTable {
  uint32_t key[kColSlots];  // node index | kColDirty
  float px[kColSlots], py[kColSlots], pz[kColSlots], im[kColSlots], vx[kColSlots], vy[kColSlots], vz[kColSlots], r[kColSlots];
  uint16_t ent[kColMaxEntries];  // table slot of every bucket entry, cell after cell
};
constexpr int kColSlotBits = kColSlots == 256 ? 8 : kColSlots == 512 ? 9 : kColSlots == 1024 ? 10 : 11;
static_assert((1u << kColSlotBits) == kColSlots, "kColSlots must be 256, 512, 1024 or 2048");
PIES_DEV uint32_t col_hash(uint32_t j) { return (j * 2654435761u) >> (32 - kColSlotBits); }
PIES_DEV uint32_t col_find(const uint32_t* key, uint32_t j) {  // j is present
  uint32_t h = col_hash(j);
  while ((key[h] & ~kColDirty) != j) h = (h + 1) & (kColSlots - 1);
  return h;
}
PIES_DEV NodeState load_node(const ColTable& T, uint32_t s) {
  return NodeState{T.px[s], T.py[s], T.pz[s], T.im[s], T.vx[s], T.vy[s], T.vz[s], T.r[s]};
}
PIES_DEV void store_node(ColTable& T, uint32_t s, uint32_t j, const NodeState& n) {  // slot s holds node j: moved, to be written back
  T.px[s] = n.px; T.py[s] = n.py; T.pz[s] = n.pz;
  T.vx[s] = n.vx; T.vy[s] = n.vy; T.vz[s] = n.vz;
  T.key[s] = j | kColDirty;
}

// ---- one bucket ----------------------------------------------------------------------------------------------------
// Where the candidates of a bucket live.  load(e, c, at): node index and state of entry e, `at` = where a result goes;
// store(at, j, o): the new state of candidate j, from one lane; flush(): behind each batch of 64 entries.
struct GlobalBucket {  // entries [bs, ..) of the sorted list, state straight from global memory
  const GlobalNodes& G;
  const uint32_t* __restrict__ val;
  uint32_t bs;
  PIES_DEV uint32_t load(uint32_t e, NodeState& c, uint32_t& at) const {
    at = val[bs + e] & kNodeMask;
    c = load_node(G, at);  // candidate state up front: a resolve then needs no further loads
    return at;
  }
  PIES_DEV void store(uint32_t at, uint32_t, const NodeState& o) const { store_node(G, at, o); }
  PIES_DEV void flush() const { drain_stores(); }
};
struct StagedBucket {  // entries [off, ..) of the table's entry list, state in the table
  ColTable& T;
  uint32_t off;
  PIES_DEV uint32_t load(uint32_t e, NodeState& c, uint32_t& at) const {
    at = T.ent[off + e];
    c = load_node(T, at);
    return T.key[at] & ~kColDirty;
  }
  PIES_DEV void store(uint32_t at, uint32_t j, const NodeState& o) const { store_node(T, at, j, o); }
  PIES_DEV void flush() const {}
};
// One bucket of bc entries met by visiting node i, whose state `a` lives in registers (wave uniform): 64 candidates are tested
// at a time, hits are resolved one by one in bucket order and the rest re-tested (the visiting node has moved).  Returns the
// number of resolved pairs.
template <class Bucket>
PIES_DEV uint32_t walk_bucket(const Bucket& C, uint32_t bc, uint32_t i, NodeState& a, int lane, float friction, float staticThreshold,
                              uint32_t& tested) {
  uint32_t resolved = 0;
  tested += bc;  // statistics: candidates this visit looks at (SURVEY 8d counts 16 B per candidate neighbour)
  for (uint32_t base = 0; base < bc; base += 64) {
    const bool valid = base + lane < bc;
    NodeState c = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f};
    uint32_t at = 0;
    const uint32_t j = valid ? C.load(base + lane, c, at) : 0xffffffffu;
    int cursor = 0;
    for (;;) {
      if (valid && j == i) { c.px = a.px; c.py = a.py; c.pz = a.pz; }  // the self pair sees the node's current position
      const float ddx = c.px - a.px, ddy = c.py - a.py, ddz = c.pz - a.pz;
      const float dist = sqrtf(ddx * ddx + ddy * ddy + ddz * ddz);
      const float disp = a.r + c.r - dist;
      const bool hit = valid && lane >= cursor && disp > 0.0f;
      const unsigned long long m = __ballot(hit);
      if (m == 0ull) break;
      const int l = __builtin_ctzll(m);
      const uint32_t hj = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(j), l));
      const bool self = hj == i;
      NodeState o = self ? a : lane_node(c, static_cast<uint32_t>(l));  // (the node meeting itself, quirk Q3: folded into a)
      visit_wide(a, o, self, friction, staticThreshold, lane);
      if (!self && lane == l) C.store(at, j, o);
      ++resolved;
      cursor = l + 1;
    }
    C.flush();
  }
  return resolved;
}

// ---- one group ---------------------------------------------------------------------------------------------------------
// The nodes of a group are the entries of its own cell's bucket that carry kMinFlag (ascending node index, like the
// bucket).  Returns the bucket-relative position of the next one at or after `from`, or cnt.
PIES_DEV uint32_t next_min_entry(const uint32_t* __restrict__ val, uint32_t start, uint32_t cnt, uint32_t from, int lane) {
  for (uint32_t base = from & ~63u; base < cnt; base += 64) {
    const uint32_t e = base + static_cast<uint32_t>(lane);
    const bool f = e < cnt && e >= from && (val[start + e] & kMinFlag) != 0u;
    const unsigned long long m = __ballot(f);
    if (m) return base + static_cast<uint32_t>(__builtin_ctzll(m));
  }
  return cnt;
}

// what a resolve kernel's wavefront works with (wave uniform but for the lane)
struct ResolveCtx {
  GlobalNodes G;
  int lane;
  GridBox B;
  const uint32_t* __restrict__ val;  // the sorted entries' values
  float friction, staticThreshold;
};
PIES_DEV ResolveCtx resolve_begin(const HashArrays& H, float4* pos4, float4* vel4, const float* __restrict__ radius, float friction,
                                  float staticThreshold) {
  ResolveCtx X;
  X.G = GlobalNodes{reinterpret_cast<float*>(pos4), reinterpret_cast<float*>(vel4), radius};
  X.lane = threadIdx.x & 63;
  X.B = grid_box(H.counters);
  X.val = H.val[grid_passes(X.B) & 1u];
  X.friction = friction;
  X.staticThreshold = staticThreshold;
  return X;
}
// a wavefront's statistics, one atomic per wave at the end (a per-pair atomic on one word serialises the chip)
PIES_DEV void count_pass(const HashArrays& H, uint32_t resolved, uint32_t tested, int lane) {
  if (lane == 0 && resolved) atomicAdd(&H.counters[kCounterPairs], resolved);
  if (lane == 0 && tested) atomicAdd(reinterpret_cast<unsigned long long*>(&H.counters[kCounterCandidates]), static_cast<unsigned long long>(tested));
}

// Resolve of one group straight from global memory: every candidate's state is fetched again for every visiting
// node.  Only used for groups whose neighbourhood does not fit the LDS staging of k_collide (dense pile-ups).
PIES_DEV uint32_t collide_group_global(const HashArrays& H, const ResolveCtx& X, uint32_t gslot, uint32_t& tested) {
  uint32_t resolved = 0;
  const uint32_t gs = H.start[gslot], gn = H.end[gslot] - gs;
  for (uint32_t ge = next_min_entry(X.val, gs, gn, 0, X.lane); ge < gn; ge = next_min_entry(X.val, gs, gn, ge + 1, X.lane)) {
    const uint32_t i = X.val[gs + ge] & kNodeMask;
    NodeState a = load_node(X.G, i);
    const int4 rg = H.rng[i];
    const uint32_t lx = rg.w & 0xff, ly = (rg.w >> 8) & 0xff, lz = (rg.w >> 16) & 0xff;
    for (uint32_t dx = 0; dx < lx; ++dx)
      for (uint32_t dy = 0; dy < ly; ++dy)
        for (uint32_t dz = 0; dz < lz; ++dz) {
          const uint32_t cs = find_bucket(H, X.B, rg.x + (int)dx, rg.y + (int)dy, rg.z + (int)dz);
          if (cs == 0xffffffffu) continue;
          const uint32_t bs = H.start[cs];
          resolved += walk_bucket(GlobalBucket{X.G, X.val, bs}, H.end[cs] - bs, i, a, X.lane, X.friction, X.staticThreshold, tested);
        }
    if (X.lane == 0) store_node(X.G, i, a);
    drain_stores();
  }
  return resolved;
}

// One group on the staged path (or, for a dense neighbourhood, the unstaged one), in two halves.
//  * group_prepare reads only what the grid build left behind (buckets, entries, ranges): the group's eight buckets, the
//    table of distinct nodes, the table slot of every bucket entry, and - in registers, one own-cell entry per lane - the
//    group's own nodes with their ranges and slots.  k_collide_flow runs it BEFORE it waits for the conflicting groups of
//    earlier passes, so this half (about a quarter of a group's time) is off the chain of the 27 passes.
//  * group_resolve loads the node state, replays the visiting order of collide_group_global on the copies and writes the
//    touched nodes back.  Node state is read and written through agent-scope (sc1) loads and stores: in k_collide_flow the
//    previous owner of a node may be a wavefront of the same launch on another XCD.  Returns the number of resolved pairs.
struct GroupPlan {
  uint32_t cStart[8], cCnt[8], cOff[9];  // the 2x2x2 buckets above the group's cell (wave uniform)
  bool empty, staged, ownInLanes;
  uint32_t ownVal, ownRng, ownSlot;      // lane e: entry e of the own cell (cell 0), its range word and table slot
};
PIES_DEV void group_prepare(const HashArrays& H, const GridBox& B, const uint32_t* __restrict__ val, ColTable& T, uint32_t gslot, int lane,
                            int forceGlobal, GroupPlan& P) {
  P.empty = H.gcnt[gslot] == 0;
  P.staged = false;
  P.ownInLanes = false;
  P.ownVal = P.ownRng = P.ownSlot = 0;
  if (P.empty) return;
  // ---- the 2x2x2 cells above the group's cell: lanes 0..7 look one up each ------------------------------
  int gx, gy, gz;
  box_cell(B, H.keys[gslot], gx, gy, gz);
  uint32_t myStart = 0, myCnt = 0;
  if (lane < 8) {
    const uint32_t cs = find_bucket(H, B, gx + ((lane >> 2) & 1), gy + ((lane >> 1) & 1), gz + (lane & 1));
    if (cs != 0xffffffffu) { myStart = H.start[cs]; myCnt = H.end[cs] - myStart; }
  }
  P.cOff[0] = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    P.cStart[c] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(myStart), c));
    P.cCnt[c] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(myCnt), c));
    P.cOff[c + 1] = P.cOff[c] + P.cCnt[c];
  }
  bool staged = !forceGlobal && P.cOff[8] <= kColMaxEntries;
  if (staged) {
    for (uint32_t t = lane; t < kColSlots; t += 64) T.key[t] = kColEmpty;
    uint32_t unique = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      for (uint32_t base = 0; base < P.cCnt[c] && staged; base += 64) {
        bool fresh = false;
        if (base + lane < P.cCnt[c]) {
          const uint32_t v = val[P.cStart[c] + base + lane];
          const uint32_t j = v & kNodeMask;
          uint32_t h = col_hash(j);
          for (;;) {  // at most kColMaxUnique + 64 live entries: the probe ends
            const uint32_t old = atomicCAS(&T.key[h], kColEmpty, j);
            if (old == kColEmpty) { fresh = true; break; }
            if (old == j) break;
            h = (h + 1) & (kColSlots - 1);
          }
          T.ent[P.cOff[c] + base + lane] = static_cast<uint16_t>(h);
          if (c == 0 && base == 0) {  // the own cell's first 64 entries stay in the lanes
            P.ownVal = v;
            P.ownSlot = h;
            if (v & kMinFlag) P.ownRng = static_cast<uint32_t>(H.rng[j].w);
          }
        }
        unique += static_cast<uint32_t>(__popcll(__ballot(fresh)));
        if (unique > kColMaxUnique) staged = false;
      }
    }
  }
  P.staged = staged;
  P.ownInLanes = staged && P.cCnt[0] <= 64u;
}
PIES_DEV uint32_t group_resolve(const HashArrays& H, const ResolveCtx& X, ColTable& T, uint32_t gslot, const GroupPlan& P, uint32_t& tested) {
  uint32_t resolved = 0;
  if (P.empty) return 0;
  if (!P.staged) return collide_group_global(H, X, gslot, tested);
  const int lane = X.lane;
  const uint32_t* cStart = P.cStart;
  const uint32_t* cCnt = P.cCnt;
  const uint32_t* cOff = P.cOff;
  // Node records as two 16-byte loads (and stores, below).  Coherence with the wavefronts that owned these nodes earlier
  // in the launch, possibly on another XCD, is the memory model's: the caller's acquire fence at agent scope after the
  // wait orders these loads behind the predecessors' stores, which their release store of the completion stamp published
  // (round 1 read and wrote eight relaxed agent-scope dwords per node instead).
  const float4* pos4 = reinterpret_cast<const float4*>(X.G.pos);
  const float4* vel4 = reinterpret_cast<const float4*>(X.G.vel);
  for (uint32_t t = lane; t < kColSlots; t += 64) {
    const uint32_t j = T.key[t];
    if (j == kColEmpty) continue;
    const float4 pj = pos4[j], vj = vel4[j];
    T.px[t] = pj.x; T.py[t] = pj.y; T.pz[t] = pj.z; T.im[t] = pj.w;
    T.vx[t] = vj.x; T.vy[t] = vj.y; T.vz[t] = vj.z;
    T.r[t] = X.G.radius[j];
  }
  // ---- the visiting order of collide_group_global on the staged copies -----------------------------------
  // (the group's own cell is cell 0 of the eight)
  // the group's own nodes in ascending entry order: from the lanes when the own cell has at most 64 entries (no global
  // load and no table probe per node), otherwise looked up one by one
  unsigned long long own = P.ownInLanes ? __ballot(static_cast<uint32_t>(lane) < cCnt[0] && (P.ownVal & kMinFlag) != 0u) : 0ull;
  for (uint32_t ge = P.ownInLanes ? (own ? static_cast<uint32_t>(__builtin_ctzll(own)) : cCnt[0]) : next_min_entry(X.val, cStart[0], cCnt[0], 0, lane);
       ge < cCnt[0];
       ge = P.ownInLanes ? ((own &= own - 1ull) ? static_cast<uint32_t>(__builtin_ctzll(own)) : cCnt[0]) : next_min_entry(X.val, cStart[0], cCnt[0], ge + 1, lane)) {
    uint32_t i, si, rw;
    if (P.ownInLanes) {
      i = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(P.ownVal), static_cast<int>(ge))) & kNodeMask;
      si = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(P.ownSlot), static_cast<int>(ge)));
      rw = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(P.ownRng), static_cast<int>(ge)));
    } else {
      i = X.val[cStart[0] + ge] & kNodeMask;
      si = col_find(T.key, i);
      rw = static_cast<uint32_t>(H.rng[i].w);
    }
    NodeState a = load_node(T, si);
    const uint32_t lx = rw & 0xff, ly = (rw >> 8) & 0xff, lz = (rw >> 16) & 0xff;
    for (uint32_t dx = 0; dx < lx; ++dx)
      for (uint32_t dy = 0; dy < ly; ++dy)
        for (uint32_t dz = 0; dz < lz; ++dz) {
          const uint32_t c = dx * 4 + dy * 2 + dz;
          uint32_t off = 0, bc = 0;
#pragma unroll
          for (int q = 0; q < 8; ++q)
            if (c == static_cast<uint32_t>(q)) { off = cOff[q]; bc = cCnt[q]; }
          resolved += walk_bucket(StagedBucket{T, off}, bc, i, a, lane, X.friction, X.staticThreshold, tested);
        }
    if (lane == 0) store_node(T, si, i, a);
  }
  // ---- write the touched nodes back --------------------------------------------------------------------
  for (uint32_t t = lane; t < kColSlots; t += 64) {
    const uint32_t kj = T.key[t];
    if (kj == kColEmpty || !(kj & kColDirty)) continue;
    const uint32_t j = kj & ~kColDirty;
    reinterpret_cast<float4*>(X.G.pos)[j] = make_float4(T.px[t], T.py[t], T.pz[t], T.im[t]);
    reinterpret_cast<float4*>(X.G.vel)[j] = make_float4(T.vx[t], T.vy[t], T.vz[t], 0.0f);  // (the fourth component of a velocity record is 0 everywhere)
  }
  return resolved;  // (the caller's release store of the completion stamp publishes these stores)
}

// The 27 residue classes as 27 launches: inside a launch no two groups share a node.
__global__ void __launch_bounds__(kColBlock) k_collide(HashArrays H, float4* pos4, float4* vel4, const float* __restrict__ radius,
                                                       uint32_t pass, float friction, float staticThreshold, int forceGlobal) {
  __shared__ ColTable tables[kColBlock / 64];
  ColTable& T = tables[threadIdx.x >> 6];
  if (H.counters[kCounterFlags] || H.counters[kCounterDense]) return;  // failed: the host latches _simFailed; a pile: the sequential loop runs the pass
  const ResolveCtx X = resolve_begin(H, pos4, vel4, radius, friction, staticThreshold);
  const uint32_t wave = (blockIdx.x * kColBlock + threadIdx.x) >> 6, nwaves = (gridDim.x * kColBlock) >> 6;
  const uint32_t ngroups = H.counters[kCounterPass0 + pass];
  uint32_t resolved = 0, tested = 0;
  for (uint32_t g = wave; g < ngroups; g += nwaves) {
    const uint32_t gslot = H.passList[static_cast<size_t>(pass) * H.n + g];
    GroupPlan P;
    group_prepare(H, X.B, X.val, T, gslot, X.lane, forceGlobal, P);
    resolved += group_resolve(H, X, T, gslot, P, tested);
  }
  count_pass(H, resolved, tested, X.lane);
}

// The same order of conflicting groups in ONE launch.  Groups are handed out through a ticket counter in pass-major
// order; before a wavefront touches its group it waits until every group of an earlier pass within two cells (the
// only ones that can share a node with it) has published its completion stamp.  A ticket's predecessors were all
// taken earlier by wavefronts that are resident and running, so the wait always ends; it is bounded anyway and a
// timeout latches the failure flag, which every wait loop polls.  Against the 27 launches this removes the barrier
// after each pass (a pass lasted as long as its slowest group, with ~1.7 wavefronts per SIMD).
PIES_DEV uint32_t ldu(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__global__ void __launch_bounds__(kColBlock) k_collide_flow(HashArrays H, float4* pos4, float4* vel4, const float* __restrict__ radius,
                                                            float friction, float staticThreshold, int forceGlobal, uint32_t maxSpins) {
  __shared__ ColTable tables[kColBlock / 64];
  ColTable& T = tables[threadIdx.x >> 6];
  if (H.counters[kCounterFlags] || H.counters[kCounterDense]) return;
  const ResolveCtx X = resolve_begin(H, pos4, vel4, radius, friction, staticThreshold);
  const int lane = X.lane;
  const uint32_t epoch = H.counters[kCounterEpoch];
  // inclusive prefix of the groups per pass, lane p holding pass p
  uint32_t incl = lane < 27 ? H.counters[kCounterPass0 + lane] : 0u;
#pragma unroll
  for (int off = 1; off < 32; off <<= 1) {
    const uint32_t v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  const uint32_t total = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(incl), 26));
  uint32_t resolved = 0, tested = 0;
  for (;;) {
    uint32_t ticket = 0;
    if (lane == 0) ticket = atomicAdd(&H.counters[kCounterTicket], 1u);
    ticket = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(ticket)));
    if (ticket >= total) break;
    const uint32_t pass = static_cast<uint32_t>(__popcll(__ballot(lane < 27 && incl <= ticket)));
    const uint32_t before = pass ? static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(incl), pass - 1)) : 0u;
    const uint32_t gslot = H.passList[static_cast<size_t>(pass) * H.n + (ticket - before)];
    // ---- what does not depend on the predecessors' results: buckets, table of distinct nodes, own entries ------------
    GroupPlan P;
    group_prepare(H, X.B, X.val, T, gslot, lane, forceGlobal, P);
    // ---- wait for the conflicting groups of earlier passes -------------------------------------------------
    int x, y, z;
    box_cell(X.B, H.keys[gslot], x, y, z);
    bool gaveUp = false;
    for (int q = lane; q < 125; q += 64) {
      const int dx = q % 5 - 2, dy = (q / 5) % 5 - 2, dz = q / 25 - 2;
      if (dx == 0 && dy == 0 && dz == 0) continue;
      const uint32_t other = static_cast<uint32_t>(mod3(x + dx) + 3 * mod3(y + dy) + 9 * mod3(z + dz));
      if (other >= pass) continue;
      const uint32_t os = find_bucket(H, X.B, x + dx, y + dy, z + dz);
      if (os == 0xffffffffu || H.gcnt[os] == 0u) continue;
      uint32_t spins = 0;
      while (ldu(H.done + os) != epoch) {
        __builtin_amdgcn_s_sleep(2);
        if ((++spins & 255u) == 0u && ((maxSpins && spins > maxSpins) || ldu(H.counters + kCounterFlags))) { gaveUp = true; break; }
      }
    }
    if (__ballot(gaveUp)) {  // a predecessor never finished (or the simulation failed elsewhere): latch and leave
      if (lane == 0) atomicOr(&H.counters[kCounterFlags], kFailFlowWait);
      break;
    }
    // the stamps were polled relaxed; this fence orders every later load of the wavefront after them (pairs with the
    // release store below): the predecessors' node writes are visible by the memory model, not by cache behaviour
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    resolved += group_resolve(H, X, T, gslot, P, tested);
    if (lane == 0) __hip_atomic_store(H.done + gslot, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
  count_pass(H, resolved, tested, lane);
}

// The reference's loop as it stands (Solver.cpp:85-130, SpatialHash.h:101-127): nodes in ascending index; a node's
// cell range comes from its position when its turn starts (the node may have been moved by earlier pairs of this
// pass), buckets are those of the grid built at the start of the iteration, visited in dx, dy, dz order.  The loop is
// one dependent chain: one wavefront runs it.  Lanes look up to 64 cells of the range at once.
__global__ void __launch_bounds__(64) k_collide_reference(HashArrays H, float4* pos4, float4* vel4, const float* __restrict__ radius, uint32_t n,
                                                          float scale, float friction, float staticThreshold, const uint32_t* __restrict__ gate,
                                                          unsigned long long budget) {
  if (gate && *gate == 0u) return;        // (the fallback of a parallel order: only when that pass asks for it)
  if (H.counters[kCounterFlags]) return;  // failed: the host latches _simFailed
  if (gate) {
    // What the pass costs here: the sum over the cells of (nodes in the cell)^2 candidate tests, ~15 M of them per second on this one
    // wavefront.  A pile whose pass would take minutes (BASELINE config 2 with the node-node pass on collapses 100 000 nodes into a few
    // cells - quirk Q2 -: 10^10 tests per iteration, hours per tick in the reference as well) is declared failed instead of keeping
    // the device busy for longer than a host waits: the one limit of this build the reference does not have (PIES_FALLBACK_VISITS, 1e9).
    const uint32_t used = H.counters[kCounterUsed];
    unsigned long long est = 0;
    for (uint32_t u = threadIdx.x; u < used; u += 64u) {
      const uint32_t sl = H.used[u];
      const unsigned long long len = H.end[sl] - H.start[sl];
      est += len * len;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) est += __shfl_xor(est, o, 64);
    if (est > budget) {
      if (threadIdx.x == 0) atomicOr(&H.counters[kCounterFlags], kFailBudget);
      return;
    }
  }
  const ResolveCtx X = resolve_begin(H, pos4, vel4, radius, friction, staticThreshold);
  const int lane = X.lane;
  uint32_t resolved = 0, tested = 0;
  for (uint32_t i = 0; i < n; ++i) {
    NodeState a = load_node(X.G, i);
    int mx, my, mz;
    uint32_t lx, ly, lz;
    if (!node_range(a.px, a.py, a.pz, a.r, scale, mx, my, mz, lx, ly, lz)) {
      if (lane == 0) atomicOr(&H.counters[kCounterFlags], kFailNonFinite);
      break;
    }
    const uint32_t ncell = lx * ly * lz;
    for (uint32_t cbase = 0; cbase < ncell; cbase += 64) {
      const uint32_t c = cbase + static_cast<uint32_t>(lane);
      uint32_t myStart = 0, myCnt = 0;
      if (c < ncell) {  // cell c of the range, dz fastest (SpatialHash.h:108-125)
        const uint32_t dz = c % lz, dy = (c / lz) % ly, dx = c / (lz * ly);
        const uint32_t cs = find_bucket(H, X.B, mx + static_cast<int>(dx), my + static_cast<int>(dy), mz + static_cast<int>(dz));
        if (cs != 0xffffffffu) { myStart = H.start[cs]; myCnt = H.end[cs] - myStart; }
      }
      const uint32_t here = min(64u, ncell - cbase);
      for (uint32_t q = 0; q < here; ++q) {
        const uint32_t bs = static_cast<uint32_t>(__shfl(static_cast<int>(myStart), static_cast<int>(q), 64));
        const uint32_t bc = static_cast<uint32_t>(__shfl(static_cast<int>(myCnt), static_cast<int>(q), 64));
        if (bc) resolved += walk_bucket(GlobalBucket{X.G, X.val, bs}, bc, i, a, lane, X.friction, X.staticThreshold, tested);
      }
    }
    if (lane == 0) {
      store_node(X.G, i, a);
      if ((i & 1023u) == 0u) H.counters[kCounterProgress] = i;
    }
    drain_stores();
  }
  count_pass(H, resolved, tested, lane);
}

// resets the work queue of k_collide_flow without a new hash build (profile replays)
__global__ void k_collide_rearm(HashArrays H) {
  if (threadIdx.x == 0) {
    H.counters[kCounterTicket] = 0;
    H.counters[kCounterEpoch] += 1;
  }
}

// ----------------------------------------------------------------------------------------------------
uint32_t launch_collide(hipStream_t st_, const HashArrays& H, const NodeArrays& nd, float scale, float friction, float staticThreshold, bool rearm) {
  if (nd.n == 0) return 0;
  const dim3 grid(std::max<uint32_t>(1u, std::min<uint32_t>(2048u, (nd.n / 8 + 1) / 2)));
  auto flag = [](const char* name) { const char* e = tuning_env(name); return e && e[0] == '1' ? 1 : 0; };
  const int forceGlobal = flag("PIES_COLLIDE_GLOBAL");  // diagnostics, read when the substep is captured
  const int passes = flag("PIES_COLLIDE_PASSES");
  if (!passes) {
    uint32_t maxSpins = kColMaxSpins;
    if (const char* e = tuning_env("PIES_COLLIDE_SPIN_LIMIT")) maxSpins = static_cast<uint32_t>(std::strtoul(e, nullptr, 10));
    else if (const char* e = std::getenv("PIES_PROFILER_SAFE"); e && e[0] == '1') maxSpins = 0;
    if (rearm) hipLaunchKernelGGL(k_collide_rearm, dim3(1), dim3(64), 0, st_, H);
    hipLaunchKernelGGL(k_collide_flow, grid, dim3(kColBlock), 0, st_, H, nd.pos, nd.vel, nd.radius, friction, staticThreshold, forceGlobal,
                       maxSpins);
    // a cell with more nodes than the group order's tables hold: the pass in the reference's own order (returns at once otherwise)
    return 1 + launch_collide_reference(st_, H, nd, scale, friction, staticThreshold, H.counters + kCounterDense);
  }
  for (uint32_t pass = 0; pass < 27; ++pass)
    hipLaunchKernelGGL(k_collide, grid, dim3(kColBlock), 0, st_, H, nd.pos, nd.vel, nd.radius, pass, friction, staticThreshold, forceGlobal);
  return 27 + launch_collide_reference(st_, H, nd, scale, friction, staticThreshold, H.counters + kCounterDense);
}

uint32_t launch_collide_reference(hipStream_t st_, const HashArrays& H, const NodeArrays& nd, float scale, float friction, float staticThreshold,
                                  const uint32_t* gate) {
  if (nd.n == 0) return 0;
  unsigned long long budget = 1000000000ull;  // candidate tests a fallback pass may cost (a minute on the one wavefront; BASELINE config 4: 3.4e8)
  if (const char* e = tuning_env("PIES_FALLBACK_VISITS")) budget = std::strtoull(e, nullptr, 10);
  hipLaunchKernelGGL(k_collide_reference, dim3(1), dim3(64), 0, st_, H, nd.pos, nd.vel, nd.radius, nd.n, scale, friction, staticThreshold, gate, budget);
  return 1;
}

}  // namespace pies
