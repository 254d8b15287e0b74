// What the two orders of the node-node resolve by dependency levels share (pair_levels.hip: the pair order; pair_turns.hip: the
// reference's order by turns): the state a pass starts from, every node's filtered list of partners, the verification behind the
// pass, the check that arms its repeat - and the host steps that launch them.
//
// Filter.  Of the ~300 nodes that share a cell with a node only ~20 are near enough to ever touch it.  A pair is listed
// only if its distance at grid-build time is below r_i + r_j + s_i + s_j, and every node is checked to stay within its
// slack s_i of its build-time position whenever it has been moved: while that holds, every unlisted visit is a miss
// (|p_i - p_j| >= d0 - s_i - s_j >= r_i + r_j) and the result is that of the full order.  The slack is per node and follows
// what the node did in the passes before.  A node that leaves its slack is put on a list; after the pass one wavefront per
// listed node looks at the unlisted nodes it shares a cell with and tests, with the largest excursions both nodes had in the
// pass, whether the two can have touched (d0 - e_i - e_j < r_i + r_j).  Only if one such pair exists is the pass repeated from
// the saved state, the nodes that left their slack now listing every node they share a cell with; a repeat that fails the
// same test is counted (pies_get_collision_health: passes_inexact).
#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>
#include <utility>

#include "pair_device.h"

namespace pies {

constexpr uint32_t kMaxCand = 512;                         // distinct nodes of a group's 2x2x2 cells (BASELINE config 4: 216-343)
constexpr uint32_t kMaxOwn = 256;                          // nodes of one group
constexpr uint32_t kMaxDeg = 1024;                         // listed partners of one node
constexpr int kBuildWaves = 2;                            // wavefronts of a workgroup of the list kernel: one group at a time

// The reference order by turns looks a node's range up from its LIVE position when its turn starts, so a node can be met in a cell its
// partner was not inserted into when the lists were built.  The lists hold the pairs within reach that share a cell of the two INSERTED
// ranges; the ranges cover [p - r - 0.5, p + r + 0.5] per axis (Solver.cpp:877-901), so two nodes whose inserted ranges share no cell
// are r_i + r_j + 1 apart on some axis and can only touch in a pass in which their excursions add up to 1: while every node's
// excursion stays below kTurnMaxExcursion the lists (and k_pair_verify's test of the unlisted nodes that DO share a cell) cover every
// visit that can hit.  The nodes that stray further are looked at one by one after the pass (k_pair_verify); only a pass in which
// one of them can have touched a node it shares no inserted cell with is left to the sequential loop.
constexpr float kTurnMaxExcursion = 0.45f;
// slack of a node after a pass in which it strayed `exc` from its build-time position
PIES_DEV float next_slack(float exc, float previous, float r) {
  const float want = fmaxf(2.0f * exc + 0.1f * r, 0.4f * r);
  return previous < 1.0e30f ? fmaxf(want, 0.95f * previous) : want;
}

// every node's meetings with itself: it is in every bucket of its own range, once per cell (quirk Q3)
PIES_DEV uint32_t self_visits(const HashArrays& H, const PairArrays& P, uint32_t i, NodeState& a, const float4 p0, float friction, float staticThreshold) {
  const int4 rg = H.rng[i];
  const uint32_t m = (rg.w & 0xff) * ((rg.w >> 8) & 0xff) * ((rg.w >> 16) & 0xff);
  uint32_t hits = 0;
  for (uint32_t q = 0; q < m; ++q) hits += visit(a, a, friction, staticThreshold) ? 1u : 0u;
  if (hits) note_excursion(P, i, a, p0);
  return hits;
}

// ---- save: the state the pass starts from, control words, the meetings of every node with itself -------------------------
__global__ void __launch_bounds__(kBlock) k_pair_save(HashArrays H, PairArrays P, const float4* __restrict__ pos, const float4* __restrict__ vel,
                                                      const float* __restrict__ radius, float friction, float staticThreshold) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if (i == 0) {
    P.ctl[kPairFlags] = 0;
    P.ctl[kPairRetry] = 0;
    P.ctl[kPairRounds] = 0;
    P.ctl[kPairEdges] = 0;
    P.ctl[kPairGroups] = 0;
    P.ctl[kPairSpilled] = 0;
    P.ctl[kPairFallback] = 0;
    P.ctl[kPairBarrier] = 0;  // (the grid barrier of the levels behind the captured launches: counter, abort word)
    P.ctl[kPairBarrier + 1] = 0;
  }
  if (i < kPairPools) P.pool[i * kPairPad] = 0;
  if (i < 3u * kPairLists) P.frCount[i * kPairPad] = 0;
  if (i < 64u) { P.stat[i * kPairPad] = 0; P.stat[i * kPairPad + 1u] = 0; P.stat[i * kPairPad + 2u] = 0; }
  uint32_t hits = 0;
  if (i < P.n && !H.counters[kCounterFlags]) {
    const float4 p = pos[i], v = vel[i];
    const float r = radius[i];
    float sl = P.node[4u * i + 2u].w;
    if (!(sl > 0.0f)) sl = 0.5f * r;  // first pass after pies_finalize
    const float4 p0 = make_float4(p.x, p.y, p.z, sl);
    P.node[4u * i + 2u] = p0;
    P.bq[i] = make_float4(p.x, p.y, p.z, r + sl);
    P.vel0[i] = v;
    P.exc[i] = 0u;
    NodeState a{p.x, p.y, p.z, p.w, v.x, v.y, v.z, r};
    if (!P.byIndex) hits = self_visits(H, P, i, a, p0, friction, staticThreshold);
    store_node(P.node, i, a);
    // (by turns: a node meets itself inside its own turn, at its place in the bucket; a node no list is written for - an empty range -
    // has its own turn as its only event)
    store_rec(P.node, i, P.byIndex ? make_uint4(0u, 0u, 0u, i) : make_uint4(0u, 0u, 0u, 0u));
    if (P.byIndex) P.turnCnt[i] = 1u;
  }
  count_hits(P, hits, lane);
}
// the same for the repeat of a pass: the saved state is back in place (k_pair_check), the meetings with itself again
__global__ void __launch_bounds__(kBlock) k_pair_self(HashArrays H, PairArrays P, float friction, float staticThreshold) {
  if (!P.ctl[kPairRetry] || H.counters[kCounterFlags]) return;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint32_t hits = 0;
  if (i < P.n && P.byIndex) {  // by turns: the records start over (k_pair_save)
    store_rec(P.node, i, make_uint4(0u, 0u, 0u, i));
    P.turnCnt[i] = 1u;
  } else if (i < P.n) {
    NodeState a = load_node(P.node, i);
    hits = self_visits(H, P, i, a, P.node[4u * i + 2u], friction, staticThreshold);
    if (hits) store_node(P.node, i, a);
  }
  count_hits(P, hits, lane);
}

// ---- groups: one descriptor per group (the nodes whose minimum cell is the same cell) -------------------------------------
// The list kernel works group by group; what it needs of a group - the buckets of the 2x2x2 cells above the group's cell - is
// looked up here, one lane per cell in use, where the dependent look-ups of different cells overlap.
//   descriptor: [0..7] first entry of the eight buckets   [8..11] their lengths, 16 bits each   [12] the cell's slot
__global__ void __launch_bounds__(kBlock) k_pair_groups(HashArrays H, PairArrays P, uint32_t repeat) {
  if (repeat && !P.ctl[kPairRetry]) return;
  if (H.counters[kCounterFlags]) return;
  __shared__ uint32_t lcount, lbase;
  const uint32_t used = H.counters[kCounterUsed];
  const GridBox B = grid_box(H.counters);
  const uint32_t* __restrict__ val = H.val[grid_passes(B) & 1u];
  for (uint32_t first = blockIdx.x * kBlock; first < used; first += gridDim.x * kBlock) {  // (workgroup uniform)
    if (threadIdx.x == 0) lcount = 0;
    __syncthreads();
    const uint32_t u = first + threadIdx.x;
    uint32_t s = 0, rank = 0;
    bool have = false;
    if (u < used) {
      s = H.used[u];
      // a group exists where some node has its minimum cell (kMinFlag).  (k_grid_groups leaves that count in gcnt for the
      // group order; builds for the pair order skip that launch and look here.)
      const uint32_t bs = H.start[s], be = H.end[s];
      if (be - bs > 0xffffu) atomicOr(&P.ctl[kPairFlags], 2u);  // (a descriptor holds 16-bit bucket lengths; such a pile is the sequential loop's)
      for (uint32_t e = bs; e < be && !have; ++e) have = (val[e] >> 31) != 0u;
      if (have) rank = atomicAdd(&lcount, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && lcount) lbase = atomicAdd(&P.ctl[kPairGroups], lcount);
    __syncthreads();
    if (have) {
      int gx, gy, gz;
      box_cell(B, H.keys[s], gx, gy, gz);
      uint32_t st[8], cn[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t cs = find_bucket(H, B, gx + ((c >> 2) & 1), gy + ((c >> 1) & 1), gz + (c & 1));
        st[c] = cs != 0xffffffffu ? H.start[cs] : 0u;
        cn[c] = cs != 0xffffffffu ? min(H.end[cs] - st[c], 0xffffu) : 0u;  // (a bucket holds at most 2048 nodes)
      }
      uint4* d = P.grp + 4ull * (lbase + rank);
      d[0] = make_uint4(st[0], st[1], st[2], st[3]);
      d[1] = make_uint4(st[4], st[5], st[6], st[7]);
      d[2] = make_uint4(cn[0] | (cn[1] << 16), cn[2] | (cn[3] << 16), cn[4] | (cn[5] << 16), cn[6] | (cn[7] << 16));
      d[3] = make_uint4(s, 0u, 0u, 0u);
    }
    __syncthreads();
  }
}

// ---- lists: one workgroup per group -------------------------------------------------------------------------------------
// Everything a node of the group can share a cell with sits in the buckets of the 2x2x2 cells above the group's cell.  A node
// is in several of them; it is taken from the one that is the minimum corner of what its range shares with the block, which
// the side bits of its entry decide without a look at the node: (cell's offset in the block) & (cell's side in the node's
// range) == 0 on every axis.  The workgroup's wavefronts share the table of candidates and split the group's own nodes.
// The kernel exists in two sizes.  The small one (a group of BASELINE config 4 has ~300 candidates, a node ~20 partners) keeps
// twelve groups in flight per CU - the kernel is bound by the chain of dependent look-ups of a group, not by arithmetic - and
// passes groups that do not fit on to a list the large one works through.
template <uint32_t MAXC, uint32_t MAXD, uint32_t MAXOWN>
struct BuildLds {
  uint32_t id[MAXC];                                 // the distinct candidates: node index
  float px[MAXC], py[MAXC], pz[MAXC], rs[MAXC];      // position at grid-build time, radius + slack
  uint32_t rg[MAXC];                                 // (min cell - group cell + 1) per axis, 2 bits each; (length - 1) per axis from bit 8
  uint16_t own[MAXOWN];                              // candidates that are the group's own nodes
  uint32_t ncand, nown, spill;
  uint32_t looked[8];                                // candidates in the cells of a range of (1 or 2) x (1 or 2) x (1 or 2) cells from the group's cell
  uint64_t lk[kBuildWaves][MAXD];                    // one node's partners: pair key
  uint32_t le[kBuildWaves][MAXD];                    //                     partner | (shared cells - 1) << 28
  uint16_t near[kBuildWaves][2][MAXD];               // table slots of the candidates within reach of the wavefront's two nodes (first sweep)
};

// cells two ranges share on one axis: [a0, a0 + la) and [b0, b0 + lb)
PIES_DEV uint32_t shared_cells(int a0, uint32_t la, int b0, uint32_t lb) {
  const int lo = max(a0, b0), hi = min(a0 + static_cast<int>(la), b0 + static_cast<int>(lb));
  return hi > lo ? static_cast<uint32_t>(hi - lo) : 0u;
}

// appends the accepted candidates of the wavefront's lanes to the node's partner list in LDS; returns the new length
template <uint32_t MAXD>
PIES_DEV uint32_t push_partners(uint64_t* lk, uint32_t* le, uint32_t d, bool accept, uint32_t i, uint32_t j, uint32_t m, float pix, float piy, float piz,
                                float pjx, float pjy, float pjz, int lane, bool byIndex) {
  const unsigned long long mask = __ballot(accept);
  if (accept) {
    const uint32_t at = d + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
    if (at < MAXD) {
      // (the reference order by turns walks a node's partners in ascending index: the partner's index is the key)
      lk[at] = byIndex ? static_cast<uint64_t>(j) : pair_key_of(i, j, pix, piy, piz, pjx, pjy, pjz);
      le[at] = j | ((m - 1u) << 28);
    }
  }
  return d + static_cast<uint32_t>(__popcll(mask));
}

// sorts the d partners by key (rank sort: the keys are distinct) and writes the node's list into the wavefront's pool
PIES_DEV void write_list(const PairArrays& P, const uint64_t* lk, const uint32_t* le, uint32_t i, uint32_t d, uint32_t pool, int lane,
                         const uint32_t* lm = nullptr) {
  uint32_t at = 0;
  for (uint32_t tries = 0;; ++tries) {  // a full pool (long lists of one dense group) passes the node on to the next one
    if (lane == 0 && d) at = atomicAdd(&P.pool[pool * kPairPad], d);
    at = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(at)));
    if (at + d <= P.poolCap) break;
    if (tries + 1u == kPairPools) {  // (the node keeps an empty list; its partners wait for it for ever: flagged, the host latches the failure)
      if (lane == 0) atomicOr(&P.ctl[kPairFlags], 2u);
      return;
    }
    pool = (pool + 1u) % kPairPools;
  }
  const uint32_t off = pool * P.poolCap + at;
  __builtin_amdgcn_wave_barrier();
  uint32_t firstEntry = 0;
  bool haveFirst = false;
  for (uint32_t e = lane; e < d; e += 64) {
    const uint64_t k = lk[e];
    uint32_t rank = 0;
    for (uint32_t f = 0; f < d; ++f) rank += lk[f] < k ? 1u : 0u;
    const uint32_t v = le[e];
    P.nbr[off + rank] = v;
    if (lm) P.nbrM[off + rank] = lm[e];
    if (rank == 0u) { firstEntry = v; haveFirst = true; }
  }
  // the node's record: first entry, entries, cursor 0 reached in round 0, the current entry itself (from the lane that holds it)
  const unsigned long long who = __ballot(haveFirst);
  const uint32_t v0 = who ? static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(firstEntry), __builtin_ctzll(who))) : 0u;
  if (P.byIndex) {
    // reference order by turns (k_turn_round): entries | partners with a lower index << 16, event 0, the node whose turn the first
    // event is (the first partner if it has a lower index, else the node itself); the turn waits for its d + 1 members
    uint32_t below = 0;
    for (uint32_t e = lane; e < d; e += 64) below += lk[e] < static_cast<uint64_t>(i) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) below += __shfl_xor(below, o, 64);
    if (lane == 0) {
      store_rec(P.node, i, make_uint4(off, d | (below << 16), 0u, below ? (v0 & kPairNodeMask) : i));
      P.turnCnt[i] = d + 1u;
    }
  } else if (lane == 0) store_rec(P.node, i, make_uint4(off, d, 0u, v0));
  __builtin_amdgcn_wave_barrier();
}

// BIG: the groups the small kernel passed on (and, beyond MAXC candidates, node by node straight from the buckets)
// (The small instance asks for six wavefronts per SIMD: with two nodes per wavefront it took 100 registers - four wavefronts per
// SIMD, eight groups in flight per compute unit instead of twelve - and the third fewer instructions bought 10 %; at 80 registers
// and 11 spilled words config 4 went 95 / 137 -> 100 / 143.  The level kernel at the same setting was slower: 94 / 136.)
template <uint32_t MAXC, uint32_t MAXD, uint32_t MAXOWN, bool BIG>
__global__ void __launch_bounds__(64 * kBuildWaves, BIG ? 1 : 6) k_pair_build(HashArrays H, PairArrays P, uint32_t repeat) {
  __shared__ BuildLds<MAXC, MAXD, MAXOWN> L;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (repeat && !P.ctl[kPairRetry]) return;
  if (H.counters[kCounterFlags]) return;
  const uint32_t ngroups = BIG ? min(P.ctl[kPairSpilled], P.n) : min(P.ctl[kPairGroups], P.n);
  if (ngroups == 0u) return;
  const GridBox B = grid_box(H.counters);
  const uint32_t* __restrict__ val = H.val[grid_passes(B) & 1u];
  const uint32_t pool = (blockIdx.x * kBuildWaves + wv) % kPairPools;
  uint64_t* lk = L.lk[wv];
  uint32_t* le = L.le[wv];
  uint64_t tested = 0;
  uint32_t edges = 0;
  uint64_t testedAll = 0;
  uint32_t edgesAll = 0;
  for (uint32_t u = blockIdx.x; u < ngroups; u += gridDim.x, testedAll += tested, edgesAll += edges) {  // (workgroup uniform)
    tested = 0;
    edges = 0;
    const uint32_t g = BIG ? P.spill[u] : u;
    const uint4* __restrict__ desc = P.grp + 4ull * g;
    const uint4 d0 = desc[0], d1 = desc[1], d2 = desc[2];
    const uint32_t cStart[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
    const uint32_t cCnt[8] = {d2.x & 0xffffu, d2.x >> 16, d2.y & 0xffffu, d2.y >> 16, d2.z & 0xffffu, d2.z >> 16, d2.w & 0xffffu, d2.w >> 16};
    if (threadIdx.x == 0) { L.ncand = 0; L.nown = 0; L.spill = 0; }
    if (threadIdx.x < 8u) {  // (statistics: what the reference's loop would look at for a node of this group, by the lengths of its range)
      uint32_t sum = 0;
#pragma unroll
      for (uint32_t c = 0; c < 8u; ++c)
        if ((c & ~threadIdx.x) == 0u) sum += cCnt[c];
      L.looked[threadIdx.x] = sum;
    }
    __syncthreads();
    // ---- the distinct nodes of the eight buckets, each from its canonical cell; the group's own nodes.  Cells are dealt to the
    // wavefronts; a wavefront reserves a run of the table per 64 entries (the order of the table does not matter)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if ((c % kBuildWaves) != wv) continue;
      for (uint32_t base = 0; base < cCnt[c]; base += 64) {
        uint32_t v = 0;
        bool take = false;
        if (base + lane < cCnt[c]) {
          v = val[cStart[c] + base + lane];
          take = ((v >> kSideShift) & 7u & static_cast<uint32_t>(c)) == 0u;
        }
        const unsigned long long tm = __ballot(take);
        const bool mine = take && c == 0 && (v & kMinFlag) != 0u;
        const unsigned long long mm = __ballot(mine);
        uint32_t at = 0, ao = 0;
        if (lane == 0) {
          at = atomicAdd(&L.ncand, static_cast<uint32_t>(__popcll(tm)));
          if (mm) ao = atomicAdd(&L.nown, static_cast<uint32_t>(__popcll(mm)));
        }
        at = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(at))) + static_cast<uint32_t>(__popcll(tm & ((1ull << lane) - 1ull)));
        ao = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(ao))) + static_cast<uint32_t>(__popcll(mm & ((1ull << lane) - 1ull)));
        if (take && at < MAXC) {
          L.id[at] = v & kNodeMask;
          // the node's range relative to the group's cell, from the entry alone: its minimum is this cell minus the side bits
          const uint32_t side = (v >> kSideShift) & 7u, two = (v >> kLongShift) & 7u, cc = static_cast<uint32_t>(c);
          const uint32_t mnx = ((cc >> 2) & 1u) + 1u - ((side >> 2) & 1u), mny = ((cc >> 1) & 1u) + 1u - ((side >> 1) & 1u), mnz = (cc & 1u) + 1u - (side & 1u);
          L.rg[at] = mnx | (mny << 2) | (mnz << 4) | (((two >> 2) & 1u) << 8) | (((two >> 1) & 1u) << 14) | ((two & 1u) << 20);
        }
        if (mine && ao < MAXOWN && at < MAXC) L.own[ao] = static_cast<uint16_t>(at);
      }
    }
    __syncthreads();
    const uint32_t ncand = L.ncand, nown = L.nown;
    if (ncand > MAXC || nown > MAXOWN) {
      if (!BIG) {  // does not fit the small kernel: the large one takes the group
        if (threadIdx.x == 0) P.spill[atomicAdd(&P.ctl[kPairSpilled], 1u)] = g;
        __syncthreads();
        continue;
      }
      // ---- a dense neighbourhood: candidates straight from the buckets, node by node (wavefront 0 alone).  A partner sits in
      // several of the node's cells; it is taken where the cell is the minimum corner of what the two ranges share.
      if (wv == 0) {
        int gx, gy, gz;
        box_cell(B, H.keys[desc[3].x], gx, gy, gz);
        for (uint32_t ge = 0; ge < cCnt[0]; ++ge) {
          const uint32_t v = val[cStart[0] + ge];
          if (!(v & kMinFlag)) continue;  // (wave uniform)
          const uint32_t i = v & kNodeMask;
          const float4 pi = P.node[4u * i + 2u];
          const float rsi = P.node[4u * i + 1u].w + pi.w;
          const int4 rgi = H.rng[i];
          const uint32_t lxi = rgi.w & 0xff, lyi = (rgi.w >> 8) & 0xff, lzi = (rgi.w >> 16) & 0xff;
          uint32_t d = 0;
          for (uint32_t dx = 0; dx < lxi; ++dx)
            for (uint32_t dy = 0; dy < lyi; ++dy)
              for (uint32_t dz = 0; dz < lzi; ++dz) {
                const uint32_t c = (dx * 4 + dy * 2 + dz) & 7u;
                uint32_t bs = 0, bc = 0;
#pragma unroll
                for (int q = 0; q < 8; ++q)
                  if (c == static_cast<uint32_t>(q)) { bs = cStart[q]; bc = cCnt[q]; }
                tested += bc;
                const int cx = gx + static_cast<int>(dx), cy = gy + static_cast<int>(dy), cz = gz + static_cast<int>(dz);
                for (uint32_t base = 0; base < bc; base += 64) {
                  bool accept = false;
                  uint32_t j = 0, m = 0;
                  float4 pj = make_float4(0.f, 0.f, 0.f, 0.f);
                  if (base + lane < bc) {
                    j = val[bs + base + lane] & kNodeMask;
                    if (j != i) {
                      const int4 rgj = H.rng[j];
                      if (cx == max(rgi.x, rgj.x) && cy == max(rgi.y, rgj.y) && cz == max(rgi.z, rgj.z)) {
                        m = shared_cells(rgi.x, lxi, rgj.x, rgj.w & 0xff) * shared_cells(rgi.y, lyi, rgj.y, (rgj.w >> 8) & 0xff) *
                            shared_cells(rgi.z, lzi, rgj.z, (rgj.w >> 16) & 0xff);
                        pj = P.node[4u * j + 2u];
                        const float ddx = pj.x - pi.x, ddy = pj.y - pi.y, ddz = pj.z - pi.z;
                        const float cut = 1.001f * (rsi + (P.node[4u * j + 1u].w + pj.w));
                        accept = m != 0u && !(ddx * ddx + ddy * ddy + ddz * ddz >= cut * cut);
                      }
                    }
                  }
                  d = push_partners<MAXD>(lk, le, d, accept, i, j, m, pi.x, pi.y, pi.z, pj.x, pj.y, pj.z, lane, P.byIndex != 0u);
                }
              }
          __builtin_amdgcn_wave_barrier();
          if (d > MAXD) {  // a pile-up beyond anything a simulation survives: latch, like the > 2048 nodes in a cell of the grid
            if (lane == 0) atomicOr(&P.ctl[kPairFlags], 2u);
            d = MAXD;
          }
          write_list(P, lk, le, i, d, pool, lane);
          edges += d;
        }
      }
      __syncthreads();
      continue;
    }
    for (uint32_t t = threadIdx.x; t < ncand; t += 64 * kBuildWaves) {
      const float4 p = P.bq[L.id[t]];  // (the one gather per candidate)
      L.px[t] = p.x; L.py[t] = p.y; L.pz[t] = p.z; L.rs[t] = p.w;
    }
    __syncthreads();
    // Two own nodes per turn of a wavefront.  The first sweep - the distance test over all ~300 candidates - runs node after node
    // with all 64 lanes and leaves the slots of the ~25 within reach in LDS; when both nodes have at most 32 of them (nearly
    // always) the second sweep - shared cells and the pair key, 60 % of the instructions of a candidate round - and the rank sort
    // run for both at once, a half of the wavefront each: the kernel is bound by VALU issue (~350 wavefront instructions per
    // node) and these two parts kept 25 and 11 of 64 lanes busy.
    bool stop = false;
    for (uint32_t o = 2u * static_cast<uint32_t>(wv); o < nown && !stop; o += 2u * kBuildWaves) {
      const bool haveB = o + 1u < nown;
      uint32_t nnAB[2] = {0u, 0u};
      for (uint32_t h = 0; h < (haveB ? 2u : 1u); ++h) {  // ---- first sweep
        const uint32_t si = L.own[o + h];
        const float pix = L.px[si], piy = L.py[si], piz = L.pz[si], rsi = L.rs[si];
        uint16_t* near = L.near[wv][h];
        // a lane keeps the rounds in which its candidate was within reach as bits and the slots are compacted once at the end (a
        // ballot, two bit counts and a bounds test per round were two thirds of a round's instructions); up to 32 rounds (MAXC <= 2048)
        uint32_t bits = 0;
        for (uint32_t base = 0, r = 0; base < ncand; base += 64, ++r) {
          const uint32_t t = base + static_cast<uint32_t>(lane);
          if (t < ncand && t != si) {
            const float ddx = L.px[t] - pix, ddy = L.py[t] - piy, ddz = L.pz[t] - piz;
            const float cut = 1.001f * (rsi + L.rs[t]);  // (wide for a node that left its slack in the first attempt)
            if (!(ddx * ddx + ddy * ddy + ddz * ddz >= cut * cut)) bits |= 1u << r;
          }
        }
        const uint32_t mine = static_cast<uint32_t>(__popc(bits));
        uint32_t incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const uint32_t up = __shfl_up(incl, off, 64);
          if (lane >= off) incl += up;
        }
        const uint32_t nn = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(incl), 63));
        uint32_t at = incl - mine;
        while (bits) {
          const uint32_t r = static_cast<uint32_t>(__builtin_ctz(bits));
          bits &= bits - 1u;
          if (at < MAXD) near[at] = static_cast<uint16_t>(r * 64u + static_cast<uint32_t>(lane));
          ++at;
        }
        nnAB[h] = nn;
      }
      __builtin_amdgcn_wave_barrier();
      // the candidates the reference's loop would look at for a node (statistics: SURVEY 8d counts 16 B for each): the cells
      // (dx, dy, dz) below its range's lengths, from the group's table (a loop over cCnt[] here cost 150-260 instructions per node)
      auto looked_of = [&](uint32_t rgi) { return L.looked[(((rgi >> 8) & 1u) << 2) | (((rgi >> 14) & 1u) << 1) | ((rgi >> 20) & 1u)]; };
      if (!BIG && haveB && nnAB[0] <= 32u && nnAB[1] <= 32u && P.byIndex == 0u) {
        // ---- second sweep and lists of both nodes, a half of the wavefront each
        const uint32_t h = static_cast<uint32_t>(lane) >> 5, hl = static_cast<uint32_t>(lane) & 31u;
        const unsigned long long halfMask = 0xffffffffull << (32u * h);
        const uint32_t si = L.own[o + h];
        const uint32_t i = L.id[si];
        const float pix = L.px[si], piy = L.py[si], piz = L.pz[si];
        const uint32_t rgi = L.rg[si];
        const uint32_t lxi = ((rgi >> 8) & 63u) + 1u, lyi = ((rgi >> 14) & 63u) + 1u, lzi = ((rgi >> 20) & 63u) + 1u;
        const uint32_t nn = h ? nnAB[1] : nnAB[0];
        uint64_t* lkh = lk + h * (MAXD / 2u);
        uint32_t* leh = le + h * (MAXD / 2u);
        bool accept = false;
        uint32_t j = 0, m = 0;
        float pjx = 0.f, pjy = 0.f, pjz = 0.f;
        if (hl < nn) {
          const uint32_t t = L.near[wv][h][hl];
          pjx = L.px[t]; pjy = L.py[t]; pjz = L.pz[t];
          j = L.id[t];
          const uint32_t rgj = L.rg[t];
          m = shared_cells(0, lxi, static_cast<int>(rgj & 3u) - 1, ((rgj >> 8) & 63u) + 1u) *
              shared_cells(0, lyi, static_cast<int>((rgj >> 2) & 3u) - 1, ((rgj >> 14) & 63u) + 1u) *
              shared_cells(0, lzi, static_cast<int>((rgj >> 4) & 3u) - 1, ((rgj >> 20) & 63u) + 1u);
          accept = m != 0u;
        }
        const unsigned long long am = __ballot(accept) & halfMask;
        const uint32_t d = static_cast<uint32_t>(__popcll(am));
        if (accept) {
          const uint32_t at = static_cast<uint32_t>(__popcll(am & ((1ull << lane) - 1ull)));
          lkh[at] = pair_key_of(i, j, pix, piy, piz, pjx, pjy, pjz);
          leh[at] = j | ((m - 1u) << 28);
        }
        __builtin_amdgcn_wave_barrier();
        // storage from a pool (a full pool passes the node on to the next one, like write_list)
        uint32_t poolH = pool, at = 0;
        bool placed = false, failed = false;
        for (uint32_t tries = 0; tries < kPairPools; ++tries) {
          uint32_t got = 0;
          if (!placed && hl == 0u && d) got = atomicAdd(&P.pool[poolH * kPairPad], d);
          got = static_cast<uint32_t>(__shfl(static_cast<int>(got), static_cast<int>(32u * h), 64));
          if (!placed) {
            if (got + d <= P.poolCap) { at = got; placed = true; }
            else if (tries + 1u == kPairPools) { failed = true; placed = true; }
            else poolH = (poolH + 1u) % kPairPools;
          }
          if (__ballot(!placed) == 0ull) break;
        }
        if (failed && hl == 0u) atomicOr(&P.ctl[kPairFlags], 2u);  // (the node keeps an empty list: flagged, the pass goes to the sequential loop)
        const uint32_t off = poolH * P.poolCap + at;
        uint32_t firstEntry = 0;
        bool haveFirst = false;
        const uint32_t dMax = max(static_cast<uint32_t>(__shfl(static_cast<int>(d), 0, 64)), static_cast<uint32_t>(__shfl(static_cast<int>(d), 32, 64)));
        if (!failed) {
          const uint64_t k = hl < d ? lkh[hl] : 0ull;
          uint32_t rank = 0;
          for (uint32_t f = 0; f < dMax; ++f) rank += (f < d && lkh[min(f, MAXD / 2u - 1u)] < k) ? 1u : 0u;
          if (hl < d) {
            const uint32_t v = leh[hl];
            P.nbr[off + rank] = v;
            if (rank == 0u) { firstEntry = v; haveFirst = true; }
          }
        }
        const unsigned long long who = __ballot(haveFirst) & halfMask;
        const uint32_t v0 = static_cast<uint32_t>(__shfl(static_cast<int>(firstEntry), who ? __builtin_ctzll(who) : 0, 64));
        if (hl == 0u && !failed) store_rec(P.node, i, make_uint4(off, d, 0u, who ? v0 : 0u));
        __builtin_amdgcn_wave_barrier();
        tested += looked_of(L.rg[L.own[o]]) + looked_of(L.rg[L.own[o + 1u]]);
        edges += static_cast<uint32_t>(__shfl(static_cast<int>(d), 0, 64)) + static_cast<uint32_t>(__shfl(static_cast<int>(d), 32, 64));
        continue;
      }
      for (uint32_t h = 0; h < (haveB ? 2u : 1u) && !stop; ++h) {  // ---- a node at a time (long lists, the large kernel, the order by turns)
        const uint32_t si = L.own[o + h];
        const uint32_t i = L.id[si];
        const float pix = L.px[si], piy = L.py[si], piz = L.pz[si];
        const uint32_t rgi = L.rg[si];
        const uint32_t lxi = ((rgi >> 8) & 63u) + 1u, lyi = ((rgi >> 14) & 63u) + 1u, lzi = ((rgi >> 20) & 63u) + 1u;
        const uint16_t* near = L.near[wv][h];
        const uint32_t nn = nnAB[h];
        uint32_t d = nn > MAXD ? MAXD + 1u : 0u;  // (more within reach than a list holds: handled below like a list that is too long)
        for (uint32_t base = 0; base < nn && nn <= MAXD; base += 64) {
          const uint32_t e = base + static_cast<uint32_t>(lane);
          bool accept = false;
          uint32_t j = 0, m = 0;
          float pjx = 0.f, pjy = 0.f, pjz = 0.f;
          if (e < nn) {
            const uint32_t t = near[e];
            pjx = L.px[t]; pjy = L.py[t]; pjz = L.pz[t];
            j = L.id[t];
            const uint32_t rgj = L.rg[t];
            m = shared_cells(0, lxi, static_cast<int>(rgj & 3u) - 1, ((rgj >> 8) & 63u) + 1u) *
                shared_cells(0, lyi, static_cast<int>((rgj >> 2) & 3u) - 1, ((rgj >> 14) & 63u) + 1u) *
                shared_cells(0, lzi, static_cast<int>((rgj >> 4) & 3u) - 1, ((rgj >> 20) & 63u) + 1u);
            accept = m != 0u;
          }
          d = push_partners<MAXD>(lk, le, d, accept, i, j, m, pix, piy, piz, pjx, pjy, pjz, lane, P.byIndex != 0u);
        }
        __builtin_amdgcn_wave_barrier();
        if (d > MAXD) {
          if (!BIG) { if (lane == 0) L.spill = 1; stop = true; break; }  // (the large kernel redoes the group; lists written so far are replaced)
          if (lane == 0) atomicOr(&P.ctl[kPairFlags], 2u);  // a pile-up beyond anything a simulation survives: latch
          d = MAXD;
        }
        tested += looked_of(rgi);
        write_list(P, lk, le, i, d, pool, lane);
        edges += d;
      }
    }
    __syncthreads();  // (the table is reused by the next group)
    if (!BIG && L.spill) {
      if (threadIdx.x == 0) P.spill[atomicAdd(&P.ctl[kPairSpilled], 1u)] = g;
      tested = 0;  // (what this group has counted so far is counted again by the large kernel)
      edges = 0;
      __syncthreads();
    }
  }
  // statistics, striped (same-address atomics of 16 000 wavefronts would take longer than the lists)
  if (lane == 0 && testedAll) atomicAdd(reinterpret_cast<unsigned long long*>(&P.stat[(blockIdx.x % 64u) * kPairPad]), static_cast<unsigned long long>(testedAll));
  if (lane == 0 && edgesAll) atomicAdd(&P.stat[(blockIdx.x % 64u) * kPairPad + 2u], edgesAll);
}

// ---- lists for scenes whose ranges are wider than two cells per axis (gridSpacing < 2 (r + 0.5): NodeCompRange allows up to 50
// cells per axis): one wavefront per NODE walks the buckets of the node's own range.  A partner sits in several of them; it is
// taken where the cell is the minimum corner of what the two ranges share (a look at the partner's range: one more gather per
// candidate than the 2x2x2 path needs).  The number of shared cells does not fit the entry's four bits: it goes to nbrM.
struct WideLds {
  uint64_t lk[kMaxDeg];
  uint32_t le[kMaxDeg], lm[kMaxDeg];
};
__global__ void __launch_bounds__(64) k_pair_build_wide(HashArrays H, PairArrays P, uint32_t repeat) {
  __shared__ WideLds L;
  const int lane = threadIdx.x;
  if (repeat && !P.ctl[kPairRetry]) return;
  if (H.counters[kCounterFlags]) return;
  const GridBox B = grid_box(H.counters);
  const uint32_t* __restrict__ val = H.val[grid_passes(B) & 1u];
  const uint32_t pool = blockIdx.x % kPairPools;
  uint64_t tested = 0;
  uint32_t edges = 0;
  for (uint32_t i = blockIdx.x; i < P.n; i += gridDim.x) {
    const int4 rgi = H.rng[i];
    const uint32_t lxi = rgi.w & 0xff, lyi = (rgi.w >> 8) & 0xff, lzi = (rgi.w >> 16) & 0xff;
    if (lxi * lyi * lzi == 0u) continue;  // an over-long range is empty (Solver.cpp:896-898): the node visits nothing
    const float4 pi = P.node[4u * i + 2u];
    const float rsi = P.node[4u * i + 1u].w + pi.w;
    uint32_t d = 0;
    for (uint32_t dx = 0; dx < lxi; ++dx)
      for (uint32_t dy = 0; dy < lyi; ++dy)
        for (uint32_t dz = 0; dz < lzi; ++dz) {
          const int cx = rgi.x + static_cast<int>(dx), cy = rgi.y + static_cast<int>(dy), cz = rgi.z + static_cast<int>(dz);
          const uint32_t cs = find_bucket(H, B, cx, cy, cz);
          if (cs == 0xffffffffu) continue;
          const uint32_t bs = H.start[cs], bc = H.end[cs] - bs;
          tested += bc;
          for (uint32_t base = 0; base < bc; base += 64) {
            bool accept = false;
            uint32_t j = 0, m = 0;
            float4 pj = make_float4(0.f, 0.f, 0.f, 0.f);
            if (base + lane < bc) {
              j = val[bs + base + lane] & kNodeMask;
              if (j != i) {
                const int4 rgj = H.rng[j];
                if (cx == max(rgi.x, rgj.x) && cy == max(rgi.y, rgj.y) && cz == max(rgi.z, rgj.z)) {
                  m = shared_cells(rgi.x, lxi, rgj.x, rgj.w & 0xff) * shared_cells(rgi.y, lyi, rgj.y, (rgj.w >> 8) & 0xff) *
                      shared_cells(rgi.z, lzi, rgj.z, (rgj.w >> 16) & 0xff);
                  pj = P.node[4u * j + 2u];
                  const float ddx = pj.x - pi.x, ddy = pj.y - pi.y, ddz = pj.z - pi.z;
                  const float cut = 1.001f * (rsi + (P.node[4u * j + 1u].w + pj.w));
                  accept = m != 0u && !(ddx * ddx + ddy * ddy + ddz * ddz >= cut * cut);
                }
              }
            }
            const unsigned long long mask = __ballot(accept);
            if (accept) {
              const uint32_t at = d + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
              if (at < kMaxDeg) {
                L.lk[at] = P.byIndex ? static_cast<uint64_t>(j) : pair_key_of(i, j, pi.x, pi.y, pi.z, pj.x, pj.y, pj.z);
                L.le[at] = j;
                L.lm[at] = m;
              }
            }
            d += static_cast<uint32_t>(__popcll(mask));
          }
        }
    __builtin_amdgcn_wave_barrier();
    if (d > kMaxDeg) {  // a pile-up beyond anything a simulation survives: latch
      if (lane == 0) atomicOr(&P.ctl[kPairFlags], 2u);
      d = kMaxDeg;
    }
    write_list(P, L.lk, L.le, i, d, pool, lane, L.lm);
    edges += d;
  }
  if (lane == 0 && tested) atomicAdd(reinterpret_cast<unsigned long long*>(&P.stat[(blockIdx.x % 64u) * kPairPad]), static_cast<unsigned long long>(tested));
  if (lane == 0 && edges) atomicAdd(&P.stat[(blockIdx.x % 64u) * kPairPad + 2u], edges);
}

// ---- after the pass: can an unlisted pair have touched? -----------------------------------------------------------------
// One wavefront per node that left its slack: the nodes it shares a cell with but did not list (d0 >= cut) are tested with the
// largest excursions of the pass.
__global__ void __launch_bounds__(kBlock) k_pair_verify(HashArrays H, PairArrays P, uint32_t repeat, float scale) {
  if (repeat && !P.ctl[kPairRetry]) return;
  if (H.counters[kCounterFlags]) return;
  const int lane = threadIdx.x & 63;
  const GridBox B = grid_box(H.counters);
  const uint32_t* __restrict__ val = H.val[grid_passes(B) & 1u];
  const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6, nwaves = (gridDim.x * kBlock) >> 6;
  if (P.byIndex) {
    // By turns: the nodes that strayed far (see kTurnMaxExcursion) may have walked buckets of cells their inserted range does not
    // hold and met nodes no list knows.  One wavefront per such node looks at every node inserted into a cell its live range can
    // have reached - the range of a sphere of radius r + excursion around its build-time position - that shares NO inserted cell
    // with it, and tests with the largest excursions of the pass whether the two can have touched.  If so the pass is the
    // sequential loop's (a repeat would list the same pairs).
    bool lost = false;
    for (uint32_t base = wave * 64u; base < P.n; base += nwaves * 64u) {  // (wavefront uniform)
      const uint32_t mine = base + static_cast<uint32_t>(lane);
      const float em = mine < P.n ? __uint_as_float(P.exc[mine]) : 0.0f;
      unsigned long long far = __ballot(!(em < kTurnMaxExcursion));
      while (far) {
        const uint32_t q = static_cast<uint32_t>(__builtin_ctzll(far));
        far &= far - 1ull;
        const uint32_t i = base + q;
        const float4 pi = P.node[4u * i + 2u];
        const float ri = P.node[4u * i + 1u].w, ei = lane_value(em, q);
        const int4 rgi = H.rng[i];
        int mx, my, mz;
        uint32_t lx, ly, lz;
        if (!node_range(pi.x, pi.y, pi.z, ri + ei, scale, mx, my, mz, lx, ly, lz) || lx * ly * lz == 0u) { lost = true; continue; }
        for (uint32_t c = 0; c < lx * ly * lz; ++c) {
          const uint32_t cs = find_bucket(H, B, mx + static_cast<int>(c / (lz * ly)), my + static_cast<int>((c / lz) % ly), mz + static_cast<int>(c % lz));
          if (cs == 0xffffffffu) continue;
          const uint32_t bs = H.start[cs], bc = H.end[cs] - bs;
          for (uint32_t b0 = 0; b0 < bc; b0 += 64u) {
            if (b0 + lane >= bc) continue;
            const uint32_t j = val[bs + b0 + lane] & kNodeMask;
            if (j == i) continue;
            const int4 rgj = H.rng[j];
            if (shared_cells(rgi.x, rgi.w & 0xff, rgj.x, rgj.w & 0xff) * shared_cells(rgi.y, (rgi.w >> 8) & 0xff, rgj.y, (rgj.w >> 8) & 0xff) *
                    shared_cells(rgi.z, (rgi.w >> 16) & 0xff, rgj.z, (rgj.w >> 16) & 0xff) != 0u)
              continue;  // (they share an inserted cell: the lists and the test below cover the pair)
            const float4 pj = P.node[4u * j + 2u];
            const float ddx = pj.x - pi.x, ddy = pj.y - pi.y, ddz = pj.z - pi.z;
            const float reach = 1.001f * (ri + P.node[4u * j + 1u].w + ei + __uint_as_float(P.exc[j]));
            if (!(ddx * ddx + ddy * ddy + ddz * ddz >= reach * reach)) lost = true;
          }
        }
      }
    }
    if (__ballot(lost) && lane == 0) atomicOr(&P.ctl[kPairFlags], 2u);
  }
  const uint32_t count = min(P.ctl[kPairLeft], P.n);
  if (count == 0u) return;
  bool bad = false;
  for (uint32_t u = wave; u < count; u += nwaves) {
    const uint32_t i = P.left[u];
    const float4 pi = P.node[4u * i + 2u];
    const float ri = P.node[4u * i + 1u].w, ei = __uint_as_float(P.exc[i]);
    const int4 rg = H.rng[i];
    const uint32_t lx = rg.w & 0xff, ly = (rg.w >> 8) & 0xff, lz = (rg.w >> 16) & 0xff;
    for (uint32_t dx = 0; dx < lx; ++dx)
      for (uint32_t dy = 0; dy < ly; ++dy)
        for (uint32_t dz = 0; dz < lz; ++dz) {
          const uint32_t cs = find_bucket(H, B, rg.x + static_cast<int>(dx), rg.y + static_cast<int>(dy), rg.z + static_cast<int>(dz));
          if (cs == 0xffffffffu) continue;
          const uint32_t bs = H.start[cs], bc = H.end[cs] - bs;
          for (uint32_t base = 0; base < bc; base += 64) {
            if (base + lane >= bc) continue;
            const uint32_t j = val[bs + base + lane] & kNodeMask;
            if (j == i) continue;
            const float4 pj = P.node[4u * j + 2u];
            const float rj = P.node[4u * j + 1u].w;
            const float ddx = pj.x - pi.x, ddy = pj.y - pi.y, ddz = pj.z - pi.z;
            const float d2 = ddx * ddx + ddy * ddy + ddz * ddz;
            const float cut = 1.001f * ((ri + pi.w) + (rj + pj.w));
            if (!(d2 >= cut * cut)) continue;  // listed: it was visited
            const float reach = 1.001f * (ri + rj + ei + __uint_as_float(P.exc[j]));
            if (!(d2 >= reach * reach)) bad = true;  // the two may have touched while the pair was skipped
          }
        }
  }
  if (__ballot(bad) && lane == 0) atomicOr(&P.ctl[kPairFlags], 1u);
}

// first = after the first attempt.  A failed verification puts the saved state back and arms the repeat, in which the nodes
// that left their slack get the room they took in the first attempt and more.  Otherwise (and after the repeat) the result goes
// back to the solver's node arrays and every node's slack follows what it did.
__global__ void __launch_bounds__(kBlock) k_pair_check(HashArrays H, PairArrays P, float4* pos, float4* vel, uint32_t first) {
  const uint32_t flags = P.ctl[kPairFlags];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool overflow = (flags & 2u) != 0u;  // the lists are incomplete: the pass is the sequential loop's, nothing of it is kept
  const bool repeat = first && (flags & 1u) && !overflow;
  if (!first && !P.ctl[kPairRetry]) return;  // nothing was repeated: the first check has done everything
  if (i < P.n && !H.counters[kCounterFlags]) {
    const float4 p0 = P.node[4u * i + 2u];
    const float e = __uint_as_float(P.exc[i]), sl = p0.w;
    if (repeat) {
      const float4 v0 = P.vel0[i];
      const float r = P.node[4u * i + 1u].w;
      P.node[4u * i] = make_float4(p0.x, p0.y, p0.z, P.node[4u * i].w);
      P.node[4u * i + 1u] = make_float4(v0.x, v0.y, v0.z, r);
      store_rec(P.node, i, make_uint4(0u, 0u, 0u, 0u));
      P.exc[i] = 0u;
      if (!(e <= 0.999f * sl)) {  // (the repeat follows the first attempt's course until a newly listed pair touches)
        const float room = 2.0f * e + 0.2f * r;
        P.node[4u * i + 2u].w = room;
        P.bq[i].w = r + room;
      }
    } else {
      const float4 p = P.node[4u * i], v = P.node[4u * i + 1u];
      // (by turns, a pass that could not be proved exact in its repeat either is left to the sequential loop: pos / vel keep the
      // state the pass started from)
      if (!(P.byIndex && !first && (flags & 1u)) && !overflow) {
        pos[i] = p;
        vel[i] = make_float4(v.x, v.y, v.z, 0.0f);  // (the fourth component of a velocity record is 0 everywhere)
      }
      P.node[4u * i + 2u].w = next_slack(e, sl, v.w);
    }
  }
  // the pass's resolved pairs go to the statistics when its result stands (a pass that is repeated counts once; one that is left to
  // the sequential loop is counted by that loop)
  if (blockIdx.x == 0 && !repeat && !(P.byIndex && !first && (flags & 1u)) && !overflow) {
    uint32_t sum = 0;
    for (uint32_t k = threadIdx.x; k < kPairStripes; k += kBlock) { sum += P.hitStripe[k * kPairPad]; P.hitStripe[k * kPairPad] = 0; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&H.counters[kCounterPairs], sum);
    if (threadIdx.x < 64) {  // candidates looked at (64 bit) and listed entries
      unsigned long long c = *reinterpret_cast<unsigned long long*>(&P.stat[threadIdx.x * kPairPad]);
      uint32_t e = P.stat[threadIdx.x * kPairPad + 2u];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) { c += __shfl_xor(c, o, 64); e += __shfl_xor(e, o, 64); }
      if (threadIdx.x == 0) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&H.counters[kCounterCandidates]), c);
        P.ctl[kPairEdges] = e;
      }
    }
  } else if (blockIdx.x == 0) {
    for (uint32_t k = threadIdx.x; k < kPairStripes; k += kBlock) P.hitStripe[k * kPairPad] = 0;
    if (threadIdx.x < 64) { P.stat[threadIdx.x * kPairPad] = 0; P.stat[threadIdx.x * kPairPad + 1u] = 0; P.stat[threadIdx.x * kPairPad + 2u] = 0; }
  }
  if (i != 0 || first) return;
  if (flags & 1u) P.ctl[kPairInexact] += 1;
  if ((P.byIndex && (flags & 1u)) || (flags & 2u)) { P.ctl[kPairFallback] = 1u; P.ctl[kPairFallbacks] += 1u; }  // (list storage overflow in the repeat)
  P.ctl[kPairLeft] = 0;
}
// (one thread, after every block of the first k_pair_check has read the flags)
__global__ void k_pair_arm(HashArrays H, PairArrays P) {
  if (P.ctl[kPairFlags] & 1u) {
    if (threadIdx.x < kPairPools) P.pool[threadIdx.x * kPairPad] = 0;
    for (uint32_t k = threadIdx.x; k < 3u * kPairLists; k += 64) P.frCount[k * kPairPad] = 0;
  }
  if (threadIdx.x != 0) return;
  const uint32_t flags = P.ctl[kPairFlags];
  P.ctl[kPairLeft] = 0;
  if (flags & 2u) {  // a pile the lists do not hold (more than 1 024 partners of a node, more entries than reserved): no repeat - the
    P.ctl[kPairFallback] = 1u;  // sequential loop runs the pass from the state it started with (the reference has no such limit)
    P.ctl[kPairFallbacks] += 1u;
    return;
  }
  if (!(flags & 1u)) return;
  P.ctl[kPairRetry] = 1;
  P.ctl[kPairBarrier] = 0;      // k_pair_repeat's grid barrier: counter, abort word
  P.ctl[kPairBarrier + 1] = 0;
  P.ctl[kPairRetries] += 1;
  P.ctl[kPairFlags] = 0;
  P.ctl[kPairEdges] = 0;
  P.ctl[kPairSpilled] = 0;
}

// ---- the host steps of a pass that both orders share -----------------------------------------------------------------------------
uint32_t resident_blocks_halved(const void* kernel, int threads, uint32_t ldsBytes) {
  static std::mutex mu;
  static std::map<std::tuple<const void*, uint32_t, int>, uint32_t> cache;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_tuple(kernel, ldsBytes, dev);
  const auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int perCu = 0;
  hipDeviceProp_t prop;
  uint32_t v = 0;
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess && hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, kernel, threads, ldsBytes) == hipSuccess)
    v = static_cast<uint32_t>(std::max(0, perCu)) * static_cast<uint32_t>(std::max(0, prop.multiProcessorCount)) / 2u;
  cache[key] = v;
  return v;
}

static dim3 per_node(uint32_t n) { return dim3((n + kBlock - 1) / kBlock); }

uint32_t pass_begin(hipStream_t st, const HashArrays& H, const PairArrays& P, const NodeArrays& nd, float friction, float staticThreshold) {
  uint32_t launches = 0;
  hipLaunchKernelGGL(k_pair_save, per_node(P.n), dim3(kBlock), 0, st, H, P, nd.pos, nd.vel, nd.radius, friction, staticThreshold); ++launches;
  if (!P.nbrM) { hipLaunchKernelGGL(k_pair_groups, dim3(std::min<uint32_t>(2048u, (H.capacity / 8 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, H, P, 0u); ++launches; }
  return launches;
}

uint32_t pass_lists(hipStream_t st, const HashArrays& H, const PairArrays& P, float friction, float staticThreshold, uint32_t repeat) {
  const uint32_t n = P.n;
  uint32_t launches = 0;
  if (repeat) { hipLaunchKernelGGL(k_pair_self, per_node(n), dim3(kBlock), 0, st, H, P, friction, staticThreshold); ++launches; }
  if (P.nbrM) {  // ranges of more than two cells per axis: lists node by node
    hipLaunchKernelGGL(k_pair_build_wide, dim3(std::max<uint32_t>(1u, std::min<uint32_t>(16384u, n))), dim3(64), 0, st, H, P, repeat); ++launches;
  } else {
    const dim3 groups(std::max<uint32_t>(1u, std::min<uint32_t>(8192u, n / 8 + 1)));
    hipLaunchKernelGGL((k_pair_build<384, 96, 64, false>), groups, dim3(64 * kBuildWaves), 0, st, H, P, repeat); ++launches;
    hipLaunchKernelGGL((k_pair_build<kMaxCand, kMaxDeg, kMaxOwn, true>), dim3(512), dim3(64 * kBuildWaves), 0, st, H, P, repeat); ++launches;
  }
  return launches;
}

uint32_t pass_end(hipStream_t st, const HashArrays& H, const PairArrays& P, const NodeArrays& nd, float gridSpacing, float friction,
                  float staticThreshold, uint32_t repeat) {
  uint32_t launches = 0;
  hipLaunchKernelGGL(k_pair_verify, dim3(64), dim3(kBlock), 0, st, H, P, repeat, gridSpacing); ++launches;
  hipLaunchKernelGGL(k_pair_check, per_node(P.n), dim3(kBlock), 0, st, H, P, nd.pos, nd.vel, repeat ? 0u : 1u); ++launches;
  if (!repeat) { hipLaunchKernelGGL(k_pair_arm, dim3(1), dim3(64), 0, st, H, P); ++launches; }
  // a pile the lists do not hold, or (by turns) a pass that could not be proved exact twice: the sequential loop in the reference's
  // own order, on the state the pass started from (it returns at once otherwise)
  else launches += launch_collide_reference(st, H, nd, gridSpacing, friction, staticThreshold, P.ctl + kPairFallback);
  return launches;
}
}  // namespace pies
