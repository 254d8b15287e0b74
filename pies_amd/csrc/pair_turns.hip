// ======================================================================================================================
// The REFERENCE's order (Solver.cpp:85-130) by dependency levels of TURNS
// ======================================================================================================================
// The reference's loop gives every node its turn in ascending index: the node's cell range is looked up from its LIVE position
// (SpatialHash.h:101-106), the buckets of that range are walked in dx, dy, dz order and their nodes in ascending index, and every
// overlapping visit is resolved at once.  k_collide_reference (group_resolve.hip) runs that as one chain on one wavefront: 20 us
// per node.  Here the same turns run by dependency levels:
//   * who a turn can touch: the node's partners within reach when the grid was built (the pair order's filtered lists, sorted by
//     INDEX here; a visit to anybody else is a miss as long as every node stays within its slack - the pair order's proof obligation,
//     checked by the same k_pair_verify, repeated with wider slacks, and left to the sequential kernel when that fails too);
//   * a node j lives through the turns of its partners below it, its own turn, the turns of its partners above it - in that order.
//     Turn i may run when every member of it (i and its partners) has had all its earlier events.  Two turns that are ready at the
//     same time share no member, so a level is one launch, one wavefront per turn;
//   * inside a turn the wavefront holds the partners in its lanes (ascending index).  For every cell of the live range, in order:
//     the lanes whose partner was INSERTED into that cell test the overlap against the node's current state, the lowest hit is
//     resolved (Solver.cpp:88-126, the same visit() as the pair order's), the node's new state goes to every lane, the lanes above
//     test again; the node meets itself at its place in the bucket (quirk Q3).  The visits that are skipped are the ones that miss.
// The result is the sequential loop's, bit for bit: tests/test_collisions_gpu.py runs both against the oracle's plain loop.
#include <algorithm>

#include "pair_device.h"

namespace pies {

constexpr uint32_t kTurnDone = 0xffffffffu;
constexpr uint32_t kTurnBlock = 256;

// the node whose turn event t of node j is: partners below j, j itself, partners above j
PIES_DEV uint32_t turn_event_node(const PairArrays& P, uint32_t j, uint32_t off, uint32_t d, uint32_t below, uint32_t t) {
  if (t > d) return kTurnDone;
  if (t == below) return j;
  return P.nbr[off + (t < below ? t : t - 1u)] & kPairNodeMask;
}
PIES_DEV bool cell_in_range(const int4 rg, int cx, int cy, int cz) {
  const int lx = rg.w & 0xff, ly = (rg.w >> 8) & 0xff, lz = (rg.w >> 16) & 0xff;
  return cx >= rg.x && cx < rg.x + lx && cy >= rg.y && cy < rg.y + ly && cz >= rg.z && cz < rg.z + lz;
}


// One bucket of a turn: the lanes with inCell hold the bucket's partners of node a (ascending index over the lanes), selfAt = the
// lane before which the node meets itself (64: behind the last lane; kTurnDone: not in this bucket / not in this batch).
PIES_DEV void turn_cell(NodeState& a, NodeState& b, bool inCell, uint32_t selfAt, int lane, float friction, float staticThreshold, uint32_t& hits,
                        bool& aMoved, bool& bMoved) {
  unsigned long long pending = __ballot(inCell);
  for (;;) {
    bool hit = false;
    if ((pending >> lane) & 1ull) {  // the overlap test of visit(), on the live states
      const float dx = b.px - a.px, dy = b.py - a.py, dz = b.pz - a.pz;
      const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
      hit = a.r + b.r - dist > 0.0f;
    }
    const unsigned long long hm = __ballot(hit);
    const uint32_t first = hm ? static_cast<uint32_t>(__builtin_ctzll(hm)) : 64u;
    if (selfAt != kTurnDone && selfAt <= first) {  // everything below the node's own place has missed: it meets itself
      if (a.r + a.r > 0.0f) {  // (visit()'s test: the distance to itself is 0)
        NodeState o = a;
        visit_wide(a, o, true, friction, staticThreshold, lane);
        ++hits;
        aMoved = true;
      }
      pending = selfAt >= 64u ? 0ull : pending & ~((1ull << selfAt) - 1ull);
      selfAt = kTurnDone;
      continue;  // (its state may have changed: the lanes above test again)
    }
    if (first >= 64u) break;
    NodeState o = lane_node(b, first);
    visit_wide(a, o, false, friction, staticThreshold, lane);
    if (lane == static_cast<int>(first)) { b = o; bMoved = true; }
    ++hits;
    aMoved = true;
    pending = first >= 63u ? 0ull : pending & ~((2ull << first) - 1ull);
  }
}

// the members of a finished turn move on: `j` (lane-held, valid where have) to its next event; a node whose turn has all its
// members waiting for it goes to the next frontier
PIES_DEV void turn_advance(const PairArrays& P, bool have, uint32_t j, uint32_t round, uint32_t sub, int lane) {
  uint32_t ready = kTurnDone;
  if (have) {
    const uint4 r = load_rec(P.node, j);
    const uint32_t d = r.y & 0xffffu, below = r.y >> 16, t = r.z + 1u;
    const uint32_t nxt = turn_event_node(P, j, r.x, d, below, t);
    store_rec(P.node, j, make_uint4(r.x, r.y, t, nxt));
    if (nxt != kTurnDone && atomicSub(&P.turnCnt[nxt], 1u) == 1u) ready = nxt;
  }
  frontier_append(P, round, sub, lane, ready != kTurnDone, ready);
}

// the turn of node i, by one wavefront; returns the visits it resolved
PIES_DEV uint32_t run_turn(const HashArrays& H, const PairArrays& P, uint32_t i, float scale, float friction, float staticThreshold, uint32_t round,
                           uint32_t sub, int lane) {
  float4* node = P.node;
  const uint4 ri = load_rec(node, i);
  const uint32_t off = ri.x, d = ri.y & 0xffffu, below = ri.y >> 16;
  NodeState a = load_node(node, i);
  const int4 rgi = H.rng[i];
  int mx, my, mz;
  uint32_t lx, ly, lz;
  if (!node_range(a.px, a.py, a.pz, a.r, scale, mx, my, mz, lx, ly, lz)) {  // (the sequential loop stops there, Solver.cpp's would not: latched)
    if (lane == 0) atomicOr(&H.counters[kCounterFlags], kFailNonFinite);
    lx = ly = lz = 0;
  }
  const uint32_t ncell = lx * ly * lz;
  // (a node that was inserted with an empty - over-long - range has no list; should its live range hold cells, the lists cannot serve)
  if (ncell != 0u && (rgi.w & 0xffffff) == 0 && lane == 0) atomicOr(&P.ctl[kPairFlags], 1u);
  uint32_t hits = 0;
  bool aMoved = false;
  if (d < 64u) {  // the partners in the lanes' registers for the whole turn (lane d: the node itself, for the bookkeeping behind the turn)
    const bool have = static_cast<uint32_t>(lane) < d;
    const uint32_t j = have ? P.nbr[off + lane] & kPairNodeMask : 0u;
    NodeState b = have ? load_node(node, j) : NodeState{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int4 rgj = have ? H.rng[j] : make_int4(0, 0, 0, 0);
    // (the build-time positions and the excursions so far of the members, for the bookkeeping behind the turn: requested now -
    // behind the turn a load and a returning atomic were two more dependent round trips; a member belongs to this turn alone
    // for the whole level, so its excursion is read and written plainly)
    const uint32_t mj0 = have ? j : i;
    const float4 p0m = static_cast<uint32_t>(lane) <= d ? node[4u * mj0 + 2u] : make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t excm = static_cast<uint32_t>(lane) <= d ? P.exc[mj0] : 0u;
    // what the members need when the turn is over - their records (the same cache line as their state) and the nodes whose turns
    // their NEXT events are - is requested now, beside the states: behind the turn these would be two more dependent round trips
    const bool member = static_cast<uint32_t>(lane) <= d;
    const uint32_t mj = have ? j : i;
    const uint4 mr = member ? (have ? load_rec(node, j) : ri) : make_uint4(0u, 0u, 0u, 0u);
    const uint32_t mnext = member ? turn_event_node(P, mj, mr.x, mr.y & 0xffffu, mr.y >> 16, mr.z + 1u) : kTurnDone;
    bool bMoved = false;
    for (uint32_t c = 0; c < ncell; ++c) {  // dz fastest (SpatialHash.h:108-125)
      const int cx = mx + static_cast<int>(c / (lz * ly)), cy = my + static_cast<int>((c / lz) % ly), cz = mz + static_cast<int>(c % lz);
      turn_cell(a, b, have && cell_in_range(rgj, cx, cy, cz), cell_in_range(rgi, cx, cy, cz) ? below : kTurnDone, lane, friction, staticThreshold,
                hits, aMoved, bMoved);
    }
    if (bMoved) {
      store_node(node, j, b);
      note_excursion_owned(P, j, b, p0m, excm);
    }
    if (aMoved && static_cast<uint32_t>(lane) == d) {  // (lane d holds the node's own build-time position and excursion)
      store_node(node, i, a);
      note_excursion_owned(P, i, a, p0m, excm);
    }
    // every member moves on to its next event; a node whose turn has all its members waiting for it goes to the next frontier
    uint32_t ready = kTurnDone;
    if (member) {
      store_rec(node, mj, make_uint4(mr.x, mr.y, mr.z + 1u, mnext));
      if (mnext != kTurnDone && atomicSub(&P.turnCnt[mnext], 1u) == 1u) ready = mnext;
    }
    frontier_append(P, round, sub, lane, ready != kTurnDone, ready);
    return hits;
  } else {  // a dense neighbourhood: 64 partners at a time, their states through memory (a partner sits in one batch)
    for (uint32_t c = 0; c < ncell; ++c) {
      const int cx = mx + static_cast<int>(c / (lz * ly)), cy = my + static_cast<int>((c / lz) % ly), cz = mz + static_cast<int>(c % lz);
      const bool selfIn = cell_in_range(rgi, cx, cy, cz);
      for (uint32_t base = 0; base < d; base += 64u) {
        const bool have = base + static_cast<uint32_t>(lane) < d;
        const uint32_t j = have ? P.nbr[off + base + lane] & kPairNodeMask : 0u;
        NodeState b = have ? load_node(node, j) : NodeState{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int4 rgj = have ? H.rng[j] : make_int4(0, 0, 0, 0);
        bool bMoved = false;
        // the node's own place: before lane below - base of the batch that holds it, behind the last batch when every partner is below
        uint32_t selfAt = kTurnDone;
        if (selfIn && below >= base && (below < base + 64u || (below == d && base + 64u >= d))) selfAt = below - base;
        turn_cell(a, b, have && cell_in_range(rgj, cx, cy, cz), selfAt, lane, friction, staticThreshold, hits, aMoved, bMoved);
        if (bMoved) {
          store_node(node, j, b);
          note_excursion(P, j, b, node[4u * j + 2u]);
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
    if (aMoved && lane == 0) {
      store_node(node, i, a);
      note_excursion(P, i, a, node[4u * i + 2u]);
    }
    for (uint32_t base = 0; base < d; base += 64u) {
      const bool have = base + static_cast<uint32_t>(lane) < d;
      turn_advance(P, have, have ? P.nbr[off + base + lane] & kPairNodeMask : 0u, round, sub, lane);
    }
  }
  turn_advance(P, lane == 0, i, round, sub, lane);  // the node itself: on to its first partner above it
  return hits;
}

// the first events: every node tells the node whose turn its first event is that it is waiting; turns with all members waiting
// make the first frontier (the lists of round 2: round 1 means "every node" to frontier_view)
__global__ void __launch_bounds__(kBlock) k_turn_first(HashArrays H, PairArrays P, uint32_t repeat) {
  if (repeat && !P.ctl[kPairRetry]) return;
  if (H.counters[kCounterFlags]) return;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint32_t ready = kTurnDone;
  if (i < P.n) {
    const uint32_t f = load_rec(P.node, i).w;
    if (f != kTurnDone && atomicSub(&P.turnCnt[f], 1u) == 1u) ready = f;
  }
  frontier_append(P, 1u, ((blockIdx.x * kBlock + threadIdx.x) >> 6) % kPairLists, lane, ready != kTurnDone, ready);  // (round 1 appends to round 2's lists)
}

// one level: the turns of the frontier of `round`, one wavefront each (the caller's is wavefront `first` of the launch's `waves`);
// returns the visits the wavefront's turns resolved
PIES_DEV uint32_t turn_level(const HashArrays& H, const PairArrays& P, float scale, float friction, float staticThreshold, uint32_t round,
                             const FrontierView& view, uint32_t first, uint32_t waves, int lane) {
  uint32_t hits = 0;
  for (uint32_t e = first; e < view.total; e += waves) {  // (wavefront uniform)
    const uint32_t i = frontier_node(P, view, round, e);
    hits += run_turn(H, P, i, scale, friction, staticThreshold, round, e % kPairLists, lane);
  }
  return hits;
}

__global__ void __launch_bounds__(kTurnBlock) k_turn_round(HashArrays H, PairArrays P, float scale, float friction, float staticThreshold, uint32_t round,
                                                           uint32_t repeat) {
  if (!pass_guard(H, P, repeat, false)) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const FrontierView view = frontier_view(P, round, lane);
  level_open(P, round, round - 1u, repeat, view, false);
  if (view.total == 0u) return;
  count_wave_hits(P, turn_level(H, P, scale, friction, staticThreshold, round, view, blockIdx.x * (kTurnBlock / 64u) + static_cast<uint32_t>(wv),
                                gridDim.x * (kTurnBlock / 64u), lane), lane);
}

// whatever levels are left after the captured launches (and all levels of a repeated pass): one workgroup, a workgroup barrier
// where the levels have a kernel boundary (slow, never wrong)
__global__ void __launch_bounds__(1024) k_turn_tail(HashArrays H, PairArrays P, float scale, float friction, float staticThreshold, uint32_t round,
                                                    uint32_t repeat) {
  if (!pass_guard(H, P, repeat, true)) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t hits = finish_levels(
      P, round, true, repeat,
      [&](uint32_t r, const FrontierView& view) { return turn_level(H, P, scale, friction, staticThreshold, r, view, static_cast<uint32_t>(wv), blockDim.x / 64u, lane); },
      WorkgroupBarrier{});
  count_wave_hits(P, hits, lane);
}

// The same with resident workgroups and a grid barrier between the levels: a pass deeper than the captured launches no longer
// finishes on one compute unit, and a repeated pass runs here whole.
__global__ void __launch_bounds__(kTurnBlock) k_turn_finish(HashArrays H, PairArrays P, float scale, float friction, float staticThreshold, uint32_t round,
                                                            uint32_t repeat) {
  if (!pass_guard(H, P, repeat, true)) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t passed = 0;
  const uint32_t hits = finish_levels(
      P, round, true, repeat,
      [&](uint32_t r, const FrontierView& view) {
        return turn_level(H, P, scale, friction, staticThreshold, r, view, blockIdx.x * (kTurnBlock / 64u) + static_cast<uint32_t>(wv),
                           gridDim.x * (kTurnBlock / 64u), lane);
      },
      [&] { return pair_grid_barrier(P.ctl + kPairBarrier, gridDim.x, passed); });
  count_wave_hits(P, hits, lane);
}

uint32_t launch_collide_turns(hipStream_t st, const HashArrays& H, const PairArrays& Pin, const NodeArrays& nd, float gridSpacing, float friction,
                              float staticThreshold, uint32_t rounds) {
  if (nd.n == 0) return 0;
  PairArrays P = Pin;
  P.byIndex = 1u;
  const uint32_t n = nd.n;
  // a level of BASELINE config 4 holds a few hundred turns: one wavefront each
  const dim3 level(std::max<uint32_t>(1u, std::min<uint32_t>(1024u, (n / 64u + kTurnBlock / 64u) / (kTurnBlock / 64u))));
  uint32_t launches = pass_begin(st, H, P, nd, friction, staticThreshold);
  for (uint32_t repeat = 0; repeat < 2; ++repeat) {
    launches += pass_lists(st, H, P, friction, staticThreshold, repeat);
    hipLaunchKernelGGL(k_turn_first, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, H, P, repeat); ++launches;
    // (a repeated pass - rare: a node left its slack and an unlisted pair may have touched - runs all its levels in the tail kernel)
    // PIES_TURN_LEVEL_LAUNCHES=0: no captured level launches at all - every level behind the grid barrier
    uint32_t captured = repeat ? 0u : rounds;
    if (const char* e = tuning_env("PIES_TURN_LEVEL_LAUNCHES"); e && e[0] == '0') captured = 0u;
    for (uint32_t r = 2; r < 2u + captured; ++r) {
      hipLaunchKernelGGL(k_turn_round, level, dim3(kTurnBlock), 0, st, H, P, gridSpacing, friction, staticThreshold, r, repeat); ++launches;
    }
    const uint32_t residentFinish = resident_blocks_halved(reinterpret_cast<const void*>(k_turn_finish), kTurnBlock);
    // PIES_TURN_FINISH_BLOCKS: workgroups behind the grid barrier (a level of config 4 holds ~460 turns, one wavefront each; measured with every level behind the barrier: 512 workgroups 293 ms per tick, 128: 217, 64: 284 - captured launches: 160-172); 0 (diagnostics): the single workgroup of k_turn_tail, which otherwise runs only where no resident count can be had
    const uint32_t finishCap = tuning_uint("PIES_TURN_FINISH_BLOCKS", 0, 4096, 128u);
    const uint32_t finishBlocks = std::min<uint32_t>(std::min<uint32_t>(finishCap, residentFinish), level.x);
    if (finishBlocks) { hipLaunchKernelGGL(k_turn_finish, dim3(finishBlocks), dim3(kTurnBlock), 0, st, H, P, gridSpacing, friction, staticThreshold, 2u + captured, repeat); ++launches; }
    else { hipLaunchKernelGGL(k_turn_tail, dim3(1), dim3(1024), 0, st, H, P, gridSpacing, friction, staticThreshold, 2u + captured, repeat); ++launches; }
    launches += pass_end(st, H, P, nd, gridSpacing, friction, staticThreshold, repeat);
  }
  return launches;
}

}  // namespace pies
