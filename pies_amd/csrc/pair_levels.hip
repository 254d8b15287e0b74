// Node-node resolve of the PBD substep (Src/Solver.cpp:85-130) in the PAIR ORDER.
//
// The reference's loop lets node i meet node j once per grid cell both were inserted into, in each direction, itself
// included (quirk Q3), and resolves every overlapping meeting at once.  The result depends on the order of the meetings
// that share a node and on nothing else.  The pair order keeps every meeting and re-orders them pair by pair:
//   1. every node's meetings with itself (one per cell of its range);
//   2. the unordered pairs {i < j} whose inserted ranges share m > 0 cells, in ascending order of pair_key (a class from the
//      pair's direction and place when the grid was built - pairs of one class seldom share a node -, then a 64-bit mix of
//      the two indices: a total order), each as m visits of i to j followed by m visits of j to i.  Every visit tests the live
//      positions, like the reference's.
// The oracle replays exactly this with a sort and a sequential loop (FLAG_COLLISION_RULE = 2).  On the device the order is
// executed by dependency levels: a pair's turn comes when it is the next unprocessed pair in the key-sorted lists of BOTH
// its nodes, and the pairs whose turn has come share no node, so a level is one data-parallel launch.  The classed key keeps the chains short: 30-45 levels for the 3-4 M pairs of
// BASELINE config 4 (60-80 with the hash alone), against 27 passes x 350 dependent visits per group in the group order.
// (the lists and their filter: pair_lists.hip)
#include <algorithm>

#include "pair_device.h"

namespace pies {

// the visits of a taken pair {x, y} in one lane (rx: x's record): those of the lower node to the higher one, then as many back;
// returns the visits that resolved
PIES_DEV uint32_t visit_pair(const PairArrays& P, uint32_t x, uint32_t y, const uint4 rx, float friction, float staticThreshold) {
  float4* node = P.node;
  const bool xLow = x < y;
  const uint32_t lo = xLow ? x : y, hi = xLow ? y : x;
  NodeState a = load_node(node, lo), b = load_node(node, hi);
  const float dx = b.px - a.px, dy = b.py - a.py, dz = b.pz - a.pz;
  const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
  if (!(a.r + b.r - dist > 0.0f)) return 0u;
  const float4 a0 = node[4u * lo + 2u], b0 = node[4u * hi + 2u];
  const uint32_t m = P.nbrM ? P.nbrM[rx.x + (rx.z & 0xffffu)] : (rx.w >> 28) + 1u;  // (wide ranges keep the count beside the entry)
  uint32_t h = 0;
  for (uint32_t t = 0; t < m; ++t) h += visit(a, b, friction, staticThreshold) ? 1u : 0u;
  for (uint32_t t = 0; t < m; ++t) h += visit(b, a, friction, staticThreshold) ? 1u : 0u;
  store_node(node, lo, a);
  store_node(node, hi, b);
  note_excursion(P, lo, a, a0);
  note_excursion(P, hi, b, b0);
  return h;
}

// one level with a lane per frontier node, by the wavefronts that call (`first`: the lane's position in the frontier in the first
// turn of the loop, `step`: the positions the calling wavefronts cover per turn)
PIES_DEV uint32_t process_frontier(const HashArrays& H, const PairArrays& P, float friction, float staticThreshold, uint32_t round, uint32_t first,
                                   uint32_t step, const FrontierView& view, int lane) {
  const uint32_t count = view.total;
  uint32_t hits = 0;
  for (uint32_t base = first - static_cast<uint32_t>(lane); base < count; base += step) {  // (wave uniform trip count)
    bool moveX = false, moveY = false;
    uint32_t x = 0, y = 0;
    uint4 rx, ry;
    if (frontier_take(P, view, round, base + static_cast<uint32_t>(lane), count, x, y, rx, ry)) {
      hits += visit_pair(P, x, y, rx, friction, staticThreshold);
      moveX = move_on(P.node, x, rx, next_entry(P, rx), round & 0xffffu);
      moveY = move_on(P.node, y, ry, next_entry(P, ry), round & 0xffffu);
    }
    // the nodes that moved on and have entries left go to the sub-list this chunk is dealt to (a sub-list takes at most 128 nodes
    // from each of its chunks: frCap covers that)
    frontier_append(P, round, (base >> 6) % kPairLists, lane, moveX, x, moveY, y);
  }
  return hits;
}

// One level as a launch of 256-thread workgroups.  Half the lanes of a frontier find that they have nothing to do (the other
// node's lane takes the pair, or the partner is not there yet), and a lane that takes a pair runs up to sixteen visits of 350
// instructions while the rest of its wavefront waits - with one wavefront per workgroup the 1 125 wavefronts of a settled
// level of config 4 each carried a few such lanes, and the hundred SIMDs that got two of them set the level's time.  Here the
// workgroup's four wavefronts look at their nodes, the lanes that take a pair put it into LDS, and the pairs are dealt out
// again densely: the first wavefronts get full loads, the others leave.  Half as many wavefronts run visits, one per SIMD.
constexpr uint32_t kRoundBlock = 256;
struct TakenPair {
  uint32_t x, y;
  uint4 rx, ry;
};
__global__ void __launch_bounds__(kRoundBlock) k_pair_round(HashArrays H, PairArrays P, float friction, float staticThreshold, uint32_t round, uint32_t repeat) {
  __shared__ TakenPair taken[kRoundBlock];
  __shared__ uint32_t waveTook[kRoundBlock / 64];
  if (!pass_guard(H, P, repeat, false)) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const FrontierView view = frontier_view(P, round, lane);
  level_open(P, round, round, repeat, view, false);
  const uint32_t count = view.total;
  if (count == 0u) return;  // (a pass that will be repeated is finished all the same: it finds every node that leaves its slack)
  uint32_t hits = 0;
  for (uint32_t chunk = blockIdx.x; chunk * kRoundBlock < count; chunk += gridDim.x) {  // (workgroup uniform)
    // ---- who takes a pair
    uint32_t x = 0, y = 0;
    uint4 rx = make_uint4(0u, 0u, 0u, 0u), ry = rx;
    const bool take = frontier_take(P, view, round, chunk * kRoundBlock + threadIdx.x, count, x, y, rx, ry);
    // ---- the taken pairs, densely
    const unsigned long long tm = __ballot(take);
    if (lane == 0) waveTook[wv] = static_cast<uint32_t>(__popcll(tm));
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kRoundBlock / 64; ++w) {
      const uint32_t c = waveTook[w];
      if (w < static_cast<uint32_t>(wv)) before += c;
      total += c;
    }
    if (take) taken[before + static_cast<uint32_t>(__popcll(tm & ((1ull << lane) - 1ull)))] = TakenPair{x, y, rx, ry};
    __syncthreads();
    // ---- the visits
    bool moveX = false, moveY = false;
    if (threadIdx.x < total) {
      const TakenPair t = taken[threadIdx.x];
      x = t.x; y = t.y;
      hits += visit_pair(P, x, y, t.rx, friction, staticThreshold);
      moveX = move_on(P.node, x, t.rx, next_entry(P, t.rx), round & 0xffffu);
      moveY = move_on(P.node, y, t.ry, next_entry(P, t.ry), round & 0xffffu);
    }
    // the nodes that moved on and have entries left go to the sub-list this wavefront's chunk is dealt to (a sub-list takes at
    // most 128 nodes from each of its chunks: frCap covers that)
    if (static_cast<uint32_t>(wv) * 64u < total)  // (wavefront uniform)
      frontier_append(P, round, (chunk * (kRoundBlock / 64) + static_cast<uint32_t>(wv)) % kPairLists, lane, moveX, x, moveY, y);
    __syncthreads();  // (the table is reused by the next chunk)
  }
  count_hits(P, hits, lane);
}

// ---- the same level with FOUR LANES PER PAIR (round 5) ---------------------------------------------------------------------
// A lane that takes a pair runs up to sixteen visits of ~350 instructions - fifteen correctly rounded divisions each - while a level
// waits for its slowest lane.  Here a pair is taken by a quad of lanes, lane k holding component k of the positions and velocities
// (lane 3 idles along with a copy of component 0): the three sums of a visit (|d|^2, r.u, |q|^2) are quad permutes (v_mov_dpp) added
// in visit()'s order, every lane divides for its own component only - five divisions instead of fifteen, ~120 instructions
// instead of ~350 -, same operations on the same operands: the bits of visit().  A workgroup looks at 64 frontier nodes (its first
// wavefront), the pairs taken go through LDS, and all four wavefronts run their visits.
// Measured on BASELINE config 4: a settled frame 9.16 -> 8.76-8.9 ms (burst window 71.8 -> 73.0 substeps/s): a third of the
// instructions in the slowest lane bought 4 %, because the levels are bound by the NUMBER of wavefront instructions issued (per-level
// counters: profiles/r05_levels_pmc_config4_before.txt), and a quad wavefront holds 16 pairs where a lane-per-pair one holds 64: what
// pays is full wavefronts of quads with equal numbers of visits - the sorted table of pair_level4.
constexpr uint32_t kQuadNodes = 64;     // frontier nodes a wavefront looks at per turn of a workgroup's loop
constexpr uint32_t kQuadLookMax = 4;    // wavefronts of a workgroup that look (PIES_PAIR_LOOK_WAVES: 1, 2 or 4): the table holds 64 pairs for each
constexpr uint32_t kQuadBins = 9;       // pairs by visits per side: 8 and more ... 1, and the ones that do not overlap
struct QuadTable {
  TakenPair taken[kQuadNodes * kQuadLookMax];
  uint32_t bins[64];  // [bin * look + wavefront] (9 x 4 used)
};
// one level by the workgroups of the calling launch (all threads of a workgroup call: barriers); T: the workgroup's LDS; look: the
// wavefronts of the workgroup that look at frontier nodes (at most blockDim.x / 64)
PIES_DEV uint32_t pair_level4(const HashArrays& H, const PairArrays& P, float friction, float staticThreshold, uint32_t round, const FrontierView& view,
                              QuadTable& T, uint32_t look) {
  uint32_t hits = 0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t count = view.total;
  float4* node = P.node;
  const uint32_t stampNow = round & 0xffffu;
  const int k = lane & 3;
  const uint32_t per = kQuadNodes * look;  // frontier nodes per turn
  TakenPair* taken = T.taken;
  for (uint32_t chunk = blockIdx.x; chunk * per < count; chunk += gridDim.x) {  // (workgroup uniform)
    // ---- who takes a pair: the first wavefronts look at the chunk's frontier nodes, 64 each
    bool take = false;
    uint32_t x = 0, y = 0, key = 0, rank = 0;
    uint4 rx = make_uint4(0u, 0u, 0u, 0u), ry = rx;
    if (static_cast<uint32_t>(wv) < look) {
      take = frontier_take(P, view, round, chunk * per + static_cast<uint32_t>(wv) * kQuadNodes + static_cast<uint32_t>(lane), count, x, y, rx, ry);
      // The pairs go into the table sorted: the ones that overlap first, by descending number of shared cells (= visits from either
      // side), the ones that do not (most, once a pile has settled: they only move on) last.  A wavefront of the visits runs as long
      // as its busiest quad, and the level launches of config 4 turned out to be bound by VALU issue (profiles/
      // r05_levels_pmc_config4.txt: 20 M wavefront instructions in level 1, SQ_ACTIVE_INST_ANY x 8 resident wavefronts > a SIMD's
      // cycles): in arrival order a wavefront's sixteen pairs held ~6 overlapping ones with 1-8 shared cells each.  The overlap test
      // is visit()'s own (same operands, same order), on lines the records' loads have just brought in.
      if (take) {
        const bool xLow = x < y;
        const uint32_t lo = xLow ? x : y, hi = xLow ? y : x;
        const float4 ap = node[4u * lo], av = node[4u * lo + 1u], bp = node[4u * hi], bv = node[4u * hi + 1u];
        const float dx = bp.x - ap.x, dy = bp.y - ap.y, dz = bp.z - ap.z;
        const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
        if (av.w + bv.w - dist > 0.0f) {
          const uint32_t m = P.nbrM ? P.nbrM[rx.x + (rx.z & 0xffffu)] : (rx.w >> 28) + 1u;
          key = min(m, kQuadBins - 1u);
        }
      }
      // (bin b of the table = key kQuadBins - 1 - b: descending; the counts lie bin by bin, wavefront by wavefront: the table's order)
#pragma unroll
      for (uint32_t b = 0; b < kQuadBins; ++b) {
        const bool mine = take && key == kQuadBins - 1u - b;
        const unsigned long long mk = __ballot(mine);
        if (mine) rank = static_cast<uint32_t>(__popcll(mk & ((1ull << lane) - 1ull)));
        if (lane == 0) T.bins[b * look + static_cast<uint32_t>(wv)] = static_cast<uint32_t>(__popcll(mk));
      }
    }
    __syncthreads();
    // a pair's place: the pairs of the bins before its own, its bin's pairs of the wavefronts before its own, the lanes before it -
    // a prefix sum over the 9 x look counts, one per lane
    uint32_t total, nOv;  // pairs taken; the ones of them that overlap (they come first)
    {
      const uint32_t cells = kQuadBins * look;
      const uint32_t c = static_cast<uint32_t>(lane) < cells ? T.bins[lane] : 0u;
      uint32_t incl = c;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
      }
      total = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(incl), 63));
      nOv = static_cast<uint32_t>(__shfl(incl, static_cast<int>((kQuadBins - 1u) * look - 1u), 64));
      const uint32_t mine = (kQuadBins - 1u - key) * look + min(static_cast<uint32_t>(wv), look - 1u);
      const uint32_t at = static_cast<uint32_t>(__shfl(incl - c, static_cast<int>(mine), 64));
      if (take) taken[at + rank] = TakenPair{x, y, rx, ry};
    }
    __syncthreads();
    // the nodes of a wavefront's pairs that moved on and have entries left go to the sub-list their 64 places of the table are dealt
    // to (at most 128 nodes for every 64 frontier nodes looked at: frCap covers that)
    auto append = [&](bool moveX, bool moveY, uint32_t x, uint32_t y, uint32_t place) {
      frontier_append(P, round, (chunk * look + (place >> 6)) % kPairLists, lane, moveX, x, moveY, y);
    };
    // ---- the visits: the workgroup's quads take the overlapping pairs, blockDim.x / 4 at a time (a workgroup of one wavefront: 16; of four: 64)
    const uint32_t quads = blockDim.x >> 2;
    for (uint32_t q0 = 0; q0 < nOv; q0 += quads) {  // (workgroup uniform)
      const uint32_t q = q0 + (threadIdx.x >> 2);
      bool moveX = false, moveY = false;
      uint32_t x = 0, y = 0;
      if (q < nOv) {
        const TakenPair t = taken[q];
        x = t.x; y = t.y;
        const bool xLow = x < y;
        const uint32_t lo = xLow ? x : y, hi = xLow ? y : x;
        // everything the pair may need is requested at once (one round trip instead of four dependent ones: the positions the
        // lists were built from, the excursions so far and the next list entries used to be fetched when they were needed)
        const float4 ap = node[4u * lo], av = node[4u * lo + 1u], bp = node[4u * hi], bv = node[4u * hi + 1u];
        const float4 a0 = node[4u * lo + 2u], b0 = node[4u * hi + 2u];
        const uint32_t ea = P.exc[lo], eb = P.exc[hi];  // (a node is in one pair of a level: nobody else touches its excursion now)
        const uint32_t nextX = next_entry_clamped(P, t.rx), nextY = next_entry_clamped(P, t.ry);
        QuadNode a{comp4(ap, k), comp4(av, k), ap.w, av.w}, b{comp4(bp, k), comp4(bv, k), bp.w, bv.w};
        const float d = b.p - a.p;
        const float dist = sqrtf(quad_sum3(d * d));
        if (a.r + b.r - dist > 0.0f) {
          const uint32_t m = P.nbrM ? P.nbrM[t.rx.x + (t.rx.z & 0xffffu)] : (t.rx.w >> 28) + 1u;  // (wide ranges keep the count beside the entry)
          uint32_t h = 0;
          for (uint32_t v = 0; v < m; ++v) h += visit_quad(a, b, k, friction, staticThreshold) ? 1u : 0u;
          for (uint32_t v = 0; v < m; ++v) h += visit_quad(b, a, k, friction, staticThreshold) ? 1u : 0u;
          // the quad's first lane puts the components together and stores the two nodes
          const float apy = quad_lane(a.p, 1), apz = quad_lane(a.p, 2), avy = quad_lane(a.v, 1), avz = quad_lane(a.v, 2);
          const float bpy = quad_lane(b.p, 1), bpz = quad_lane(b.p, 2), bvy = quad_lane(b.v, 1), bvz = quad_lane(b.v, 2);
          if (k == 0) {
            const NodeState na{a.p, apy, apz, a.w, a.v, avy, avz, a.r}, nb{b.p, bpy, bpz, b.w, b.v, bvy, bvz, b.r};
            store_node(node, lo, na);
            store_node(node, hi, nb);
            note_excursion_owned(P, lo, na, a0, ea);
            note_excursion_owned(P, hi, nb, b0, eb);
            hits += h;
          }
        }
        if (k == 0) {
          moveX = move_on(node, x, t.rx, nextX, stampNow);
          moveY = move_on(node, y, t.ry, nextY, stampNow);
        }
      }
      const uint32_t first = q0 + static_cast<uint32_t>(wv) * 16u;  // the wavefront's sixteen places of the table
      if (first < nOv) append(moveX, moveY, x, y, first);  // (wavefront uniform)
    }
    // ---- the pairs that do not overlap only move on: a lane each, the table's 64-places at a time (the first of them may begin
    //      with overlapping pairs: the quads had those)
    for (uint32_t base = (nOv & ~63u) + static_cast<uint32_t>(wv) * 64u; base < total; base += blockDim.x) {  // (wavefront uniform)
      const uint32_t p = base + static_cast<uint32_t>(lane);
      bool moveX = false, moveY = false;
      uint32_t x = 0, y = 0;
      if (p >= nOv && p < total) {
        const TakenPair t = taken[p];
        x = t.x; y = t.y;
        const uint32_t nextX = next_entry_clamped(P, t.rx), nextY = next_entry_clamped(P, t.ry);
        moveX = move_on(node, x, t.rx, nextX, stampNow);
        moveY = move_on(node, y, t.ry, nextY, stampNow);
      }
      append(moveX, moveY, x, y, base);
    }
    __syncthreads();  // (the table is reused by the next chunk)
  }
  return hits;
}

// as many looking wavefronts as it takes to give every workgroup of the launch one turn (a small frontier in chunks of 256 would
// leave most compute units idle: the levels 26-36 of a settled pass of config 4 took 20 us instead of 14)
PIES_DEV uint32_t looking_waves(const FrontierView& view) {
  return max((view.total + kQuadNodes * gridDim.x - 1u) / (kQuadNodes * gridDim.x), 1u);
}

__global__ void __launch_bounds__(kRoundBlock) k_pair_round4(HashArrays H, PairArrays P, float friction, float staticThreshold, uint32_t round, uint32_t repeat,
                                                             uint32_t look) {
  __shared__ QuadTable table;
  if (!pass_guard(H, P, repeat, false)) return;
  const int lane = threadIdx.x & 63;
  const FrontierView view = frontier_view(P, round, lane);
  level_open(P, round, round, repeat, view, false);
  if (view.total == 0u) return;
  count_hits(P, pair_level4(H, P, friction, staticThreshold, round, view, table, min(look, looking_waves(view))), lane);
}

// ---- the levels of a REPEATED pass in one launch ----------------------------------------------------------------------------------
// A pass is repeated when a node left its slack and an unlisted pair may have touched: twice in the first three ticks of BASELINE
// config 4, never afterwards.  Until round 5 every pass captured its repeat's level launches all the same - half as many again as
// the first attempt's, 72 per settled pass of config 4, each returning on the "no repeat" word for the price of its dispatch (0.7 ms
// of a 9-ms tick).  Now the repeat's levels are ONE launch: its workgroups - all resident - run level after level with a grid
// barrier where the captured launches have a kernel boundary (release, counter, bounded wait, acquire: the CG continuation's
// barrier, pd_cg_device.h), slower per level than a launch and run twice in a simulation's life.  A wait that times out hands the
// pass to the sequential loop (flag 2).
// (repeat = 0: the same launch as the TAIL of the first attempt - whatever levels are left behind the captured launches, from
// `firstRound` on.  Until round 5 that was one workgroup (k_pair_tail): a pass deeper than the captured count - the first ticks of a
// scene, a pile that forms between two looks of the host - ran its surplus levels on one compute unit, ten times slower than the
// launches (config 4 pinned at 48 captured levels: 8 substeps/s instead of 100).)
__global__ void __launch_bounds__(kRoundBlock) k_pair_repeat(HashArrays H, PairArrays P, float friction, float staticThreshold, uint32_t firstRound,
                                                             uint32_t repeat) {
  __shared__ QuadTable table;
  if (!pass_guard(H, P, repeat, true)) return;
  uint32_t passed = 0;
  const uint32_t hits = finish_levels(
      P, firstRound, false, repeat,
      [&](uint32_t round, const FrontierView& view) {
        return pair_level4(H, P, friction, staticThreshold, round, view, table, min(kQuadLookMax, looking_waves(view)));
      },
      [&] { return pair_grid_barrier(P.ctl + kPairBarrier, gridDim.x, passed); });
  count_hits(P, hits, threadIdx.x & 63);
}

// The same on ONE workgroup, a lane per pair: where no workgroup count could be had for the grid barrier, or lanes per pair is
// what was asked for (PIES_PAIR_QUADS=0, PIES_PAIR_REPEAT_LAUNCHES=1).
__global__ void __launch_bounds__(1024) k_pair_tail(HashArrays H, PairArrays P, float friction, float staticThreshold, uint32_t round, uint32_t repeat) {
  if (!pass_guard(H, P, repeat, true)) return;
  const int lane = threadIdx.x & 63;
  const uint32_t hits = finish_levels(
      P, round, false, repeat,
      [&](uint32_t r, const FrontierView& view) { return process_frontier(H, P, friction, staticThreshold, r, threadIdx.x, blockDim.x, view, lane); },
      WorkgroupBarrier{});
  count_hits(P, hits, lane);
}

uint32_t launch_collide_pairs(hipStream_t st, const HashArrays& H, const PairArrays& P, const NodeArrays& nd, float gridSpacing, float friction,
                              float staticThreshold, uint32_t rounds) {
  if (nd.n == 0) return 0;
  const uint32_t n = nd.n;
  // workgroups of a level launch: a settled level of config 4 has ~280 chunks of frontier nodes, and 60 % of the captured level
  // launches find nothing to do (the repeat's, and the spare ones of the first attempt) - an empty launch costs what its dispatch
  // costs.  Measured on config 4 (burst / settled substeps/s): cap 256: 55.5 / 76.3, 512: 66.7 / 91.3, 1 024: 68.2 / 97.3, 2 048 (rounds
  // 3's): 65.3 / 94.2.  PIES_PAIR_LEVEL_BLOCKS sets the cap (chunks beyond it are taken in a grid-stride loop).
  const uint32_t levelCap = tuning_uint("PIES_PAIR_LEVEL_BLOCKS", 1, 65535, 1024u);
  const dim3 level(std::max<uint32_t>(1u, std::min<uint32_t>(levelCap, (n + kRoundBlock - 1u) / kRoundBlock)));
  // the level launches of the REPEAT almost always find "no repeat" and return: a small grid makes that cheap (a repeat that does
  // run takes its frontier in a grid-stride loop)
  const uint32_t repeatCap = tuning_uint("PIES_PAIR_REPEAT_BLOCKS", 1, 65535, levelCap);
  const dim3 levelRepeat(std::max<uint32_t>(1u, std::min<uint32_t>(repeatCap, level.x)));
  // four lanes per pair (k_pair_round4): a workgroup takes 64 frontier nodes per round of its loop; PIES_PAIR_QUADS=0: one lane per pair
  bool quads = true;
  if (const char* e = tuning_env("PIES_PAIR_QUADS")) quads = e[0] != '0';
  // threads of a level's workgroups (PIES_PAIR_QUAD_THREADS: 64, 128 or 256): a workgroup looks at 64 frontier nodes per turn of its
  // loop whatever its size, and as many workgroups as the chip holds at once take part (8 of 256 threads per compute unit).
  // Measured on config 4 (burst / settled), before the table was sorted: 256: 75.6 / 109.9, 128: 68.8 / 102.0, 64: 63.4 / 94.3 - more,
  // smaller workgroups put every chunk of a level in flight at once and were slower, and requesting all of a pair's operands at once
  // (one round trip instead of four) changed nothing (75.2 / 109.1): a level is bound by VALU issue, not by its round trips.
  uint32_t threads4 = tuning_uint("PIES_PAIR_QUAD_THREADS", 64, 256, kRoundBlock);
  if (threads4 != 64u && threads4 != 128u) threads4 = kRoundBlock;
  // (measured on config 4 with 256 threads and the sorted table, burst / settled substeps/s: 512: 81 / 116, 768: 87 / 121, 1 024: 90 / 127, 1 536: 86 / 123, 2 048: 82 / 117)
  const uint32_t cap4 = tuning_uint("PIES_PAIR_QUAD_BLOCKS", 1, 65535, 1024u * (kRoundBlock / threads4));
  // wavefronts of a level's workgroup that look at frontier nodes, 64 each (PIES_PAIR_LOOK_WAVES: 1, 2 or 4): the pairs they take are
  // sorted by visits across the whole workgroup, so more of them make the visiting wavefronts denser and more alike
  uint32_t look4 = tuning_uint("PIES_PAIR_LOOK_WAVES", 1, 4, 4u);
  if (look4 == 3u) look4 = 4u;
  look4 = std::min(look4, threads4 / 64u);
  const dim3 level4(std::max<uint32_t>(1u, std::min<uint32_t>(cap4, (n + kQuadNodes * look4 - 1u) / (kQuadNodes * look4))));
  const dim3 levelRepeat4(std::max<uint32_t>(1u, std::min<uint32_t>(repeatCap, level4.x)));
  // the repeat's levels in one launch of resident workgroups (PIES_PAIR_REPEAT_LAUNCHES=1: captured level launches as in rounds 3-4)
  const uint32_t residentRepeat = resident_blocks_halved(reinterpret_cast<const void*>(k_pair_repeat), kRoundBlock);
  uint32_t repeatBlocks = std::min<uint32_t>(std::min<uint32_t>(512u, residentRepeat), level4.x);
  if (const char* e = tuning_env("PIES_PAIR_REPEAT_LAUNCHES"); e && e[0] == '1') repeatBlocks = 0;
  uint32_t launches = pass_begin(st, H, P, nd, friction, staticThreshold);
  for (uint32_t repeat = 0; repeat < 2; ++repeat) {
    launches += pass_lists(st, H, P, friction, staticThreshold, repeat);
    // (the repeat lists more partners and runs deeper: half as many launches again; they return at once - 2.5 us each - when
    // nothing is repeated)
    if (repeat && quads && repeatBlocks) {  // the repeat's levels: one launch (k_pair_repeat runs until the frontier is empty)
      hipLaunchKernelGGL(k_pair_repeat, dim3(repeatBlocks), dim3(kRoundBlock), 0, st, H, P, friction, staticThreshold, 1u, 1u); ++launches;
    } else if (quads && repeatBlocks) {  // the first attempt: captured level launches, then whatever is left in one launch of resident workgroups
      for (uint32_t r = 1; r <= rounds; ++r) {
        hipLaunchKernelGGL(k_pair_round4, level4, dim3(threads4), 0, st, H, P, friction, staticThreshold, r, 0u, look4);
        ++launches;
      }
      hipLaunchKernelGGL(k_pair_repeat, dim3(repeatBlocks), dim3(kRoundBlock), 0, st, H, P, friction, staticThreshold, rounds + 1u, 0u); ++launches;
    } else {
      const uint32_t captured = repeat ? rounds + rounds / 2u : rounds;
      for (uint32_t r = 1; r <= captured; ++r) {
        if (quads) hipLaunchKernelGGL(k_pair_round4, repeat ? levelRepeat4 : level4, dim3(threads4), 0, st, H, P, friction, staticThreshold, r, repeat, look4);
        else hipLaunchKernelGGL(k_pair_round, repeat ? levelRepeat : level, dim3(kRoundBlock), 0, st, H, P, friction, staticThreshold, r, repeat);
        ++launches;
      }
      hipLaunchKernelGGL(k_pair_tail, dim3(1), dim3(1024), 0, st, H, P, friction, staticThreshold, captured + 1u, repeat); ++launches;
    }
    launches += pass_end(st, H, P, nd, gridSpacing, friction, staticThreshold, repeat);
  }
  return launches;
}

}  // namespace pies
