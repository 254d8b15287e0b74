// Device code shared by the files of the node-node resolve by dependency levels (pair_lists.hip: what both orders share;
// pair_levels.hip: the pair order; pair_turns.hip: the reference's order by turns): the pair key, a node's record and the protocol
// by which the lanes of a level read and move it, excursions, the frontier and its appends, the opening of a level, the grid barrier
// and the loop that finishes the remaining levels of a pass in one launch.  (One visit, in every lane layout: pair_rule.h.)
#pragma once
#include <cstdint>

#include "dev_math.h"
#include "hash_device.h"
#include "pair_kernels.h"
#include "pair_rule.h"

namespace pies {

constexpr int kBlock = 256;
constexpr uint32_t kPairNodeMask = 0x01ffffffu;            // partner index (n < 2^25); bits 28-31 hold (shared cells - 1)
// Bits 25-27 of a record's current entry carry the low three bits of the cursor it belongs to.  A record is four words, written
// and read with one 16-byte access each, and a lane looks at the records of nodes that other lanes may be moving on in the same
// launch.  The protocol is safe with the old or the new record; an experiment that made lanes read records later in a launch
// (a lane going on to its node's next pair: half the levels, but each three times as long - dropped) showed readers that got the
// cursor / stamp word of one version with the entry word of the next.  The tag makes such a view recognisable; a reader that
// gets one leaves the pair alone, like one that finds the node moved on in this round (whoever moved it sees to it).
constexpr uint32_t kPairTagShift = 25;
PIES_DEV bool rec_consistent(const uint4& r) { return ((r.w >> kPairTagShift) & 7u) == (r.z & 7u); }

// oracle/ora_math.h: pair_key - direction class and parity of the pair from the positions the grid was built from, then
// murmur3's 64-bit finaliser over (i << 32 | j); i < j, (pix, ..) the lower node's position
PIES_DEV uint64_t pair_key(uint32_t i, uint32_t j, float pix, float piy, float piz, float pjx, float pjy, float pjz) {
  uint64_t k = (static_cast<uint64_t>(i) << 32) | j;
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  const float dx = pjx - pix, dy = pjy - piy, dz = pjz - piz;
  const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
  const float lim = 0.41421356f * fmaxf(ax, fmaxf(ay, az));
  int qx = ax > lim ? (dx < 0.0f ? -1 : 1) : 0, qy = ay > lim ? (dy < 0.0f ? -1 : 1) : 0, qz = az > lim ? (dz < 0.0f ? -1 : 1) : 0;
  const int lead = qx != 0 ? qx : (qy != 0 ? qy : qz);
  if (lead < 0) { qx = -qx; qy = -qy; qz = -qz; }
  const float fx = static_cast<float>(qx), fy = static_cast<float>(qy), fz = static_cast<float>(qz);
  const float qq = fmaxf(fx * fx + fy * fy + fz * fz, 1.0f);
  const float ui = (pix * fx + piy * fy + piz * fz) / qq, uj = (pjx * fx + pjy * fy + pjz * fz) / qq;
  const float len = fmaxf(fabsf(uj - ui), 0.001f);
  const float t = fminf(fmaxf(floorf(fminf(ui, uj) / len), -1.0e9f), 1.0e9f);
  const uint32_t parity = static_cast<uint32_t>(static_cast<long long>(t)) & 1u;
  const uint32_t cls = static_cast<uint32_t>((qx + 1) * 9 + (qy + 1) * 3 + (qz + 1)) * 2u + parity;  // < 54
  return (static_cast<uint64_t>(cls) << 58) | (k >> 6);
}

// the key of the pair {i, j} in either order of the arguments: ONE evaluation of pair_key on swapped operands (a wavefront's lanes
// hold pairs of both orders: `i < j ? pair_key(i, j, ..) : pair_key(j, i, ..)` made it run both - ~150 instructions each, a quarter
// of the list kernel's)
PIES_DEV uint64_t pair_key_of(uint32_t i, uint32_t j, float pix, float piy, float piz, float pjx, float pjy, float pjz) {
  const bool low = i < j;
  return pair_key(low ? i : j, low ? j : i, low ? pix : pjx, low ? piy : pjy, low ? piz : pjz, low ? pjx : pix, low ? pjy : piy, low ? pjz : piz);
}

// ---- the pass's own node records: 64 bytes = one cache line per node ------------------------------------------------------
//   [0] x, y, z, invMass          [1] vx, vy, vz, radius          [2] position when the grid was built (x, y, z), slack
//   [3] first list entry, entries, current entry | round in which the node got there << 16, the current entry itself
// A level touches a node through this line only (the level kernels are bound by the number of scattered memory transactions).
PIES_DEV NodeState load_node(const float4* __restrict__ node, uint32_t i) {
  const float4 p = node[4u * i], v = node[4u * i + 1u];
  return NodeState{p.x, p.y, p.z, p.w, v.x, v.y, v.z, v.w};
}
PIES_DEV void store_node(float4* node, uint32_t i, const NodeState& a) {
  node[4u * i] = make_float4(a.px, a.py, a.pz, a.w);
  node[4u * i + 1u] = make_float4(a.vx, a.vy, a.vz, a.r);
}
PIES_DEV uint4 load_rec(const float4* __restrict__ node, uint32_t i) { return reinterpret_cast<const uint4*>(node)[4u * i + 3u]; }
PIES_DEV void store_rec(float4* node, uint32_t i, uint4 r) { reinterpret_cast<uint4*>(node)[4u * i + 3u] = r; }
// a node has been moved: its excursion from the position the lists were built from (p0.xyz) is kept as a maximum; the first time
// it leaves its slack (p0.w) it is put on the list k_pair_verify works through
PIES_DEV void note_excursion(const PairArrays& P, uint32_t i, const NodeState& a, const float4 p0) {
  const float dx = a.px - p0.x, dy = a.py - p0.y, dz = a.pz - p0.z;
  const float e = sqrtf(dx * dx + dy * dy + dz * dz);
  const float thr = 0.999f * p0.w;
  const float old = __uint_as_float(atomicMax(&P.exc[i], __float_as_uint(e)));  // (non-negative floats order like their bits; NaN sorts above everything)
  if (!(e <= thr) && old <= thr) {
    const uint32_t at = atomicAdd(&P.ctl[kPairLeft], 1u);
    if (at < P.n) P.left[at] = i;
  }
}
// the same for a caller that owns the node for the whole launch step (no other lane can touch it) and has read its excursion already
PIES_DEV void note_excursion_owned(const PairArrays& P, uint32_t i, const NodeState& a, const float4 p0, uint32_t oldBits) {
  const float dx = a.px - p0.x, dy = a.py - p0.y, dz = a.pz - p0.z;
  const float e = sqrtf(dx * dx + dy * dy + dz * dz);
  const float thr = 0.999f * p0.w;
  if (__float_as_uint(e) > oldBits) P.exc[i] = __float_as_uint(e);
  if (!(e <= thr) && __uint_as_float(oldBits) <= thr) {
    const uint32_t at = atomicAdd(&P.ctl[kPairLeft], 1u);
    if (at < P.n) P.left[at] = i;
  }
}
// resolved pairs are counted per wavefront into one of kPairStripes words (k_pair_check adds them up)
PIES_DEV void count_wave_hits(const PairArrays& P, uint32_t hits, int lane) {  // (hits: the wavefront's, the same in its lanes)
  if (lane == 0 && hits) atomicAdd(&P.hitStripe[((blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) % kPairStripes) * kPairPad], hits);
}
PIES_DEV void count_hits(const PairArrays& P, uint32_t hits, int lane) {  // (hits: the lane's)
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) hits += __shfl_xor(hits, o, 64);
  count_wave_hits(P, hits, lane);
}
// A node moves on to its next list entry in the round with stamp `stampNow`: its new record (cursor + 1, the stamp, the entry
// under the cursor's tag).  nextEntry is looked at only if the node has an entry left; the caller fetches it its own way:
// next_entry when the move is decided, next_entry_clamped ahead of that - unconditional, beside the caller's other loads.
PIES_DEV uint4 moved_on(const uint4 r, uint32_t nextEntry, uint32_t stampNow) {
  const uint32_t c = (r.z & 0xffffu) + 1u;
  return make_uint4(r.x, r.y, c | (stampNow << 16), (c < r.y ? nextEntry : 0u) | ((c & 7u) << kPairTagShift));
}
PIES_DEV uint32_t next_entry(const PairArrays& P, const uint4 r) {
  const uint32_t c = (r.z & 0xffffu) + 1u;
  return c < r.y ? P.nbr[r.x + c] : 0u;
}
PIES_DEV uint32_t next_entry_clamped(const PairArrays& P, const uint4 r) { return P.nbr[r.x + min((r.z & 0xffffu) + 1u, r.y - 1u)]; }
// stores the record of moved_on; returns whether the node has entries left
PIES_DEV bool move_on(float4* node, uint32_t i, const uint4 r, uint32_t nextEntry, uint32_t stampNow) {
  store_rec(node, i, moved_on(r, nextEntry, stampNow));
  return (r.z & 0xffffu) + 1u < r.y;
}

PIES_DEV float comp4(const float4 v, int k) { return k == 1 ? v.y : (k == 2 ? v.z : v.x); }  // (a quad's lane 3: a copy of component 0)

// The frontier of a round is kept as kPairLists sub-lists.  A wavefront works on chunks of 64 consecutive positions of their
// concatenation and appends to the sub-list its chunk is dealt to (chunk index modulo kPairLists).
struct FrontierView {
  uint32_t incl;   // lane s: entries of sub-lists 0 .. s
  uint32_t total;
};
PIES_DEV FrontierView frontier_view(const PairArrays& P, uint32_t round, int lane) {
  FrontierView v;
  if (round == 1u) { v.incl = 0; v.total = P.n; return v; }  // (all nodes, by index)
  uint32_t c = min(__hip_atomic_load(&P.frCount[((round % 3u) * kPairLists + static_cast<uint32_t>(lane)) * kPairPad], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), P.frCap);
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(c, off, 64);
    if (lane >= off) c += t;
  }
  v.incl = c;
  v.total = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(c), 63));
  return v;
}
// position e of the concatenated sub-lists -> the node (e < total)
PIES_DEV uint32_t frontier_node(const PairArrays& P, const FrontierView& v, uint32_t round, uint32_t e) {
  if (round == 1u) return e;
  uint32_t lo = 0;  // number of sub-lists that end at or before e: binary search over the lanes' inclusive sums
#pragma unroll
  for (int bit = 32; bit >= 1; bit >>= 1) {
    const uint32_t probe = lo + static_cast<uint32_t>(bit) - 1u;
    const uint32_t end = __shfl(v.incl, static_cast<int>(probe), 64);
    if (end <= e) lo += static_cast<uint32_t>(bit);
  }
  const uint32_t prev = __shfl(v.incl, static_cast<int>(lo ? lo - 1u : 0u), 64);  // (every lane shuffles: a lane must not read from an idle one)
  const uint32_t before = lo ? prev : 0u;
  return P.fr[round & 1u][lo * P.frCap + (e - before)];
}
// Who takes a pair (pair order).  Position e of the frontier of `round` (count = view.total > 0; every lane of the wavefront
// calls: the look-up shuffles) holds node x, whose current entry names y.  The lane takes the pair {x, y} when x's record is still
// the one it reached in the last round (its partner's lane may have moved it on already), y is at its entry for x and has not
// been moved on in this round, and - should y be in this frontier as well - x is the lower index.  Which lane may touch which
// node within a level rests on this rule alone.
PIES_DEV bool frontier_take(const PairArrays& P, const FrontierView& view, uint32_t round, uint32_t e, uint32_t count, uint32_t& x, uint32_t& y,
                            uint4& rx, uint4& ry) {
  const uint32_t stampNow = round & 0xffffu, stampPrev = (round - 1u) & 0xffffu;
  const uint32_t xe = frontier_node(P, view, round, min(e, count - 1u));  // (every lane takes part in the shuffles)
  if (e >= count) return false;
  x = xe;
  rx = load_rec(P.node, x);
  if (!(rec_consistent(rx) && (rx.z & 0xffffu) < rx.y && (rx.z >> 16) == stampPrev)) return false;
  y = rx.w & kPairNodeMask;
  ry = load_rec(P.node, y);
  const uint32_t sy = ry.z >> 16;
  const bool take = rec_consistent(ry) && (ry.z & 0xffffu) < ry.y && sy != stampNow && (ry.w & kPairNodeMask) == x;
  return take && !(sy == stampPrev && y < x);  // (y is in this frontier as well and takes the pair)
}
// The lanes that want it append a node to sub-list `sub` of the frontier of round + 1: first the x of the wavefront's lanes in
// lane order, then the y (the order of a sub-list feeds frontier_node: it is part of the result's determinism, not of the
// result).  One atomic per wavefront and call; every lane of the wavefront calls.  A sub-list that is full loses the node - its
// remaining entries would never be visited -, so the pass is flagged (2) and goes to the sequential loop; frCap leaves a margin
// above what a level can append, this is the net under it.
PIES_DEV void frontier_append(const PairArrays& P, uint32_t round, uint32_t sub, int lane, bool wantX, uint32_t x, bool wantY, uint32_t y) {
  const unsigned long long mx = __ballot(wantX), my = __ballot(wantY);
  const uint32_t nx = static_cast<uint32_t>(__popcll(mx)), ny = static_cast<uint32_t>(__popcll(my));
  if (nx + ny == 0u) return;
  uint32_t at = 0;
  if (lane == 0) at = atomicAdd(&P.frCount[(((round + 1u) % 3u) * kPairLists + sub) * kPairPad], nx + ny);
  at = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(at)));
  uint32_t* dst = P.fr[(round + 1u) & 1u] + static_cast<size_t>(sub) * P.frCap;
  const uint32_t ix = at + static_cast<uint32_t>(__popcll(mx & ((1ull << lane) - 1ull)));
  const uint32_t iy = at + nx + static_cast<uint32_t>(__popcll(my & ((1ull << lane) - 1ull)));
  if (wantX && ix < P.frCap) dst[ix] = x;
  if (wantY && iy < P.frCap) dst[iy] = y;
  if (lane == 0 && at + nx + ny > P.frCap) atomicOr(&P.ctl[kPairFlags], 2u);
}
PIES_DEV void frontier_append(const PairArrays& P, uint32_t round, uint32_t sub, int lane, bool want, uint32_t node) {
  frontier_append(P, round, sub, lane, want, node, false, 0u);
}

// whether a kernel of attempt `repeat` of a pass runs at all: the repeat's only once a repeat is armed, a launch that finishes
// the first attempt's levels not after that (`finishing`), none on a grid that has failed
PIES_DEV bool pass_guard(const HashArrays& H, const PairArrays& P, uint32_t repeat, bool finishing) {
  if (repeat && !P.ctl[kPairRetry]) return false;
  if (finishing && !repeat && P.ctl[kPairRetry]) return false;
  return !H.counters[kCounterFlags];
}
// A level opens: the sub-lists' counts of the round after the next are cleared (their words were read by the previous level and
// are filled by the next), and a level that has work is noted for the diagnostics and for the host's count of captured launches
// (`level`: the round in the pair order; round - 1 by turns, whose first frontier is round 2's).  Every thread calls.
// sameLaunch: workgroups of this launch read the cleared words again (the kernels that finish the levels) - an atomic store;
// otherwise a kernel boundary follows.
PIES_DEV void level_open(const PairArrays& P, uint32_t round, uint32_t level, uint32_t repeat, const FrontierView& view, bool sameLaunch) {
  if (blockIdx.x != 0 || threadIdx.x >= kPairLists) return;
  uint32_t* count = &P.frCount[(((round + 2u) % 3u) * kPairLists + threadIdx.x) * kPairPad];
  if (sameLaunch) __hip_atomic_store(count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *count = 0;
  if (threadIdx.x == 0 && view.total) {
    P.ctl[kPairRounds] = level;
    if (!repeat && level > P.ctl[kPairDeepest]) P.ctl[kPairDeepest] = level;
  }
}

// ---- the remaining levels of a pass in ONE launch ------------------------------------------------------------------------------
// The launch's workgroups run level after level with a barrier where captured launches have a kernel boundary.  Resident
// workgroups use the grid barrier below (release, counter, bounded wait, acquire: the CG continuation's barrier, pd_cg_device.h);
// a wait that times out hands the pass to the sequential loop (flag 2).
PIES_DEV bool pair_grid_barrier(uint32_t* counter, uint32_t nblocks, uint32_t& passed) {
  __shared__ uint32_t sOk;
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    atomicAdd(counter, 1u);
    const uint32_t target = (passed + 1u) * nblocks;
    uint32_t spins = 0, ok = 1u;
    while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(2);
      if (++spins > (1u << 14)) { ok = 0u; break; }  // ~16 ms: a starved barrier (not all workgroups resident) gives the pass to the sequential loop quickly
    }
    // (a workgroup that gives up says so; one that arrives late and finds the counter past its target checks the word)
    if (!ok) __hip_atomic_store(counter + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if (__hip_atomic_load(counter + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ok = 0u;
    __threadfence();
    sOk = ok;
  }
  __syncthreads();
  ++passed;
  return sOk != 0u;
}
// a single workgroup needs no more than its own barrier: global memory written before it is visible to the workgroup after it
struct WorkgroupBarrier {
  PIES_DEV bool operator()() const {
    __threadfence();
    __syncthreads();
    return true;
  }
};
// The loop: from `round` on until a frontier is empty (the same words in every wavefront of the launch: all leave together).
// level(round, view) runs one level on the launch's workgroups and returns what the caller counts (its resolved visits),
// barrier() returns whether the launch may go on; `turns`: the level's number is round - 1 (level_open).  The caller has asked
// pass_guard.  Returns the sum of the levels' counts (a sum, not a reference the levels add to: that cost the single-workgroup
// kernels ten registers).
template <class Level, class Barrier>
PIES_DEV uint32_t finish_levels(const PairArrays& P, uint32_t round, bool turns, uint32_t repeat, Level level, Barrier barrier) {
  const int lane = threadIdx.x & 63;
  uint32_t hits = 0;
  for (;; ++round) {
    const FrontierView view = frontier_view(P, round, lane);
    if (view.total == 0u) break;
    level_open(P, round, turns ? round - 1u : round, repeat, view, true);
    hits += level(round, view);
    if (!barrier()) {
      if (threadIdx.x == 0) atomicOr(&P.ctl[kPairFlags], 2u);
      break;
    }
  }
  return hits;
}

}  // namespace pies
