// Point-triangle collisions of the Projective-Dynamics substep, second stage: from the hit records of the detection
// (tri_detect.hip) to everything the solver reads.
//
//   contact list  in the reference's order (Src/Solver.cpp:721-797, 852): offsets of the per-triangle counts (tri_scan), the list
//                 itself (tri_emit).
//   constraint    CollisionConstraint.cpp:67-194: differential coordinates w.r.t. the point (A = B), projection
//                 along the triangle normal, w = 1e4; its 4x4 block is added to the system matrix through a
//                 per-node list of contacts (diagonal into cdiag, off-diagonals applied inside the SpMV, from the incidence lists or
//                 from the merged rows of k_contact_csr).
//   levels        of the list's dependency DAG (two contacts conflict when they share a node), for the sequential passes of
//                 tri_passes.hip.
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "tri_device.h"

namespace pies {

constexpr int kBlock = 256;

// The contact list from the hit records (Solver.cpp:721-797 order: the cells of the triangle's range x-major, in each cell the
// listed triangles by ascending index, for each the triangle's corners 0, 1, 2).  One thread per record {t, o, corners}: for every
// cell both ranges hold, the entry's position = the triangle's offset + what all of the triangle's records (its chain) put in
// front of it: a record's hits x (the cells it shares with t that come earlier + this cell, if it holds it and the partner's
// index is smaller).
PIES_DEV void tri_emit(const TriArrays& T, uint32_t first, uint32_t stride) {
  const uint32_t nrec = min(T.counters[kTriCtrHitRecords], T.maxContacts);
  for (uint32_t r = first; r < nrec; r += stride) {
    const uint4 rec = T.pool[r];
    const uint32_t t = rec.x, o = rec.y;
    const int4 rg = T.rng[t];
    const CellBox S = insert_box(rg);  // (a triangle with records searched: its range is the one it was listed with)
    const CellBox mine = meet(S, insert_box(T.rng[o]));
    const uint32_t base = T.offTri[merge_rank(t, T.nt, T.threadCount)];
    const uint32_t ia[3] = {T.tris[3 * t], T.tris[3 * t + 1], T.tris[3 * t + 2]};
    const uint32_t ib = T.tris[3 * o], ic = T.tris[3 * o + 1], idd = T.tris[3 * o + 2];
    for (int x = mine.x0; x < mine.x1; ++x)
      for (int y = mine.y0; y < mine.y1; ++y)
        for (int z = mine.z0; z < mine.z1; ++z) {
          uint32_t c = base;
          for (uint32_t q = T.head[t]; q != kNil;) {
            const uint4 other = T.pool[q];
            const CellBox theirs = meet(S, insert_box(T.rng[other.y]));
            c += static_cast<uint32_t>(__popc(other.z)) * (cells_before(theirs, x, y, z) + ((other.y < o && holds(theirs, x, y, z)) ? 1u : 0u));
            q = other.w;
          }
#pragma unroll
          for (int i = 0; i < 3; ++i)
            if (rec.z >> i & 1u) {
              if (c < T.maxContacts) T.ids[c] = make_uint4(ia[i], ib, ic, idd);
              ++c;
            }
        }
  }
}
__global__ void __launch_bounds__(kBlock) k_tri_emit(TriArrays T) {
  if (T.counters[kTriCtrFailure]) return;
  tri_emit(T, blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock);
}

// exclusive scan of the per-triangle counts in the reference's merge order (one block).  Every wavefront takes one contiguous
// sixteenth of the counts: a coalesced sweep for its sum, the sixteen sums in LDS, and - only for a wavefront whose range holds
// contacts at all - a second sweep that writes the offsets (wave-wide scans over 64 counts at a time).  A substep without
// contacts is one sweep of loads that do not depend on each other (the first version gave every thread 41 consecutive counts
// and a 10-step Hillis-Steele scan over the threads: 10 us at 42k triangles).
// (a workgroup of 1024; returns the length of the contact list)
PIES_DEV uint32_t tri_scan(const TriArrays& T, uint32_t* wsum) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nt = T.nt;
  const uint32_t per = (((nt + 15u) / 16u) + 63u) & ~63u;
  const uint32_t lo = min(nt, wave * per), hi = min(nt, lo + per);
  uint32_t sum = 0;
  {  // four independent 16-byte loads per lane and round: the sweep is a chain of load latencies (one word per lane and round took
     // 38 us for the 100k triangles of config 5's body)
    const uint4* c4 = reinterpret_cast<const uint4*>(T.cntTri + lo);  // (lo is a multiple of 64)
    const uint32_t quads = (hi - lo) / 4u;
    uint32_t q = lane;
    for (; q + 192u < quads; q += 256u) {
      const uint4 a = c4[q], b = c4[q + 64u], c = c4[q + 128u], d = c4[q + 192u];
      sum += ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w)) + ((c.x + c.y) + (c.z + c.w)) + ((d.x + d.y) + (d.z + d.w));
    }
    for (; q < quads; q += 64u) { const uint4 a = c4[q]; sum += (a.x + a.y) + (a.z + a.w); }
    for (uint32_t r = lo + 4u * quads + lane; r < hi; r += 64u) sum += T.cntTri[r];
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if (lane == 0u) wsum[wave] = sum;
  __syncthreads();
  uint32_t run = 0, total = 0;
#pragma unroll
  for (uint32_t w = 0; w < 16u; ++w) {
    const uint32_t v = wsum[w];
    if (w < wave) run += v;
    total += v;
  }
  if (sum != 0u) {  // (offsets of a range without contacts are never read: the fill pass skips empty triangles)
    for (uint32_t r0 = lo; r0 < hi; r0 += 64u) {
      const uint32_t r = r0 + lane;
      const uint32_t c = r < hi ? T.cntTri[r] : 0u;
      if (__builtin_amdgcn_ballot_w64(c != 0u) == 0ull) continue;  // (64 triangles without a contact: their offsets are never read)
      uint32_t inc = c;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(inc, off, 64);
        if (lane >= static_cast<uint32_t>(off)) inc += v;
      }
      if (r < hi) T.offTri[r] = run + inc - c;
      run += __shfl(inc, 63, 64);
    }
  }
  if (tid == 0u) {
    if (total > T.maxContacts) atomicOr(&T.counters[kTriCtrFailure], kTriFailOverflow);  // contact list overflow: latch
    T.counters[kTriCtrContacts] = min(total, T.maxContacts);
  }
  return total;
}
// no hit record, no contact: the usual substep (the single-workgroup kernels below leave at this line)
PIES_DEV bool no_hit_record(const TriArrays& T) {
  if (T.counters[kTriCtrHitRecords] != 0u) return false;
  if (threadIdx.x == 0u) T.counters[kTriCtrContacts] = 0u;
  return true;
}
__global__ void __launch_bounds__(1024) k_tri_scan(TriArrays T) {
  __shared__ uint32_t wsum[16];
  if (no_hit_record(T)) return;
  tri_scan(T, wsum);
}

// ---- per-node incidence of the contacts + their diagonal blocks ---------------------------------------------
// Five steps with a device-wide dependency between them (count, used, alloc, fill, sort).  Each is a device function over
// (first item, stride); the contact-heavy graph variant runs them as five launches, the other one as part of ONE launch of a
// single workgroup (inc_chain in k_tri_tail) - a substep with few or no contacts pays one launch for the lot instead of five.
PIES_DEV void inc_count(const TriArrays& T, float* __restrict__ cdiag, uint32_t first, uint32_t stride) {
  const uint32_t M = T.counters[kTriCtrContacts];
  for (uint32_t c = first; c < M; c += stride) {
    const uint4 id = T.ids[c];
    const uint32_t n[4] = {id.x, id.y, id.z, id.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (atomicAdd(&T.incCnt[n[i]], 1u) == 0u) atomicOr(&T.usedBits[n[i] >> 5], 1u << (n[i] & 31u));
      // diag(w A^T A) = w * (3, 1, 1, 1); multiples of 1e4 add exactly in float, so the order is irrelevant
      atomicAdd(&cdiag[n[i]], kTriContactW * (i == 0 ? 3.0f : 1.0f));
    }
  }
}
// The nodes that take part in contacts, in ascending order, from the bitmap inc_count marked them in: one workgroup of 1024, a
// thread per run of bitmap words (popcounts, a prefix sum over the threads, then the set bits in order).  An append in
// arrival order would be cheaper, but the order decides which wavefront sums which contact rows (k_cg_ap), i.e. the rounding
// of p.Ap: results would differ from run to run.
PIES_DEV void inc_used(const TriArrays& T, uint32_t words, uint32_t* part) {
  const uint32_t tid = threadIdx.x;
  const uint32_t chunk = (words + 1023u) / 1024u;
  const uint32_t lo = min(words, tid * chunk), hi = min(words, lo + chunk);
  uint32_t sum = 0;
  for (uint32_t w = lo; w < hi; ++w) sum += static_cast<uint32_t>(__popc(T.usedBits[w]));
  part[tid] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
    const uint32_t v = tid >= off ? part[tid - off] : 0u;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  uint32_t at = tid ? part[tid - 1] : 0u;
  if (sum)
    for (uint32_t w = lo; w < hi; ++w) {
      uint32_t bits = T.usedBits[w];
      while (bits) {
        const uint32_t b = static_cast<uint32_t>(__ffs(bits)) - 1u;
        T.usedNodes[at++] = (w << 5) + b;
        bits &= bits - 1u;
      }
    }
  if (tid == 1023) T.counters[kTriCtrUsedNodes] = part[1023];
}
PIES_DEV void inc_alloc(const TriArrays& T, const float* __restrict__ kdiag, const float* __restrict__ cdiag, float* __restrict__ dinv,
                        uint32_t first, uint32_t stride) {
  const uint32_t used = T.counters[kTriCtrUsedNodes];
  for (uint32_t u = first; u < used; u += stride) {
    const uint32_t n = T.usedNodes[u];
    T.incStart[n] = atomicAdd(&T.counters[kTriCtrIncidences], T.incCnt[n]);
    T.incFill[n] = 0;
    T.nodeSlot[n] = u;  // the node's place in the LDS copy of the sequential passes
    dinv[n] = 1.0f / (kdiag[n] + cdiag[n]);
  }
}
PIES_DEV void inc_fill(const TriArrays& T, uint32_t first, uint32_t stride) {
  const uint32_t M = T.counters[kTriCtrContacts];
  for (uint32_t c = first; c < M; c += stride) {
    const uint4 id = T.ids[c];
    const uint32_t n[4] = {id.x, id.y, id.z, id.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) T.inc[T.incStart[n[i]] + atomicAdd(&T.incFill[n[i]], 1u)] = (c << 2) | static_cast<uint32_t>(i);
  }
}
PIES_DEV void inc_sort(const TriArrays& T, uint32_t wave, uint32_t nwaves) {
  const uint32_t used = T.counters[kTriCtrUsedNodes];
  const int lane = threadIdx.x & 63;
  for (uint32_t u = wave; u < used; u += nwaves) {
    const uint32_t n = T.usedNodes[u];
    rank_sort(T.inc, T.incSorted, T.incStart[n], T.incCnt[n], lane, T.incPos);
  }
}
__global__ void __launch_bounds__(kBlock) k_inc_count(TriArrays T, float* __restrict__ cdiag) {
  inc_count(T, cdiag, blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock);
}
__global__ void __launch_bounds__(1024) k_inc_used(TriArrays T, uint32_t words) {
  __shared__ uint32_t part[1024];
  inc_used(T, words, part);
}
__global__ void __launch_bounds__(kBlock) k_inc_alloc(TriArrays T, const float* __restrict__ kdiag, const float* __restrict__ cdiag,
                                                      float* __restrict__ dinv) {
  inc_alloc(T, kdiag, cdiag, dinv, blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock);
}
__global__ void __launch_bounds__(kBlock) k_inc_fill(TriArrays T) { inc_fill(T, blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock); }
__global__ void __launch_bounds__(kBlock) k_inc_sort(TriArrays T) {
  inc_sort(T, (blockIdx.x * kBlock + threadIdx.x) >> 6, (gridDim.x * kBlock) >> 6);
}
// between two steps run by one workgroup: a step's stores are in L2, and this compute unit's vector cache holds none of the lines
// they went to, before the next step starts (the fence), and every wavefront has finished the step (the barrier)
PIES_DEV void step_boundary() {
  __threadfence();
  __syncthreads();
}
// the five steps by one workgroup of 1024 (part: 1024 words of LDS)
PIES_DEV void inc_chain(const TriArrays& T, const float* __restrict__ kdiag, float* __restrict__ cdiag, float* __restrict__ dinv, uint32_t words,
                        uint32_t* part) {
  inc_count(T, cdiag, threadIdx.x, 1024u);
  step_boundary();
  inc_used(T, words, part);
  step_boundary();
  inc_alloc(T, kdiag, cdiag, dinv, threadIdx.x, 1024u);
  step_boundary();
  inc_fill(T, threadIdx.x, 1024u);
  step_boundary();
  inc_sort(T, threadIdx.x >> 6, 16u);
}
// The graph variant for substeps with few or no contacts: the offsets of the contact list, the list and the incidence chain by
// ONE workgroup (three launches fewer; a substep without a hit record - the usual one - leaves at the first line).
PIES_DEV bool tri_tail(const TriArrays& T, const float* __restrict__ kdiag, float* __restrict__ cdiag, float* __restrict__ dinv, uint32_t words,
                       uint32_t* part) {  // (a workgroup of 1024; part: 1024 words of LDS; false: no contact list in this substep)
  if (no_hit_record(T)) return false;
  const uint32_t total = tri_scan(T, part);
  if (total > T.maxContacts || T.counters[kTriCtrFailure]) return false;  // (latched: the tick ends as a failure)
  step_boundary();
  tri_emit(T, threadIdx.x, 1024u);
  step_boundary();
  inc_chain(T, kdiag, cdiag, dinv, words, part);
  return true;
}
__global__ void __launch_bounds__(1024) k_tri_tail(TriArrays T, const float* __restrict__ kdiag, float* __restrict__ cdiag, float* __restrict__ dinv,
                                                   uint32_t words) {
  __shared__ uint32_t part[1024];
  tri_tail(T, kdiag, cdiag, dinv, words, part);
}

// ---- merged contact rows -------------------------------------------------------------------------------------
// The off-diagonal part of a node's row of the contact matrix, w * (AtA)_i. summed over its contacts, with equal columns
// merged: a node of a contact patch sits in tens of contacts over a handful of triangles, so its ~100 row entries name
// ~15 distinct nodes.  The CG sums these rows once per iteration (k_cg_ap's row blocks): with the merged form a row is one
// gather of at most a wavefront's width instead of three dependent loads per contact.  One wavefront per node: the raw
// columns go through a small LDS hash with counts (integer adds: exact), the distinct ones are sorted by column (ranks
// among at most kRowMaxUnique entries), so the stored order - and with it the rounding of the sum - does not depend on
// which lane got where first.  A node with more distinct columns than kRowMaxUnique keeps the contact-by-contact form
// (rowLen = kRowUnmerged).  Storage: 6 entries per contact at most.
constexpr uint32_t kRowSlots = 512, kRowMaxUnique = 256, kRowUnmerged = 0xffffffffu;
__global__ void __launch_bounds__(kBlock) k_contact_csr(TriArrays T, uint32_t maxUnique) {
  __shared__ uint32_t hkey[kBlock / 64][kRowSlots];
  __shared__ uint32_t hcnt[kBlock / 64][kRowSlots];
  __shared__ uint32_t ucol[kBlock / 64][kRowMaxUnique], ucnt[kBlock / 64][kRowMaxUnique];
  const uint32_t used = T.counters[kTriCtrUsedNodes];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6, nwaves = (gridDim.x * kBlock) >> 6;
  for (uint32_t u = wave; u < used; u += nwaves) {
    const uint32_t node = T.usedNodes[u];
    const uint32_t tc = T.incCnt[node], ts = T.incStart[node];
    for (uint32_t t = lane; t < kRowSlots; t += 64) { hkey[w][t] = 0xffffffffu; hcnt[w][t] = 0; }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    uint32_t fresh = 0;
    for (uint32_t base = 0; base < tc; base += 64) {
      const uint32_t t = base + lane;
      uint32_t cols[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
      if (t < tc) {
        const uint32_t v = T.incSorted[ts + t];
        const uint4 id = T.ids[v >> 2];
        if ((v & 3u) == 0u) { cols[0] = id.y; cols[1] = id.z; cols[2] = id.w; }  // the point's row couples to the triangle's nodes,
        else cols[0] = id.x;                                                       // their rows to the point
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        bool mine = false;
        if (cols[q] != 0xffffffffu && fresh <= maxUnique) {
          uint32_t h = (cols[q] * 2654435761u) >> 23;  // 9 bits
          for (;;) {
            const uint32_t old = atomicCAS(&hkey[w][h], 0xffffffffu, cols[q]);
            if (old == 0xffffffffu) { mine = true; break; }
            if (old == cols[q]) break;
            h = (h + 1u) & (kRowSlots - 1u);
          }
          atomicAdd(&hcnt[w][h], 1u);
        }
        fresh += static_cast<uint32_t>(__popcll(__ballot(mine)));
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (fresh > maxUnique) {  // (uniform: every lane counted the same ballots)
      if (lane == 0) T.rowLen[node] = kRowUnmerged;
      continue;
    }
    // compact the occupied slots, then order them by column
    uint32_t nu = 0;
    for (uint32_t base = 0; base < kRowSlots; base += 64) {
      const uint32_t k = hkey[w][base + lane];
      const bool occ = k != 0xffffffffu;
      const unsigned long long m = __ballot(occ);
      if (occ) {
        const uint32_t at = nu + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
        ucol[w][at] = k;
        ucnt[w][at] = hcnt[w][base + lane];
      }
      nu += static_cast<uint32_t>(__popcll(m));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    uint32_t off = 0;
    if (lane == 0) off = atomicAdd(&T.counters[kTriCtrRowEntries], nu);
    off = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(off)));
    for (uint32_t t = lane; t < nu; t += 64) {
      const uint32_t c = ucol[w][t];
      uint32_t rank = 0;
      for (uint32_t o = 0; o < nu; ++o) rank += ucol[w][o] < c ? 1u : 0u;  // columns are distinct
      T.rowCol[off + rank] = c;
      T.rowCoef[off + rank] = -kTriContactW * static_cast<float>(ucnt[w][t]);
    }
    if (lane == 0) { T.rowStart[node] = off; T.rowLen[node] = nu; }
  }
}

// ---- dependency levels ---------------------------------------------------------------------------------------
// Dependency levels of the whole contact list, once per substep: level(c) = 1 + the highest level among the earlier
// contacts that share a node with c, so that running the list level by level, in any order inside a level, is the
// reference's sequential pass.  A node's contacts are already listed in ascending order (incSorted) with every
// incidence's position in that list (incPos), so the earlier contact that matters for node n is the list entry before
// c: at most four predecessors per contact, all with smaller indices.  Three algorithms: levels_by_node_owners (the fast
// path, below) writes the level lists itself; levels_by_chunked_relaxation (lists of at most kLevelsLdsCap contacts) and
// levels_by_window_walk (longer ones) find every contact's level, and bucket_by_level makes the lists.  More than
// kTriMaxLevels levels (thousands of contacts on one node) set the pass form kTriPassWalk and the passes fall back to the
// single-wavefront walk.
constexpr uint32_t kLevelsLdsCap = 49152;  // contacts whose 16-bit levels fit next to the histogram in LDS
// The fast path (the touched nodes fit the LDS copy of the sequential passes, at most kSeqLdsNodes, and the list has at most
// kLvMaxContacts entries): Kahn's algorithm with the NODES as owners.  A thread owns up to four touched nodes and walks each
// node's sorted contact list (incSorted) with a private cursor; heads[c] (one byte per contact, LDS) counts on how many of
// its four nodes contact c is the first unprocessed entry.  Round r: every owner looks at the contact its list stands at
// (heads == 4: all four owners see the same snapshot, so all four agree), barrier, the owners of ready contacts move on
// (heads of the next entry + 1) and the owner of the contact's point appends it to level r, barrier.  A round is two
// barriers and a few LDS operations, its list entries were requested four to eight rounds earlier; the number of rounds is
// the number of levels (the old path relaxed 1024 contacts at a time: the sum of the chunks' chain lengths, 6x as many
// rounds on a 29k-contact patch: 1.35 ms against 0.2 ms).
constexpr uint32_t kLvMaxContacts = 65536;
PIES_DEV uint32_t ldu32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <uint32_t kLvNodesPerThread>
PIES_DEV void levels_by_node_owners(const TriArrays& T, uint32_t* heads32, uint32_t* sCnt, const uint32_t M, const uint32_t used, const int tid) {
  // Per owned node: `head` = the list entry the node stands at (position k), nx[0..3] = the entries behind it, pend[0..3]
  // = the four after those, requested at the last refill.  Global memory is only touched at refills - every four rounds,
  // by every thread at once (a node consumes at most one entry per round) - so that no wavefront waits for a load inside
  // a round; the level lists are written with plain stores.
  const uint8_t* heads8 = reinterpret_cast<const uint8_t*>(heads32);
  for (uint32_t w = tid; w < (M + 3) / 4; w += kSeqBlock) heads32[w] = 0;
  if (tid < 3) sCnt[tid] = 0;
  __syncthreads();
  uint32_t base[kLvNodesPerThread], cnt[kLvNodesPerThread], k[kLvNodesPerThread], kRefill[kLvNodesPerThread], head[kLvNodesPerThread];
  uint32_t nx[kLvNodesPerThread][4], pend[kLvNodesPerThread][4];
  auto entry_at = [&](uint32_t j, uint32_t at) {  // list entry `at` of owned node j (any in-range entry when past the end)
    const uint32_t last = cnt[j] ? cnt[j] - 1u : 0u;
    return T.incSorted[base[j] + min(at, last)];
  };
#pragma unroll
  for (uint32_t j = 0; j < kLvNodesPerThread; ++j) {
    const uint32_t u = tid + j * kSeqBlock;
    base[j] = 0; cnt[j] = 0; k[j] = 0; kRefill[j] = 0;
    if (u < used) {
      const uint32_t n = T.usedNodes[u];
      base[j] = T.incStart[n];
      cnt[j] = T.incCnt[n];
    }
    head[j] = entry_at(j, 0);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) { nx[j][i] = entry_at(j, 1 + i); pend[j][i] = entry_at(j, 5 + i); }
    if (cnt[j]) {
      const uint32_t c = head[j] >> 2;
      atomicAdd(&heads32[c >> 2], 1u << (8u * (c & 3u)));
    }
  }
  if (tid == 0) T.lvStart[0] = 0;
  __syncthreads();
  uint32_t total = 0, r = 0;
  bool stuck = false;
  while (total < M && !stuck) {
    // refill: s = entries consumed since the last one (0..4); the entries requested then have had four rounds to arrive
#pragma unroll
    for (uint32_t j = 0; j < kLvNodesPerThread; ++j) {
      const uint32_t s = k[j] - kRefill[j];
      const uint32_t n0 = s < 4u ? nx[j][0] : pend[j][0];
      const uint32_t n1 = s < 3u ? nx[j][1] : (s == 3u ? pend[j][0] : pend[j][1]);
      const uint32_t n2 = s < 2u ? nx[j][2] : (s == 2u ? pend[j][0] : s == 3u ? pend[j][1] : pend[j][2]);
      const uint32_t n3 = s < 1u ? nx[j][3] : (s == 1u ? pend[j][0] : s == 2u ? pend[j][1] : s == 3u ? pend[j][2] : pend[j][3]);
      nx[j][0] = n0; nx[j][1] = n1; nx[j][2] = n2; nx[j][3] = n3;
      kRefill[j] = k[j];
      // (a node that consumed nothing since the last refill has its four requested entries already: a node of a 28k-contact
      // patch moves on in one round of ten, and 16 uncoalesced requests per thread every four rounds - 16 000 from ONE compute
      // unit - cost a sixth of the kernel: 1 063 -> 887 us for the 610 levels of that patch.  Fewer owning threads with more
      // nodes each are slower: 512 threads 1 126 us, 256 threads 2 906 us.  ONE barrier per round instead of two - two copies of the
      // counters, a round reads one and adds to the other, the copy it read gets the addition a round later - is slower too: 938 us:
      // a round is its LDS operations and its ~150 instructions per wavefront, sixteen wavefronts on one compute unit.)
      if (s != 0u) {
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) pend[j][i] = entry_at(j, k[j] + 5u + i);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {  // (unrolled: a loop here makes the compiler drain the refill's loads before entering it)
      if (total >= M) break;
      if (r >= kTriMaxLevels) { stuck = true; break; }
      bool ready[kLvNodesPerThread];
      uint32_t nEmit = 0;
#pragma unroll
      for (uint32_t j = 0; j < kLvNodesPerThread; ++j) {
        ready[j] = k[j] < cnt[j] && heads8[head[j] >> 2] == 4;
        nEmit += (ready[j] && (head[j] & 3u) == 0u) ? 1u : 0u;
      }
      lds_barrier();
      uint32_t at = nEmit ? total + atomicAdd(&sCnt[r % 3u], nEmit) : 0u;
#pragma unroll
      for (uint32_t j = 0; j < kLvNodesPerThread; ++j) {
        if (!ready[j]) continue;
        if ((head[j] & 3u) == 0u) T.lvOrder[at++] = head[j] >> 2;
        ++k[j];
        head[j] = nx[j][0]; nx[j][0] = nx[j][1]; nx[j][1] = nx[j][2]; nx[j][2] = nx[j][3];
        if (k[j] < cnt[j]) {
          const uint32_t c = head[j] >> 2;
          atomicAdd(&heads32[c >> 2], 1u << (8u * (c & 3u)));
        }
      }
      lds_barrier();
      const uint32_t made = sCnt[r % 3u];
      if (made == 0u) { stuck = true; break; }  // (a contact that names a node twice never becomes ready: the walk takes over)
      total += made;
      if (tid == 0) { sCnt[(r + 2u) % 3u] = 0; T.lvStart[r + 1u] = total; }
      ++r;
    }
  }
  if (stuck) {
    if (tid == 0) { T.counters[kTriCtrLevels] = 1u << 20; T.counters[kTriCtrPassForm] = kTriPassWalk; }
    return;
  }
  if (tid == 0) { T.counters[kTriCtrLevels] = r; T.counters[kTriCtrPassForm] = kTriPassLds; }
  __syncthreads();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the level lists have left the wavefronts
  __syncthreads();
  for (uint32_t q = tid; q < M; q += kSeqBlock) {  // the LDS slots of every contact's nodes, in level order
    const uint4 id = T.ids[ldu32(T.lvOrder + q)];
    T.lvSlots[q] = make_uint2(T.nodeSlot[id.x] | (T.nodeSlot[id.y] << 16), T.nodeSlot[id.z] | (T.nodeSlot[id.w] << 16));
  }
}

// The list is relaxed 1024 contacts at a time, in order: predecessors in earlier chunks are final, those inside the chunk are
// iterated to the fixed point (as many rounds as the longest chain inside the chunk; levels live in LDS, 16 bit: slv).  Leaves the
// highest level (1 << 20: more than 16 bits hold) in sMaxLevel.
PIES_DEV void levels_by_chunked_relaxation(const TriArrays& T, uint16_t* slv, int& sMaxLevel, const uint32_t M, const int tid) {
  int top = -1;
  bool overflow = false;
  for (uint32_t base = 0; base < M; base += kSeqBlock) {
    const uint32_t c = base + tid;
    const bool valid = c < M;
    uint32_t pred[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    if (valid) {
      const uint4 id = T.ids[c];
      const uint32_t node[4] = {id.x, id.y, id.z, id.w};
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const uint32_t rank = T.incPos[4 * c + l];
        if (rank) pred[l] = T.incSorted[T.incStart[node[l]] + rank - 1] >> 2;
      }
      slv[c] = 0;
    }
    __syncthreads();
    int cur = 0;
    for (;;) {
      int lv = 0;
      if (valid) {
#pragma unroll
        for (int l = 0; l < 4; ++l)
          if (pred[l] != 0xffffffffu) lv = max(lv, static_cast<int>(slv[pred[l]]) + 1);
      }
      const bool changed = valid && lv != cur;
      if (changed) { cur = lv; slv[c] = static_cast<uint16_t>(min(lv, 65535)); }
      if (!__syncthreads_or(changed ? 1 : 0)) break;
    }
    if (valid) { top = max(top, cur); overflow = overflow || cur >= 65535; }
  }
  // block maximum of the levels
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) top = max(top, __shfl_xor(top, off, 64));
  if ((tid & 63) == 0) atomicMax(&sMaxLevel, overflow ? 1 << 20 : top);
  __syncthreads();
}
// The older walk: one wavefront, 64 contacts at a time, levels inside the window with 63 cross-lane broadcasts (window_levels)
// on top of a per-node "level of the last earlier contact" array (lastLevel); the levels go to T.lvl, the highest to sMaxLevel.
PIES_DEV void levels_by_window_walk(const TriArrays& T, int& sMaxLevel, const uint32_t M, const int tid) {
  if (tid < 64) {
    int top = -1;
    for (uint32_t base = 0; base < M; base += 64) {
      const bool valid = base + tid < M;
      const uint4 id = valid ? T.ids[base + tid] : make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
      int bl = 0;
      if (valid) {
        const int a = __hip_atomic_load(T.lastLevel + id.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int b = __hip_atomic_load(T.lastLevel + id.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int c = __hip_atomic_load(T.lastLevel + id.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int d = __hip_atomic_load(T.lastLevel + id.w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bl = max(max(a, b), max(c, d)) + 1;
      }
      int maxLevel;
      const int level = window_levels(valid, id, tid, maxLevel, bl);
      if (valid) {
        T.lvl[base + tid] = static_cast<uint32_t>(level);
        atomicMax(T.lastLevel + id.x, level); atomicMax(T.lastLevel + id.y, level);
        atomicMax(T.lastLevel + id.z, level); atomicMax(T.lastLevel + id.w, level);
      }
      top = max(top, maxLevel);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the window's levels are in L2 before the next window reads them
    }
    if (tid == 0) sMaxLevel = top;
  }
  __syncthreads();
  for (uint32_t c = tid; c < M; c += kSeqBlock) {  // behind us: the per-node levels go back to -1 for the next substep
    const uint4 id = T.ids[c];
    T.lastLevel[id.x] = -1; T.lastLevel[id.y] = -1; T.lastLevel[id.z] = -1; T.lastLevel[id.w] = -1;
  }
}
// The contacts bucketed by level (level_of(c): from either algorithm above; hist: kTriMaxLevels + 1 zeroed words of LDS):
// lvStart, lvOrder and the pass form kTriPassL2.
template <class LevelOf>
PIES_DEV void bucket_by_level(const TriArrays& T, uint32_t* hist, LevelOf level_of, const int levels, const uint32_t M, const int tid) {
  for (uint32_t c = tid; c < M; c += kSeqBlock) atomicAdd(&hist[level_of(c) + 1], 1u);
  __syncthreads();
  if (tid == 0) {
    for (int b = 0; b < levels; ++b) hist[b + 1] += hist[b];  // hist[b] = first slot of level b
    T.counters[kTriCtrLevels] = static_cast<uint32_t>(levels);
    T.counters[kTriCtrPassForm] = kTriPassL2;  // level by level through L2
  }
  __syncthreads();
  for (int b = tid; b <= levels; b += kSeqBlock) T.lvStart[b] = hist[b];
  __syncthreads();
  for (uint32_t c = tid; c < M; c += kSeqBlock) T.lvOrder[atomicAdd(&hist[level_of(c)], 1u)] = c;  // any order inside a level
}

PIES_DEV void tri_levels(const TriArrays& T, int ldsForm) {  // (a workgroup of kSeqBlock)
  __shared__ __align__(16) uint32_t raw[(kTriMaxLevels + 1) + kLevelsLdsCap / 2 + 8];
  static_assert(sizeof(raw) >= kLvMaxContacts + 64, "heads[] of the fast path must fit");
  __shared__ int sMaxLevel;
  uint32_t* hist = raw;
  uint16_t* slv = reinterpret_cast<uint16_t*>(raw + kTriMaxLevels + 2);
  const uint32_t M = T.counters[kTriCtrContacts];
  const int tid = threadIdx.x;
  if (ldsForm && M != 0 && M <= kLvMaxContacts && T.counters[kTriCtrUsedNodes] <= kSeqLdsNodes) {
    const uint32_t used = T.counters[kTriCtrUsedNodes];  // nodes per thread: as few as the touched nodes need (a round's cost is per slot)
    if (used <= kSeqBlock) levels_by_node_owners<1>(T, raw + 4, raw, M, used, tid);
    else if (used <= 2 * kSeqBlock) levels_by_node_owners<2>(T, raw + 4, raw, M, used, tid);
    else levels_by_node_owners<4>(T, raw + 4, raw, M, used, tid);
    return;
  }
  for (int b = tid; b <= static_cast<int>(kTriMaxLevels); b += kSeqBlock) hist[b] = 0;
  if (tid == 0) sMaxLevel = -1;
  __syncthreads();
  if (M == 0) {
    if (tid == 0) { T.counters[kTriCtrLevels] = 0; T.counters[kTriCtrPassForm] = kTriPassLds; }
    return;
  }
  const bool inLds = M <= kLevelsLdsCap;
  if (inLds) levels_by_chunked_relaxation(T, slv, sMaxLevel, M, tid);
  else levels_by_window_walk(T, sMaxLevel, M, tid);
  const int levels = sMaxLevel + 1;
  if (levels > static_cast<int>(kTriMaxLevels)) {
    if (tid == 0) { T.counters[kTriCtrLevels] = static_cast<uint32_t>(min(levels, 1 << 20)); T.counters[kTriCtrPassForm] = kTriPassWalk; }
    return;
  }
  bucket_by_level(T, hist, [&](uint32_t c) { return inLds ? static_cast<uint32_t>(slv[c]) : T.lvl[c]; }, levels, M, tid);
}
__global__ void __launch_bounds__(kSeqBlock) k_tri_levels(TriArrays T, int ldsForm) { tri_levels(T, ldsForm); }
// The contact-light graph variant, levels in line: list offsets, list, incidence chain and dependency levels by ONE workgroup (a
// substep without a hit record leaves at the first line; k_tri_box has zeroed what the levels would report).
static_assert(kSeqBlock == 1024, "k_tri_tail_levels runs the tail's steps and the levels with one workgroup size");
__global__ void __launch_bounds__(1024) k_tri_tail_levels(TriArrays T, const float* __restrict__ kdiag, float* __restrict__ cdiag, float* __restrict__ dinv,
                                                          uint32_t words, int ldsForm) {
  __shared__ uint32_t part[1024];
  if (!tri_tail(T, kdiag, cdiag, dinv, words, part)) return;
  step_boundary();
  tri_levels(T, ldsForm);
}

// ------------------------------------------------------------------------------------------------------------
static int tri_lds_form() {
  const char* e = tuning_env("PIES_TRI_LDS");  // diagnostics, read when the substep is captured: 0 = sequential passes through L2
  return e && e[0] == '0' ? 0 : 1;
}
void launch_tri_lists(hipStream_t st_, const TriArrays& T, const NodeArrays& nd, const float* kdiag, float* cdiag, float* dinv, bool mergedRows,
                      bool levelsInLine) {
  const uint32_t words = (nd.n + 31u) / 32u;
  if (!mergedRows) {  // the variant for substeps with few or no contacts: list offsets, list and incidence chain as one launch of one workgroup
    if (levelsInLine)  // ... and the dependency levels with them (launch_tri_levels is not called then)
      hipLaunchKernelGGL(k_tri_tail_levels, dim3(1), dim3(1024), 0, st_, T, kdiag, cdiag, dinv, words, tri_lds_form());
    else
      hipLaunchKernelGGL(k_tri_tail, dim3(1), dim3(1024), 0, st_, T, kdiag, cdiag, dinv, words);
    return;
  }
  const dim3 cgrid(std::min<uint32_t>(256u, (T.maxContacts + kBlock - 1) / kBlock)), blk(kBlock);
  hipLaunchKernelGGL(k_tri_scan, dim3(1), dim3(1024), 0, st_, T);
  hipLaunchKernelGGL(k_tri_emit, cgrid, blk, 0, st_, T);
  hipLaunchKernelGGL(k_inc_count, cgrid, blk, 0, st_, T, cdiag);
  hipLaunchKernelGGL(k_inc_used, dim3(1), dim3(1024), 0, st_, T, words);
  hipLaunchKernelGGL(k_inc_alloc, cgrid, blk, 0, st_, T, kdiag, cdiag, dinv);
  hipLaunchKernelGGL(k_inc_fill, cgrid, blk, 0, st_, T);
  hipLaunchKernelGGL(k_inc_sort, cgrid, blk, 0, st_, T);
  uint32_t maxUnique = kRowMaxUnique;  // diagnostics: PIES_ROW_MAX_UNIQUE lowers it (rows with more distinct columns stay unmerged)
  if (const char* e = tuning_env("PIES_ROW_MAX_UNIQUE")) maxUnique = std::min<uint32_t>(kRowMaxUnique, static_cast<uint32_t>(std::max(0, std::atoi(e))));
  hipLaunchKernelGGL(k_contact_csr, cgrid, blk, 0, st_, T, maxUnique);
}
void launch_tri_levels(hipStream_t st_, const TriArrays& T) {
  if (T.nt == 0) return;
  hipLaunchKernelGGL(k_tri_levels, dim3(1), dim3(kSeqBlock), 0, st_, T, tri_lds_form());
}

}  // namespace pies
