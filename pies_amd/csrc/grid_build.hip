// The node grid of the PBD substep: the broad phase of every node-node order, of the PD node contacts and of the grid-build
// roofline (reference: Include/Pies/SpatialHash.h, Src/Solver.cpp:877-901).
//
// The reference keeps a parallel_flat_hash_map<CellId, vector<Node*>> that is cleared and rebuilt every solver iteration by 16
// threads which each scan all nodes.  Here the grid is rebuilt on the device as a sort:
//   (1) k_grid_range   every node computes its cell range with the reference's NodeCompRange arithmetic (up to 50 cells per axis,
//                      like the reference) and the number of cells it overlaps; the bounding box of a workgroup's ranges goes to
//                      boxPart[workgroup] (block_box_reduce), and the first workgroup zeroes the build's counters;
//   (2) prefix sum     of the per-node cell counts -> each node's first entry (k_scan_tiles, k_scan_sums; the tile sums are added
//                      by k_grid_emit).  An extra workgroup of k_scan_tiles reduces the partial boxes to the build's box and latches
//                      a box whose key the captured sort cannot hold (failure bit 512);
//   (3) k_grid_emit    one (cell key, node) entry per overlapped cell, node-major.  The key packs the cell's coordinates relative
//                      to the bounding box with just the bits the box needs (axis_bits), so a scene of 23 x 45 x 45 cells sorts on
//                      17 bits; a key of at most 32 bits travels through the sort in one word with its value;
//   (4) radix sort     least-significant-digit, stable: histogram, prefix sum of the (digit, workgroup) counts, scatter with
//                      ballot-based ranks.  The host captures as many passes as the box it last saw needs at up to kRadixMaxDigit
//                      (11) bits per pass, and the key's bits are dealt evenly to them (grid_box): 17 bits are two passes of 9.
//                      Stable + node-major input = every bucket lists its nodes in ascending index, which is the reference's
//                      bucket order (its insert threads scan the nodes in index order);
//   (5) k_grid_cells   bucket boundaries from neighbouring keys; each bucket's [start, end) goes into the cell index - the key
//                      itself as the slot where the index is long enough (direct_index), otherwise exact-key open addressing
//                      (full 64-bit compare: two cells never alias, the reference's map is exact as well);
//   (6) k_grid_groups  (group order only) per cell the nodes whose minimum cell it is, and the cell's place in the list of its
//                      residue class.
// What resolves on this grid: group_resolve.hip (group order, reference order), pair_lists.hip / pair_levels.hip / pair_turns.hip
// (the orders by dependency levels), pd_contact_kernels.hip.
#include <climits>
#include <cstdint>
#include <cstdlib>

#include "cell_table.h"
#include "hash_kernels.h"
#include "hash_device.h"

namespace pies {

constexpr int kBlock = 256;

static inline dim3 grid_for(uint32_t n) { return dim3((n + kBlock - 1) / kBlock); }

// ---- reset: only the index slots the previous build used; counters; bounding box --------------------------------
__global__ void __launch_bounds__(kBlock) k_grid_reset(HashArrays H) {
  const uint32_t used = H.counters[kCounterUsed];
  for (uint32_t u = blockIdx.x * kBlock + threadIdx.x; u < used; u += gridDim.x * kBlock) {
    const uint32_t s = H.used[u];
    H.keys[s] = kEmpty;
  }
}
// ---- range: NodeCompRange + cells per node + bounding box ---------------------------------------------------------
PIES_DEV int wave_min(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
  return v;
}
PIES_DEV int wave_max(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}
// The box of a workgroup of kBlock threads from its threads' boxes (lo, hi: min and max cell per axis): six words per wavefront,
// through LDS, six results - thread a < 6 gets word a of (min x, y, z, max x, y, z).  Every thread calls.
PIES_DEV int block_box_reduce(int (&lo)[3], int (&hi)[3]) {
  __shared__ int part[kBlock / 64][6];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = wave_min(lo[a]);
    hi[a] = wave_max(hi[a]);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { part[threadIdx.x >> 6][a] = lo[a]; part[threadIdx.x >> 6][3 + a] = hi[a]; }
  }
  __syncthreads();
  int v = 0;
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    v = part[0][a];
    for (int w = 1; w < kBlock / 64; ++w) v = a < 3 ? min(v, part[w][a]) : max(v, part[w][a]);
  }
  return v;
}
__global__ void __launch_bounds__(kBlock) k_grid_range(HashArrays H, const float4* __restrict__ pos, const float* __restrict__ radius,
                                                       uint32_t n, float scale) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (blockIdx.x == 0) {  // the build's counters (k_grid_zero's work: nothing in this launch reads them; k_grid_reset, which needs the
    const uint32_t t = threadIdx.x;  // previous build's cell count, runs before it)
    if (t == kCounterUsed || t == kCounterEntries || t == kCounterSpare || t == kCounterDense) H.counters[t] = 0;
    if (t >= kCounterPass0 && t < kCounterPass0 + 27) H.counters[t] = 0;
    if (t == kCounterTicket) H.counters[t] = 0;
    if (t == kCounterEpoch) H.counters[t] += 1;
  }
  int mx = 0, my = 0, mz = 0;
  uint32_t lx = 0, ly = 0, lz = 0;
  if (i < n) {
    const float4 p = pos[i];
    if (!node_range(p.x, p.y, p.z, radius[i], scale, mx, my, mz, lx, ly, lz)) atomicOr(&H.counters[kCounterFlags], kFailNonFinite);
    H.rng[i] = make_int4(mx, my, mz, static_cast<int>(lx | (ly << 8) | (lz << 16)));
    H.entCount[i] = lx * ly * lz;
  }
  if (i == n) H.entCount[n] = 0;  // so that the exclusive prefix sum ends with the total
  const bool have = i < n && lx * ly * lz != 0u;
  int lo[3] = {have ? mx : INT_MAX, have ? my : INT_MAX, have ? mz : INT_MAX};
  int hi[3] = {have ? mx + static_cast<int>(lx) - 1 : INT_MIN, have ? my + static_cast<int>(ly) - 1 : INT_MIN,
               have ? mz + static_cast<int>(lz) - 1 : INT_MIN};
  // -> boxPart[workgroup]; grid_box_reduce reduces the partial boxes (six global atomics per wavefront on six words took 0.5 ms
  // at 500k nodes)
  const int v = block_box_reduce(lo, hi);
  if (threadIdx.x < 6) H.boxPart[blockIdx.x * 6 + threadIdx.x] = v;
}
// ---- exclusive prefix sum of uint32 (tile sums, scan of the sums, add) -----------------------------------------
constexpr uint32_t kScanTile = 2048;  // 256 threads x 8
PIES_DEV uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds, uint32_t& total) {  // 256 threads; lds: 8 words
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(incl, off, 64);
    if (lane >= static_cast<uint32_t>(off)) incl += t;
  }
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  uint32_t base = 0;
  for (uint32_t w = 0; w < wave; ++w) base += lds[w];
  total = lds[0] + lds[1] + lds[2] + lds[3];
  __syncthreads();
  return base + incl - v;
}
// the bounding box of the nodes' cell ranges from the workgroups' partial boxes, and the sort this build runs (k_grid_box's
// work for a workgroup of kBlock threads: it rides behind the tiles of k_scan_tiles, one launch less per rebuild)
PIES_DEV void grid_box_reduce(const HashArrays& H, uint32_t nparts, uint32_t sortPasses) {
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  for (uint32_t b = threadIdx.x; b < nparts; b += kBlock) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = min(lo[a], H.boxPart[b * 6 + a]);
      hi[a] = max(hi[a], H.boxPart[b * 6 + 3 + a]);
    }
  }
  const int v = block_box_reduce(lo, hi);
  static_assert(kCounterBoxMax == kCounterBoxMin + 3, "the box's six words are consecutive");
  if (threadIdx.x < 6) H.counters[kCounterBoxMin + threadIdx.x] = static_cast<uint32_t>(v);
  if (threadIdx.x < 64) {  // the sort of this build: the captured passes, and whether they can hold the box's key
    uint32_t total = 0;
    bool empty = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int lo_ = __shfl(v, a, 64), hi_ = __shfl(v, 3 + a, 64);
      if (hi_ < lo_) empty = true;
      total += axis_bits(empty ? 0u : static_cast<uint32_t>(hi_ - lo_));
    }
    if (threadIdx.x == 0) {
      H.counters[kCounterSortPasses] = sortPasses;
      if (!empty && total > kRadixMaxDigit * sortPasses) atomicOr(&H.counters[kCounterFlags], kFailSortTooShort);
    }
  }
}
__global__ void __launch_bounds__(kBlock) k_scan_tiles(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n,
                                                       uint32_t* __restrict__ sums, HashArrays H, uint32_t boxParts, uint32_t sortPasses) {
  if (boxParts && blockIdx.x + 1u == gridDim.x) {  // (uniform per workgroup)
    grid_box_reduce(H, boxParts, sortPasses);
    return;
  }
  __shared__ uint32_t lds[8];
  const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * 8u;
  uint32_t v[8], s = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    v[k] = base + k < n ? in[base + k] : 0u;
    s += v[k];
  }
  uint32_t total;
  uint32_t run = block_exclusive_scan(s, lds, total);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (base + k < n) out[base + k] = run;
    run += v[k];
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ void __launch_bounds__(1024) k_scan_sums(uint32_t* __restrict__ sums, uint32_t m) {  // one workgroup, in place
  __shared__ uint32_t part[1024];
  const uint32_t t = threadIdx.x, per = (m + 1023u) / 1024u;
  const uint32_t lo = min(m, t * per), hi = min(m, lo + per);
  uint32_t s = 0;
  for (uint32_t k = lo; k < hi; ++k) s += sums[k];
  part[t] = s;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan of the 1024 partial sums
    const uint32_t a = t >= off ? part[t - off] : 0u;
    __syncthreads();
    part[t] += a;
    __syncthreads();
  }
  uint32_t run = part[t] - s;
  for (uint32_t k = lo; k < hi; ++k) {
    const uint32_t v = sums[k];
    sums[k] = run;
    run += v;
  }
}
// ---- emit: one (cell key, node) entry per overlapped cell, node-major --------------------------------------------
// A wavefront's 64 nodes own one contiguous stretch of the entry list (entOff is node-major).  The lanes write it slot by slot -
// lane l takes slots l, l + 64, ... of the stretch and finds the node a slot belongs to by a binary search over the lanes'
// offsets - so that a store instruction covers 64 consecutive entries.  (One lane writing its own node's entries one after the
// other put 64 separate 8-byte pieces into every store: 33 us for 4 M entries.)
__global__ void __launch_bounds__(kBlock) k_grid_emit(HashArrays H, uint32_t n) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if (i == 0) {
    const uint32_t total = H.entOff[n] + H.scanSums[n / kScanTile];
    if (total > H.maxEntries) atomicOr(&H.counters[kCounterFlags], kFailEntries);
    H.counters[kCounterEntries] = min(total, H.maxEntries);
  }
  const bool live = i < n;
  const int4 rg = live ? H.rng[i] : make_int4(0, 0, 0, 0);
  const uint32_t lx = rg.w & 0xff, ly = (rg.w >> 8) & 0xff, lz = (rg.w >> 16) & 0xff;
  const uint32_t base = live ? H.entOff[i] + H.scanSums[i / kScanTile] : 0u;  // (the tile sums are added here: k_scan_add's launch)
  uint32_t cnt = live ? lx * ly * lz : 0u;
  if (base + cnt > H.maxEntries) cnt = 0;  // flagged above: the host latches the failure
  const GridBox B = grid_box(H.counters);
  // offsets of the lanes' nodes inside the wavefront's stretch
  uint32_t incl = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  const uint32_t pre = incl - cnt, total = __shfl(incl, 63, 64);
  const uint32_t waveBase = __shfl(base, 0, 64);  // (lane 0 is live whenever any lane of the wavefront is)
  for (uint32_t j0 = 0; j0 < total; j0 += 64) {
    const uint32_t j = j0 + static_cast<uint32_t>(lane);
    // the node slot j belongs to: the last lane whose offset is <= j (lanes without entries share their offset with the next)
    uint32_t l = 0;
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
      const uint32_t pm = __shfl(pre, static_cast<int>(l) + step, 64);
      if (pm <= j) l += static_cast<uint32_t>(step);
    }
    const uint32_t pl = __shfl(pre, static_cast<int>(l), 64);
    const int ox = __shfl(rg.x, static_cast<int>(l), 64), oy = __shfl(rg.y, static_cast<int>(l), 64), oz = __shfl(rg.z, static_cast<int>(l), 64);
    const uint32_t ow = static_cast<uint32_t>(__shfl(rg.w, static_cast<int>(l), 64));
    const uint32_t ob = __shfl(base, static_cast<int>(l), 64);
    if (j >= total) continue;
    const uint32_t oly = (ow >> 8) & 0xff, olz = (ow >> 16) & 0xff, olx = ow & 0xff;
    const uint32_t e = j - pl, lyz = oly * olz;
    const uint32_t dx = e / lyz, r = e - dx * lyz, dy = r / olz, dz = r - dy * olz;
    const uint32_t node = blockIdx.x * kBlock + (threadIdx.x & ~63u) + l;
    const uint32_t side = (dx ? 4u : 0u) | (dy ? 2u : 0u) | (dz ? 1u : 0u);
    const uint32_t twoLong = (olx == 2u ? 4u : 0u) | (oly == 2u ? 2u : 0u) | (olz == 2u ? 1u : 0u);
    const uint64_t key = box_key(B, ox + static_cast<int>(dx), oy + static_cast<int>(dy), oz + static_cast<int>(dz));
    const uint32_t val = node | (twoLong << kLongShift) | (side << kSideShift) | (e == 0 ? kMinFlag : 0u);  // e == 0: the node's minimum cell
    // A key of at most 32 bits (any scene but one that spans billions of cells) travels through the sort in one word with its
    // value: 8 bytes per entry and pass instead of 8 + 4.  The last pass writes the values out for the kernels that read them.
    if (B.packed) H.key[0][ob + e] = (key << 32) | val;
    else { H.key[0][ob + e] = key; H.val[0][ob + e] = val; }
  }
  (void)waveBase;
}

// ---- radix sort of the entries by key: B.digit bits per pass, stable ------------------------------------------------
// Pass p reads buffer p & 1 and writes the other one.  A workgroup owns kRadixTile consecutive entries; wavefront w of
// it the w-th quarter, sixteen rounds of 64 consecutive entries - so (workgroup, wavefront, round, lane) is the input order.
__global__ void __launch_bounds__(kBlock) k_radix_hist(HashArrays H, uint32_t pass, uint32_t nblkMax) {
  __shared__ uint32_t h[1u << kRadixMaxDigit];
  const GridBox B = grid_box(H.counters);
  if (pass >= grid_passes(B)) return;
  const uint32_t bins = 1u << B.digit, shift = B.digit * pass + (B.packed ? 32u : 0u);
  const uint32_t E = H.counters[kCounterEntries];
  const uint32_t blk = blockIdx.x;
  if (blk * kRadixTile >= E) return;
  const uint64_t* __restrict__ src = H.key[pass & 1u];
  for (uint32_t d = threadIdx.x; d < bins; d += kBlock) h[d] = 0;
  __syncthreads();
  uint64_t kk[kRadixTile / kBlock];  // all sixteen loads in flight before the first LDS atomic
#pragma unroll
  for (uint32_t k = 0; k < kRadixTile / kBlock; ++k) {
    const uint32_t t = blk * kRadixTile + k * kBlock + threadIdx.x;
    kk[k] = t < E ? src[t] : ~0ull;
  }
#pragma unroll
  for (uint32_t k = 0; k < kRadixTile / kBlock; ++k) {
    const uint32_t t = blk * kRadixTile + k * kBlock + threadIdx.x;
    if (t < E) atomicAdd(&h[static_cast<uint32_t>(kk[k] >> shift) & (bins - 1u)], 1u);
  }
  __syncthreads();
  for (uint32_t d = threadIdx.x; d < bins; d += kBlock) H.hist[d * nblkMax + blk] = h[d];
}
// Prefix sums of the (digit, workgroup) counts in digit-major order, in two steps: workgroup d of this kernel turns row d
// (the counts of digit d over the sorting workgroups) into its exclusive prefix and leaves the row's total in
// hist[256 * nblkMax + d]; the scatter kernel adds the exclusive prefix of the 256 totals.
__global__ void __launch_bounds__(kBlock) k_radix_scan(HashArrays H, uint32_t pass, uint32_t nblkMax) {
  __shared__ uint32_t lds[8];
  const GridBox B = grid_box(H.counters);
  if (pass >= grid_passes(B) || blockIdx.x >= (1u << B.digit)) return;
  const uint32_t E = H.counters[kCounterEntries];
  const uint32_t nblk = (E + kRadixTile - 1u) / kRadixTile;
  uint32_t* __restrict__ row = H.hist + static_cast<size_t>(blockIdx.x) * nblkMax;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nblk; base += kBlock) {
    const uint32_t k = base + threadIdx.x;
    const uint32_t v = k < nblk ? row[k] : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(v, lds, total);
    if (k < nblk) row[k] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) H.hist[(1u << kRadixMaxDigit) * nblkMax + blockIdx.x] = carry;
}
__global__ void __launch_bounds__(kBlock) k_radix_scatter(HashArrays H, uint32_t pass, uint32_t nblkMax) {
  constexpr uint32_t kBins = 1u << kRadixMaxDigit;
  __shared__ uint32_t cnt[4][kBins];  // per wavefront: running count of a digit, then the wavefront's base inside the workgroup
  __shared__ uint32_t gbase[kBins];
  __shared__ uint32_t scanLds[8];
  const GridBox B = grid_box(H.counters);
  if (pass >= grid_passes(B)) return;
  const uint32_t bins = 1u << B.digit, shift = B.digit * pass + (B.packed ? 32u : 0u);
  const bool packed = B.packed, last = pass + 1u == grid_passes(B);
  const uint32_t E = H.counters[kCounterEntries];
  const uint32_t blk = blockIdx.x;
  if (blk * kRadixTile >= E) return;
  const uint64_t* __restrict__ skey = H.key[pass & 1u];
  const uint32_t* __restrict__ sval = H.val[pass & 1u];
  uint64_t* __restrict__ dkey = H.key[(pass & 1u) ^ 1u];
  uint32_t* __restrict__ dval = H.val[(pass & 1u) ^ 1u];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  constexpr int kRounds = kRadixTile / kBlock;  // 16
  for (uint32_t d = lane; d < bins; d += 64u) cnt[wave][d] = 0;
  __builtin_amdgcn_wave_barrier();
  uint64_t key[kRounds];
  uint32_t val[kRounds], rank[kRounds];
  const uint32_t first = blk * kRadixTile + wave * (kRadixTile / 4u);
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const uint32_t t = first + static_cast<uint32_t>(r) * 64u + lane;
    const bool valid = t < E;
    key[r] = valid ? skey[t] : 0ull;
    val[r] = (valid && !packed) ? sval[t] : 0u;
  }
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const uint32_t t = first + static_cast<uint32_t>(r) * 64u + lane;
    const bool valid = t < E;
    const uint32_t d = static_cast<uint32_t>(key[r] >> shift) & (bins - 1u);
    unsigned long long peers = __ballot(valid);  // lanes of this round holding the same digit
#pragma unroll
    for (int b = 0; b < static_cast<int>(kRadixMaxDigit); ++b) {
      if (static_cast<uint32_t>(b) < B.digit) {  // (uniform)
        const bool bit = (d >> b) & 1u;
        const unsigned long long m = __ballot(valid && bit);
        peers &= bit ? m : ~m;
      }
    }
    rank[r] = 0;
    if (valid) {
      const uint32_t before = cnt[wave][d];
      rank[r] = before + static_cast<uint32_t>(__popcll(peers & ((1ull << lane) - 1ull)));
      if (static_cast<uint32_t>(__builtin_ctzll(peers)) == lane) cnt[wave][d] = before + static_cast<uint32_t>(__popcll(peers));
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {  // per digit: the wavefronts' bases inside the workgroup, and the workgroup's base in the output.  A thread takes
    // kBins / kBlock consecutive digits (their totals scanned in the thread, the threads' sums across the workgroup)
    constexpr uint32_t kPer = kBins / kBlock;  // 8
    const uint32_t d0 = threadIdx.x * kPer;
    uint32_t tot[kPer], mine = 0;
#pragma unroll
    for (uint32_t q = 0; q < kPer; ++q) {
      const uint32_t d = d0 + q;
      tot[q] = d < bins ? H.hist[kBins * nblkMax + d] : 0u;
      mine += tot[q];
      if (d < bins) {
        uint32_t run = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const uint32_t c = cnt[w][d];
          cnt[w][d] = run;
          run += c;
        }
      }
    }
    uint32_t all;
    uint32_t digitBase = block_exclusive_scan(mine, scanLds, all);  // entries with a smaller digit
#pragma unroll
    for (uint32_t q = 0; q < kPer; ++q) {
      const uint32_t d = d0 + q;
      if (d < bins) gbase[d] = digitBase + H.hist[d * nblkMax + blk];
      digitBase += tot[q];
    }
  }
  __syncthreads();
  // (Round 4 measured the tile put into sorted order in LDS first and written out from there, so that a store instruction
  // covers the runs of a few digits instead of 64 entries in 64 cache lines: 41.8 us per pass against 36.5 - the pass is not
  // bound by its store pattern, and the 32 KB of staging cost a resident workgroup per CU.)
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const uint32_t t = first + static_cast<uint32_t>(r) * 64u + lane;
    if (t < E) {
      const uint32_t d = static_cast<uint32_t>(key[r] >> shift) & (bins - 1u);
      const uint32_t at = gbase[d] + cnt[wave][d] + rank[r];
      dkey[at] = key[r];
      if (!packed) dval[at] = val[r];
      else if (last) dval[at] = static_cast<uint32_t>(key[r]);  // (the values, for the kernels behind the sort)
    }
  }
}

// ---- cells: bucket boundaries -> cell index; groups per pass ------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_grid_cells(HashArrays H) {
  // a workgroup takes kRadixTile consecutive entries; the cells it creates are collected in LDS and appended to the list
  // of cells in use with ONE global atomic (47k appends on one word took 0.4 ms at 500k nodes; round 4 tried one entry per
  // thread - 16 000 workgroups, 16 000 appends: 184 us against 38).  A thread's sixteen entries are requested together.
  __shared__ uint32_t made[kRadixTile];  // at most one cell per entry of the tile (buckets of one node)
  __shared__ uint32_t nmade, base;
  const uint32_t E = H.counters[kCounterEntries];
  const uint32_t first = blockIdx.x * kRadixTile;
  if (first >= E) return;
  if (threadIdx.x == 0) nmade = 0;
  __syncthreads();
  const GridBox B = grid_box(H.counters);
  const uint32_t fb = grid_passes(B) & 1u;  // the buffer the last pass wrote
  const uint64_t* __restrict__ key = H.key[fb];
  const uint32_t ksh = B.packed ? 32u : 0u;  // (a packed entry: the key is the upper word)
  const bool direct = direct_index(H, B);
  constexpr uint32_t kRounds = kRadixTile / kBlock;
  uint64_t kp[kRounds], kc[kRounds], kn[kRounds];
#pragma unroll
  for (uint32_t r = 0; r < kRounds; ++r) {
    const uint32_t t = first + r * kBlock + threadIdx.x;
    const uint32_t tc = min(t, E - 1u);
    kc[r] = key[tc] >> ksh;
    kp[r] = key[tc ? tc - 1u : 0u] >> ksh;
    kn[r] = key[min(tc + 1u, E - 1u)] >> ksh;
  }
#pragma unroll
  for (uint32_t r = 0; r < kRounds; ++r) {
    const uint32_t t = first + r * kBlock + threadIdx.x;
    if (t >= E) continue;
    const uint64_t k = kc[r];
    const bool head = t == 0 || kp[r] != k;
    const bool tail = t + 1 == E || kn[r] != k;
    if (!(head || tail)) continue;
    bool created;
    uint32_t slot;
    if (direct) {  // the key is the slot (hash_device.h: direct_index): the bucket's head entry creates the cell
      slot = static_cast<uint32_t>(k);
      created = head;
      if (head) H.keys[slot] = k;
    } else {
      slot = insert_cell(H.keys, H.mask, k, created);  // whichever of the bucket's two ends comes first creates it
    }
    if (slot == 0xffffffffu) { atomicOr(&H.counters[kCounterFlags], kFailIndex); continue; }
    if (created) made[atomicAdd(&nmade, 1u)] = slot;
    if (head) H.start[slot] = t;
    if (tail) H.end[slot] = t + 1;
  }
  __syncthreads();
  if (threadIdx.x == 0 && nmade) base = atomicAdd(&H.counters[kCounterUsed], nmade);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < nmade; k += kBlock) H.used[base + k] = made[k];
}
// one lane per cell in use: its group size (entries carrying kMinFlag) and its place in the pass list.  Places are handed
// out per workgroup: one global atomic per (workgroup, pass) instead of one per cell on 27 words.
__global__ void __launch_bounds__(kBlock) k_grid_groups(HashArrays H) {
  __shared__ uint32_t lcount[27], lbase[27];
  const uint32_t used = H.counters[kCounterUsed];
  const GridBox B = grid_box(H.counters);
  const uint32_t* __restrict__ val = H.val[grid_passes(B) & 1u];
  for (uint32_t first = blockIdx.x * kBlock; first < used; first += gridDim.x * kBlock) {  // uniform per workgroup
    if (threadIdx.x < 27) lcount[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t u = first + threadIdx.x;
    uint32_t s = 0, pass = 0, rank = 0, gc = 0;
    if (u < used) {
      s = H.used[u];
      const uint32_t bs = H.start[s], be = H.end[s];
      if (be - bs > kMaxBucket) H.counters[kCounterDense] = 1u;  // a pile the group order's tables do not hold: the sequential loop takes the pass
      for (uint32_t e = bs; e < be; ++e) gc += val[e] >> 31;
      H.gcnt[s] = gc;
      if (gc) {
        int x, y, z;
        box_cell(B, H.keys[s], x, y, z);
        pass = static_cast<uint32_t>(mod3(x) + 3 * mod3(y) + 9 * mod3(z));
        rank = atomicAdd(&lcount[pass], 1u);
      }
    }
    __syncthreads();
    if (threadIdx.x < 27 && lcount[threadIdx.x]) lbase[threadIdx.x] = atomicAdd(&H.counters[kCounterPass0 + threadIdx.x], lcount[threadIdx.x]);
    __syncthreads();
    if (gc) H.passList[static_cast<size_t>(pass) * H.n + lbase[pass] + rank] = s;
    __syncthreads();
  }
}

// ----------------------------------------------------------------------------------------------------
uint32_t launch_hash_build(hipStream_t st_, const HashArrays& H, const NodeArrays& nd, float scale, uint32_t sortPasses, bool groups) {
  if (nd.n == 0) return 0;
  const uint32_t n = nd.n;
  uint32_t launches = 0;
  const dim3 wide(std::min<uint32_t>(2048u, (H.capacity / 8 + kBlock - 1) / kBlock));
  // (round 4: three launches fewer - the counters are zeroed by the first workgroup of k_grid_range, the bounding box is reduced
  // by an extra workgroup of k_scan_tiles, the tile sums are added by k_grid_emit itself)
  hipLaunchKernelGGL(k_grid_reset, wide, dim3(kBlock), 0, st_, H); ++launches;
  hipLaunchKernelGGL(k_grid_range, grid_for(n + 1), dim3(kBlock), 0, st_, H, nd.pos, nd.radius, n, scale); ++launches;
  const uint32_t m = n + 1, tiles = (m + kScanTile - 1) / kScanTile;
  hipLaunchKernelGGL(k_scan_tiles, dim3(tiles + 1u), dim3(kBlock), 0, st_, H.entCount, H.entOff, m, H.scanSums, H, grid_for(n + 1).x, sortPasses); ++launches;
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, st_, H.scanSums, tiles); ++launches;
  hipLaunchKernelGGL(k_grid_emit, grid_for(n), dim3(kBlock), 0, st_, H, n); ++launches;
  const uint32_t nblkMax = (H.maxEntries + kRadixTile - 1) / kRadixTile;
  for (uint32_t pass = 0; pass < sortPasses; ++pass) {  // the key's bits are dealt evenly to the passes (grid_box)
    hipLaunchKernelGGL(k_radix_hist, dim3(nblkMax), dim3(kBlock), 0, st_, H, pass, nblkMax);
    hipLaunchKernelGGL(k_radix_scan, dim3(1u << kRadixMaxDigit), dim3(kBlock), 0, st_, H, pass, nblkMax);
    hipLaunchKernelGGL(k_radix_scatter, dim3(nblkMax), dim3(kBlock), 0, st_, H, pass, nblkMax);
    launches += 3;
  }
  hipLaunchKernelGGL(k_grid_cells, dim3(nblkMax), dim3(kBlock), 0, st_, H); ++launches;
  if (groups) { hipLaunchKernelGGL(k_grid_groups, wide, dim3(kBlock), 0, st_, H); ++launches; }
  return launches;
}

}  // namespace pies
