// Device helpers shared by the CG kernels of the PD global step (pd_cg_kernels.hip: the two-launch iteration,
// pd_cg1_kernels.hip: one launch per iteration) and by the kernels that close a solve's statistics.
#pragma once
#include <cstdint>

#include "dev_math.h"
#include "pd_kernels.h"

namespace pies {

constexpr int kBlock = 256;

// ------------------------------------------------------------------------------------------------------
// Jacobi-preconditioned CG, 3 right-hand sides at once.  Launch shape: workgroups of 256 threads; a wavefront takes slices of
// the matrix (64 / lanesPerRow rows), the workgroups of one XCD a contiguous part of them (xcd_sweep).  nparts workgroups where a
// launch may have to go on behind grid_barrier, npartsI where not (CgArrays).  Dot products: per-workgroup partials, re-reduced
// in a fixed order by every workgroup of the consuming kernel (deterministic, no atomics, no extra launch).
//   partI[b]         = { r.z[3], r.r[3], f.f[3] } of the first residual   (k_cg_init, k_cg1_init)
//   two-launch form:   partA[b] = { p.Ap[3] } (k_cg_ap),  partB0 / partB1[b] = { r.z[3], r.r[3] } (k_cg_update, ping-pong)
//   one-launch form:   part1[h][b] = { r.t[3], w.t[3], r.r[3] } (k_cg1_first, k_cg1_iter, ping-pong; partCount: how many b)
//   scal, stats      : the solve's scalars and the solves' statistics, by the names of CgScal and CgStat (pd_kernels.h)
// What both forms share is stated once, here: the walk over a row's entries (row_entries), the residual of a row (row_residual),
// a row's contact part (contact_row, contact_rows_of_node), opening a solve and marking it over (solve_open, solve_over).
// ------------------------------------------------------------------------------------------------------
template <int NV> PIES_DEV void block_reduce_partials(const float* __restrict__ part, int stride, uint32_t nparts, float out[NV]) {
  __shared__ float lds[4][NV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = 0.0f;
  for (uint32_t t = threadIdx.x; t < nparts; t += kBlock)  // fixed order: the same sum in every block
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] += part[t * stride + k];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] += __shfl_xor(acc[k], off, 64);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) lds[wave][k] = acc[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) out[k] = ((lds[0][k] + lds[1][k]) + lds[2][k]) + lds[3][k];
  __syncthreads();
}

template <int NV> PIES_DEV void block_write_partial(const float acc_in[NV], float* __restrict__ part, int stride) {
  __shared__ float lds[4][NV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = acc_in[k];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] += __shfl_xor(acc[k], off, 64);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) lds[wave][k] = acc[k];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) part[blockIdx.x * stride + k] = ((lds[0][k] + lds[1][k]) + lds[2][k]) + lds[3][k];
  __syncthreads();
}

PIES_DEV bool all_converged(const float rr[3], const float bb[3], float tol2) {
  return rr[0] <= tol2 * bb[0] && rr[1] <= tol2 * bb[1] && rr[2] <= tol2 * bb[2];
}

// Off-diagonal part of the contact blocks w*AtA for row i (the diagonal 3w / w is in cdiag): the point couples
// to the three triangle nodes with -w, each triangle node to the point with -w.  FETCH(j) returns the vector at j.
// The terms are added in contact-list order; the loads of four contacts are requested together (index, ids, then
// the vectors - three dependent trips per batch instead of per contact: a node of a contact patch sits in tens of
// contacts, and one lane walking them one by one made the SpMV ten times slower than without contacts).
// (kAhead: contacts whose loads are requested together; the one-launch-per-iteration kernels, whose fetch is three gathers, take 1:
// twelve fetches in flight cost them 60 registers for a path a contact-light substep takes for a handful of rows)
// ACC: float, or double in the residual kernels (the row's contact terms are w = 1e4 times coordinates and cancel against the
// right-hand side like the elastic terms do: summed in fp32 with thousands of contacts the residual - and with it the solution -
// carried 2.6 x the deviation of the reference's own fp32 solve from the fp64 yardstick; tests/test_tri_collisions_gpu.py)
template <int kAhead = 4, class ACC = float, class Fetch> PIES_DEV void contact_row(const CgArrays& A, uint32_t i, Fetch fetch, ACC& sx, ACC& sy, ACC& sz) {
  if (!A.tIncCnt || *A.tUsedCount == 0u) return;  // (no contact in this substep: one uniform word instead of a load per row)
  const uint32_t tc = A.tIncCnt[i];
  if (!tc) return;
  if (A.useCAp && A.rowLen) {  // the merged row of this substep exists (contact-heavy variant; reached from the CG continuation)
    const uint32_t len = A.rowLen[i];
    if (len != 0xffffffffu) {
      const uint32_t off = A.rowStart[i];
      for (uint32_t t = 0; t < len; ++t) {
        const float coef = A.rowCoef[off + t];
        float q[3];
        fetch(A.rowCol[off + t], q[0], q[1], q[2]);
        sx = fma(static_cast<ACC>(coef), static_cast<ACC>(q[0]), sx); sy = fma(static_cast<ACC>(coef), static_cast<ACC>(q[1]), sy);
        sz = fma(static_cast<ACC>(coef), static_cast<ACC>(q[2]), sz);
      }
      return;
    }
  }
  const uint32_t ts = A.tIncStart[i];
  for (uint32_t k0 = 0; k0 < tc; k0 += kAhead) {
    uint32_t v[kAhead];
    uint4 id[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) v[u] = A.tInc[ts + min(k0 + u, tc - 1)];  // clamped: unconditional loads
#pragma unroll
    for (int u = 0; u < kAhead; ++u) id[u] = A.tIds[v[u] >> 2];
    float q[kAhead][3][3];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const bool point = (v[u] & 3u) == 0u;  // the point's row couples to the three triangle nodes, their rows to the point
      fetch(point ? id[u].y : id[u].x, q[u][0][0], q[u][0][1], q[u][0][2]);
      fetch(id[u].z, q[u][1][0], q[u][1][1], q[u][1][2]);
      fetch(id[u].w, q[u][2][0], q[u][2][1], q[u][2][2]);
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      if (k0 + u >= tc) break;
      const int terms = (v[u] & 3u) == 0u ? 3 : 1;
#pragma unroll
      for (int t = 0; t < 3; ++t)
        if (t < terms) {
          sx = fma(static_cast<ACC>(-kTriContactW), static_cast<ACC>(q[u][t][0]), sx);
          sy = fma(static_cast<ACC>(-kTriContactW), static_cast<ACC>(q[u][t][1]), sy);
          sz = fma(static_cast<ACC>(-kTriContactW), static_cast<ACC>(q[u][t][2]), sz);
        }
    }
  }
}

// What a wavefront or a workgroup sweeps, begin / end / step in units of its own: workgroups that share an XCD (equal
// blockIdx % 8, see xcd_block) take one contiguous segment of the `units`, so what one of them gathers was fetched into that
// XCD's L2 by its neighbours.  A workgroup takes `each` units per step, this thread the one numbered `mine` among them.
struct Sweep {
  uint32_t begin, end, step;
};
PIES_DEV Sweep xcd_sweep(uint32_t units, uint32_t nblocks, uint32_t each, uint32_t mine) {  // nblocks: the launch's sweeping blocks (the first ones)
  const uint32_t labels = nblocks < 8u ? nblocks : 8u;
  const uint32_t x = blockIdx.x % labels, xb = blockIdx.x / labels;
  const uint32_t nbx = (nblocks - x + labels - 1u) / labels;  // blocks carrying this label
  const uint32_t segBeg = static_cast<uint32_t>((static_cast<uint64_t>(units) * x) / labels);
  const uint32_t segEnd = static_cast<uint32_t>((static_cast<uint64_t>(units) * (x + 1u)) / labels);
  return {segBeg + xb * each + mine, segEnd, nbx * each};
}
// the slices (64 / LPR rows) a wavefront sweeps
template <int LPR> PIES_DEV Sweep slice_sweep(uint32_t n, uint32_t nblocks) {
  constexpr uint32_t kRows = 64u / LPR;
  return xcd_sweep((n + kRows - 1u) / kRows, nblocks, kBlock / 64u, threadIdx.x >> 6);
}

// f(value, column) for every stored entry that lane `lane` of slice `sl` holds of row i: the row dictionary (one lane per row
// only) or the SELL arrays, whose indexing is the same at every lane count
template <int LPR = 1, class F> PIES_DEV void row_entries(const CgArrays& A, uint32_t sl, uint32_t lane, uint32_t i, F f) {
  if (LPR == 1 && A.rowStencil) {
    if (i < A.n) {
      const uint32_t rs = A.rowStencil[i];
      const uint32_t b = rs & 0xffffffu, e = b + (rs >> 24);
#pragma unroll 4
      for (uint32_t q = b; q < e; ++q) {
        const int2 pr = A.stencil[q];
        f(__int_as_float(pr.y), static_cast<uint32_t>(static_cast<int>(i) + pr.x));
      }
    }
  } else {
    const uint32_t off = A.sliceOff[sl], width = (A.sliceOff[sl + 1] - off) >> 6;
#pragma unroll 4
    for (uint32_t kk = 0; kk < width; ++kk) {
      const uint32_t at = off + (kk << 6) + lane;
      f(A.val[at], A.col[at]);  // (padding entries: the row itself with value 0)
    }
  }
}

// The residual of row i: r = f - (cdiag x + K x + C x), given the row's sums (K x) = k* and (C x) = c*, then z = D^-1 r and
// acc9 += {r.z, r.r, f.f}.  In DOUBLE: the products are ~ (m / h^2) |x| ~ 1e6 and cancel against f to a residual five orders
// smaller; summed in fp32 the row carries a noise of an ulp of 1e6 (0.1: 2e-5 in x per solve, a random walk over the local/global
// iterations - measured against the oracle's fp64 solve: 2.3 x the deviation of the reference's own fp32 arithmetic, in every
// variant of the local step and of the CG).  fp64 fused multiply-adds cost these memory-bound launches nothing.
// C: the type the caller summed the contact part in (k_cg_init: float, k_cg1_init: double - see there).
template <class C>
PIES_DEV Vec3f row_residual(const CgArrays& A, uint32_t i, const float4 xi, const float4 fi, double kx, double ky, double kz, C cx, C cy, C cz,
                            Vec3f& z, float acc9[9]) {
  const float cd = A.cdiag[i], di = A.dinv[i];
  const double cdd = static_cast<double>(cd);
  const float rx = static_cast<float>(static_cast<double>(fi.x) - (fma(cdd, static_cast<double>(xi.x), kx) + static_cast<double>(cx)));
  const float ry = static_cast<float>(static_cast<double>(fi.y) - (fma(cdd, static_cast<double>(xi.y), ky) + static_cast<double>(cy)));
  const float rz = static_cast<float>(static_cast<double>(fi.z) - (fma(cdd, static_cast<double>(xi.z), kz) + static_cast<double>(cz)));
  z = Vec3f{di * rx, di * ry, di * rz};
  acc9[0] += rx * z.x; acc9[1] += ry * z.y; acc9[2] += rz * z.z;
  acc9[3] += rx * rx; acc9[4] += ry * ry; acc9[5] += rz * rz;
  acc9[6] += fi.x * fi.x; acc9[7] += fi.y * fi.y; acc9[8] += fi.z * fi.z;
  return Vec3f{rx, ry, rz};
}

// Statistics at the end of a solve (max relative residual over the tick's solves, iterations of the solve): run by one
// block, either of k_cg_finish or - for every solve but the last of a substep - of the next solve's k_cg_init, which
// saves a launch per local/global iteration.  prevPartB holds the finished solve's final residual partials.
PIES_DEV void solve_statistics(const CgArrays& A, const float* __restrict__ prevPartB) {
  float red[6];
  // a solve that converged before its last captured iteration left its final partials where k_cg_ap found them
  // (solve_over; kScalWhere = 0: partI, 1 / 2: the ping-pong pair); otherwise the last k_cg_update wrote prevPartB
  const bool done = A.scal[kScalOver] != 0.0f;
  const int where = static_cast<int>(A.scal[kScalWhere]);
  if (done && where == 0 && A.single) {  // (k_cg1_first left the norms in kScalFinalRr: partI belongs to the next solve by now)
#pragma unroll
    for (int c = 0; c < 3; ++c) red[3 + c] = A.scal[kScalFinalRr + c];
  }
  else if (done && where == 0) block_reduce_partials<6>(A.partI, 9, A.nparts, red);
  else if (A.single) {  // one launch per iteration: {r.t, w.t, r.r} per workgroup, the residual norms in the last three
    const float* last = done ? A.part1[where - 1] : prevPartB;
    block_reduce_partials<3>(last + 6, 9, A.partCount[last == A.part1[1] ? 1 : 0], red + 3);
  }
  else block_reduce_partials<6>(done ? (where == 1 ? A.partB0 : A.partB1) : prevPartB, 6, A.nparts, red);
  if (threadIdx.x == 0) {
    float worst = 0.f;
    bool above = false;  // the very test the CG kernels take their early exit on (all_converged)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float bb = A.scal[kScalBb + c];
      const float rel = bb > 0.f ? red[3 + c] / bb : 0.f;
      worst = fmaxf(worst, rel);
      above = above || !(red[3 + c] <= A.tol2 * bb);
    }
    A.stats[kStatWorst] = fmaxf(A.stats[kStatWorst], worst);
    A.stats[kStatIters] = fmaxf(A.stats[kStatIters], A.scal[kScalIters]);
    A.stats[kStatSolves] += 1.0f;
    const float ranShort = above ? 1.0f : 0.0f;  // the solve used its whole captured budget and is still above the tolerance
    A.stats[kStatShort] += ranShort;
    unsigned long long* life = reinterpret_cast<unsigned long long*>(A.stats + kStatLife);
    life[0] += above ? 1ull : 0ull;
    life[1] += 1ull;
  }
}

// The bookkeeping workgroup that opens a solve (one behind the launch's row blocks: inside block 0 it delayed that block's rows
// by 2-3 us): it closes the previous solve's statistics (prevPart != nullptr: its final partials; its scal[] entries are still
// intact, this solve's second launch is the first to overwrite them) and clears what the solve's launches tell each other.
PIES_DEV void solve_open(const CgArrays& A, const float* __restrict__ prevPart) {
  if (prevPart) solve_statistics(A, prevPart);
  if (threadIdx.x == 0) {
    A.scal[kScalOver] = 0.0f;  // this solve is not over yet
    A.ticket[0] = 0u;          // grid barrier counter of the solve's last launch
    A.ticket[1] = 0u;          // its abort word
  }
}

// The solve is over after `iterations` of them: it converged, or it went on inside its last launch and ended there.  Every later
// launch of the solve returns on kScalOver; solve_statistics finds the final residual partials by `where` (CgScal).
PIES_DEV void solve_over(const CgArrays& A, int where, int iterations) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  A.scal[kScalIters] = static_cast<float>(iterations);
  A.scal[kScalWhere] = static_cast<float>(where);
  A.scal[kScalOver] = 1.0f;
}

// Contact part of (K + C) v for the nodes that take part in contacts, one wavefront per node: lane t takes the node's
// incidences t, t + 64, ... (list order inside a lane), the 64 partial sums are combined pairwise.  Used by the
// contact-heavy graph variant only (CgArrays::useCAp): a node of a contact patch sits in tens to hundreds of contacts, and
// the row's single lane walking them inside the SpMV made one CG iteration ~10x longer.
// the wavefront's sum over one node's contact rows; fetch(j, qx, qy, qz) reads the vector
template <class Fetch> PIES_DEV void contact_rows_of_node(const CgArrays& A, uint32_t node, uint32_t lane, Fetch fetch, float& sx, float& sy, float& sz) {
  const uint32_t tc = A.tIncCnt[node], ts = A.tIncStart[node];
  sx = 0.f; sy = 0.f; sz = 0.f;
  const uint32_t len = A.rowLen ? A.rowLen[node] : 0xffffffffu;
  if (len != 0xffffffffu) {  // merged row: one gather of the distinct columns (a handful per node), coefficient = -w * multiplicity
    const uint32_t off = A.rowStart[node];
    for (uint32_t t = lane; t < len; t += 64) {
      const float coef = A.rowCoef[off + t];
      float q[3];
      fetch(A.rowCol[off + t], q[0], q[1], q[2]);
      sx = fmaf(coef, q[0], sx); sy = fmaf(coef, q[1], sy); sz = fmaf(coef, q[2], sz);
    }
  } else
  for (uint32_t t = lane; t < tc; t += 64) {
    const uint32_t v = A.tInc[ts + t];
    const uint4 id = A.tIds[v >> 2];
    const bool point = (v & 3u) == 0u;
    float q0[3], q1[3] = {0.f, 0.f, 0.f}, q2[3] = {0.f, 0.f, 0.f};
    fetch(point ? id.y : id.x, q0[0], q0[1], q0[2]);
    if (point) { fetch(id.z, q1[0], q1[1], q1[2]); fetch(id.w, q2[0], q2[1], q2[2]); }
    sx = fmaf(-kTriContactW, q0[0], sx); sy = fmaf(-kTriContactW, q0[1], sy); sz = fmaf(-kTriContactW, q0[2], sz);
    if (point) {
      sx = fmaf(-kTriContactW, q1[0], sx); sy = fmaf(-kTriContactW, q1[1], sy); sz = fmaf(-kTriContactW, q1[2], sz);
      sx = fmaf(-kTriContactW, q2[0], sx); sy = fmaf(-kTriContactW, q2[1], sy); sz = fmaf(-kTriContactW, q2[2], sz);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    sx += __shfl_xor(sx, off, 64);
    sy += __shfl_xor(sy, off, 64);
    sz += __shfl_xor(sz, off, 64);
  }
}

// the LPR lanes of a row combine their partial sums (pairwise; every lane of the row ends with the total)
template <int LPR> PIES_DEV void row_combine(float& sx, float& sy, float& sz) {
#pragma unroll
  for (int off = LPR / 2; off >= 1; off >>= 1) {
    sx += __shfl_xor(sx, off, LPR);
    sy += __shfl_xor(sy, off, LPR);
    sz += __shfl_xor(sz, off, LPR);
  }
}

// Barrier across the workgroups of a launch whose workgroups are all resident (k_cg_update: at most 1024 of 256 threads with
// a few hundred bytes of LDS, the chip holds 5 x 256 of them).  `counter` only grows (the solve's first kernel zeroes it);
// release before the arrival, acquire after the last one, as a grid-wide synchronisation has to.  The wait is bounded: a
// workgroup that gives up returns false and leaves, the others follow at their next barrier (the solve then stays where it
// was and is counted as short).
PIES_DEV bool grid_barrier(uint32_t* counter, uint32_t nblocks, uint32_t& passed) {
  __shared__ uint32_t sOk;
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    atomicAdd(counter, 1u);
    const uint32_t target = (passed + 1u) * nblocks;
    uint32_t spins = 0, ok = 1u;
    while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(2);
      if (++spins > (1u << 20)) { ok = 0u; break; }  // ~1 s
    }
    // a workgroup that gives up says so in the abort word; one that arrives late and finds the counter already past its
    // target (the others have left) must not run an iteration alone: everybody checks the word after the wait
    if (!ok) __hip_atomic_store(counter + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if (__hip_atomic_load(counter + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ok = 0u;
    __threadfence();
    sOk = ok;
  }
  __syncthreads();
  ++passed;
  return sOk != 0u;
}

}  // namespace pies
