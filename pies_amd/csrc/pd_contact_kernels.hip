// PD node-node contacts (PIES_FLAG_PD_NODE_CONTACTS): detection, the contacts' share of the local step and their friction loop.
// The reference defines the pieces - Solver::_parallelComputeCollisions (Src/Solver.cpp:509-637), CollisionConstraint
// (Src/CollisionConstraint.cpp:7-65), the friction loop over the constraint list (Src/Solver.cpp:398-428) - but never fills the
// list.  Everything here is one lane per node: a node's partners sit in a fixed-stride list that its own lane writes, the
// right-hand side and the diagonal are summed by that lane in list order, and the friction loop runs in rounds in which every
// pair that is the next unprocessed pair of both its nodes is resolved.  No float atomics: a run is reproducible bit for bit.
#include <algorithm>
#include <cstdint>

#include "dev_math.h"
#include "floor_friction.h"
#include "hash_device.h"
#include "pd_contact_kernels.h"

namespace pies {

constexpr int kNcBlock = 256;

// the host's id of device node i < C.n (the pair key and the roles a, b of a pair are the host's: pd_contact_kernels.h)
PIES_DEV uint32_t nc_host(const NodeContactArrays& C, uint32_t i) { return C.hostId ? C.hostId[i] : i; }

PIES_DEV bool nc_joined(const NodeContactArrays& C, uint32_t i, uint32_t j) {  // binary search of node i's element neighbours
  uint32_t lo = C.adjPtr[i], hi = C.adjPtr[i + 1];
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const uint32_t v = C.adj[mid];
    if (v == j) return true;
    if (v < j) lo = mid + 1; else hi = mid;
  }
  return false;
}

// One lane per node.  The candidates are the nodes of the buckets of the node's cell range (the grid of the PBD pass, built from the
// predicted positions: Solver.cpp:240 detects there); a pair that shares several cells is taken in the first cell both ranges
// share - the minimum corner of the ranges' intersection -, by both its nodes' lanes.  The contact test is the projection's own
// (CollisionConstraint.cpp:20-24, |p_i - p_j|^2 < (r_i + r_j)^2 in fp32) plus invMass_i + invMass_j > 0 (the projection divides by
// it, :36) and no element between the two.  Then the list is sorted by pair key and the diagonal gets w
// once per contact (CollisionConstraint.cpp:43-47).
__global__ void __launch_bounds__(kNcBlock) k_nc_detect(HashArrays H, NodeContactArrays C, const float4* __restrict__ pos,
                                                        const float* __restrict__ radius, const float* __restrict__ kdiag,
                                                        float* __restrict__ cdiag, float* __restrict__ dinv) {
  const uint32_t i = blockIdx.x * kNcBlock + threadIdx.x;
  if (i < kNcDeepest) C.ctl[i] = 0u;  // the friction pass's round words (not the host's [kNcDeepest])
  if (i >= C.n) return;
  C.cur[0][i] = 0u;
  uint32_t* __restrict__ list = C.part + static_cast<size_t>(i) * C.cap;
  uint32_t c = 0;
  if (H.counters[kCounterFlags] == 0u) {  // (a failed build: no contacts; the host latches the failure)
    const GridBox B = grid_box(H.counters);
    const uint32_t* __restrict__ val = H.val[grid_passes(B) & 1u];
    const int4 r = H.rng[i];
    const uint32_t lx = static_cast<uint32_t>(r.w) & 255u, ly = (static_cast<uint32_t>(r.w) >> 8) & 255u, lz = (static_cast<uint32_t>(r.w) >> 16) & 255u;
    const float4 pi = pos[i];
    const float ri = radius[i];
    for (uint32_t dx = 0; dx < lx; ++dx)
      for (uint32_t dy = 0; dy < ly; ++dy)
        for (uint32_t dz = 0; dz < lz; ++dz) {
          const int x = r.x + static_cast<int>(dx), y = r.y + static_cast<int>(dy), z = r.z + static_cast<int>(dz);
          const uint32_t slot = find_bucket(H, B, x, y, z);
          if (slot == 0xffffffffu) continue;
          const uint32_t be = H.end[slot];
          for (uint32_t e = H.start[slot]; e < be; ++e) {
            const uint32_t j = val[e] & kNodeMask;
            if (j == i || j >= C.n) continue;
            const int4 rj = H.rng[j];
            if (x != max(r.x, rj.x) || y != max(r.y, rj.y) || z != max(r.z, rj.z)) continue;  // not the first shared cell
            const float4 pj = pos[j];
            const float ex = pj.x - pi.x, ey = pj.y - pi.y, ez = pj.z - pi.z;
            const float distSq = ex * ex + ey * ey + ez * ez;
            const float rr = ri + radius[j];
            if (!(distSq < rr * rr)) continue;
            if (!(pi.w + pj.w > 0.0f)) continue;
            if (nc_joined(C, i, j)) continue;
            if (c < C.cap) list[c] = j;
            ++c;
          }
        }
    if (c > C.cap) {  // more partners than the list holds: latched like the grid's own failures (pies_failed / pies_last_error)
      atomicOr(&H.counters[kCounterFlags], kNcOverflowFlag);
      c = C.cap;
    }
    const uint32_t hi = nc_host(C, i);
    for (uint32_t a = 1; a < c; ++a) {  // ascending pair key of the host's ids (insertion sort: a handful of partners)
      const uint32_t v = list[a];
      const uint64_t kv = pair_mix(hi, nc_host(C, v));
      uint32_t b = a;
      while (b > 0 && pair_mix(hi, nc_host(C, list[b - 1])) > kv) { list[b] = list[b - 1]; --b; }
      list[b] = v;
    }
    if (c) {
      float cd = cdiag[i];
      for (uint32_t k = 0; k < c; ++k) cd += kNodePairW;  // coeffRef(i, i) += w once per contact
      cdiag[i] = cd;
      dinv[i] = 1.0f / (kdiag[i] + cd);
    }
  }
  C.cnt[i] = c;
}

// CollisionConstraint::project for the pair {a < b} (CollisionConstraint.cpp:10-41, the arithmetic of k_pd_local_node_pair): the
// projected position of node `self`
PIES_DEV void nc_project(float4 a, float4 b, float ra, float rb, bool selfIsA, float& px, float& py, float& pz) {
  px = selfIsA ? a.x : b.x; py = selfIsA ? a.y : b.y; pz = selfIsA ? a.z : b.z;
  const float dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
  const float distSq = dx * dx + dy * dy + dz * dz;
  const float r = ra + rb;
  if (distSq < r * r) {
    const float dist = sqrtf(distSq);
    const float dispLength = r - dist;
    float ex, ey, ez;
    if (dist > 0.00001f) { ex = dispLength * dx / dist; ey = dispLength * dy / dist; ez = dispLength * dz / dist; }
    else { ex = dispLength; ey = 0.0f; ez = 0.0f; }
    const float wSum = a.w + b.w;
    if (selfIsA) { px -= ex * a.w / wSum; py -= ey * a.w / wSum; pz -= ez * a.w / wSum; }
    else { px += ex * b.w / wSum; py += ey * b.w / wSum; pz += ez * b.w / wSum; }
  }
}

__global__ void __launch_bounds__(kNcBlock) k_nc_rhs(NodeContactArrays C, const float4* __restrict__ pos, const float* __restrict__ radius,
                                                     float4* __restrict__ rhs) {
  const uint32_t i = blockIdx.x * kNcBlock + threadIdx.x;
  if (i >= C.n) return;
  const uint32_t c = C.cnt[i];
  if (c == 0) return;
  const uint32_t* __restrict__ list = C.part + static_cast<size_t>(i) * C.cap;
  const float4 pi = pos[i];
  const float ri = radius[i];
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  for (uint32_t k = 0; k < c; ++k) {
    const uint32_t j = list[k];
    const float4 pj = pos[j];
    const float rj = radius[j];
    float px, py, pz;
    if (nc_host(C, i) < nc_host(C, j)) nc_project(pi, pj, ri, rj, true, px, py, pz);  // (a is the node with the lower host id)
    else nc_project(pj, pi, rj, ri, false, px, py, pz);
    sx += kNodePairW * px; sy += kNodePairW * py; sz += kNodePairW * pz;
  }
  const float4 b = rhs[i];
  rhs[i] = make_float4(b.x + sx, b.y + sy, b.z + sz, b.w);
}

// The friction of the pair {a < b} (Solver.cpp:398-428 over CollisionConstraint's nodes; k_pd_node_pair_friction's arithmetic)
PIES_DEV void nc_friction_pair(const float4* __restrict__ pos, float4* __restrict__ vel, const float* __restrict__ radius, uint32_t ia,
                               uint32_t ib, float frictionOpt, float staticThreshold) {
  const float4 a = pos[ia], b = pos[ib];
  const float dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
  const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
  if (dist > radius[ia] + radius[ib]) return;
  const float nx = dx / dist, ny = dy / dist, nz = dz / dist;
  float4 va = vel[ia], vb = vel[ib];
  const float rx = vb.x - va.x, ry = vb.y - va.y, rz = vb.z - va.z;
  const float rn = rx * nx + ry * ny + rz * nz;
  const float px = rx - rn * nx, py = ry - rn * ny, pz = rz - rn * nz;
  float friction = -frictionOpt;
  if (sqrtf(px * px + py * py + pz * pz) < staticThreshold) friction = 1.0f;
  const float wSum = a.w + b.w;
  va.x += -friction * px * a.w / wSum; va.y += -friction * py * a.w / wSum; va.z += -friction * pz * a.w / wSum;
  vb.x += friction * px * b.w / wSum; vb.y += friction * py * b.w / wSum; vb.z += friction * pz * b.w / wSum;
  vel[ia] = va;
  vel[ib] = vb;
}

// One round for node i: its next pair {i, j} runs when it is also j's next pair (the lower node's lane resolves it).  The pairs that
// run in one round share no node, and each is the lowest-keyed unprocessed pair of both its nodes: the rounds give the sequential
// loop over the pairs in ascending key, bit for bit.  Cursors are read from `in` and written to `out` (each lane its own), so a lane
// never sees a cursor moved in the same round.  Returns whether node i still has pairs left.
PIES_DEV bool nc_round_node(const NodeContactArrays& C, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t i,
                            const float4* __restrict__ pos, float4* __restrict__ vel, const float* __restrict__ radius, float friction,
                            float staticThreshold) {
  const uint32_t c = C.cnt[i];
  uint32_t p = in[i];
  if (p < c) {
    const uint32_t j = C.part[static_cast<size_t>(i) * C.cap + p];
    const uint32_t pj = in[j];
    const bool ready = pj < C.cnt[j] && C.part[static_cast<size_t>(j) * C.cap + pj] == i;
    if (ready && i < j) nc_friction_pair(pos, vel, radius, i, j, friction, staticThreshold);
    if (ready) ++p;
  }
  out[i] = p;
  return p < c;
}

__global__ void __launch_bounds__(kNcBlock) k_nc_friction_round(NodeContactArrays C, const float4* __restrict__ pos, float4* __restrict__ vel,
                                                                const float* __restrict__ radius, uint32_t round, float friction,
                                                                float staticThreshold) {
  if ((round > 0 && C.ctl[round] == 0u) || (*C.flags & kNcOverflowFlag)) return;  // every pair is done; a truncated list
  const uint32_t i = blockIdx.x * kNcBlock + threadIdx.x;
  bool left = false;
  if (i < C.n) left = nc_round_node(C, C.cur[round & 1u], C.cur[(round & 1u) ^ 1u], i, pos, vel, radius, friction, staticThreshold);
  if (__any(left) && (threadIdx.x & 63u) == 0u) atomicOr(&C.ctl[round + 1u], 1u);
}

// The rounds beyond the captured ones, in one workgroup (slow, never wrong); records how deep the pass went.
__global__ void __launch_bounds__(1024) k_nc_friction_tail(NodeContactArrays C, const float4* __restrict__ pos, float4* __restrict__ vel,
                                                           const float* __restrict__ radius, float friction, float staticThreshold) {
  __shared__ uint32_t more;
  uint32_t round = C.rounds;
  uint32_t depth = 0;
  for (uint32_t r = 1; r <= C.rounds; ++r)
    if (C.ctl[r]) depth = r + 1u;
  // (the lists are symmetric, so every round resolves at least the lowest-keyed pair left: the loop ends; an overflowed list is not)
  const uint32_t maxRounds = C.rounds + C.n * (C.cap / 2u) + 2u;
  if (C.ctl[round] != 0u && !(*C.flags & kNcOverflowFlag)) {
    for (;;) {
      __syncthreads();
      if (threadIdx.x == 0) more = 0u;
      __syncthreads();
      bool left = false;
      for (uint32_t i = threadIdx.x; i < C.n; i += 1024u)
        left |= nc_round_node(C, C.cur[round & 1u], C.cur[(round & 1u) ^ 1u], i, pos, vel, radius, friction, staticThreshold);
      if (left) more = 1u;
      __threadfence_block();
      __syncthreads();
      ++round;
      if (!more || round >= maxRounds) break;
    }
    depth = round;
  }
  if (threadIdx.x == 0 && depth) atomicMax(&C.ctl[kNcDeepest], depth);
}

// Solver.cpp:473-484 for the nodes in a node contact and in no point-triangle contact (the velocity kernel leaves them out; those in a
// point-triangle contact get it from launch_tri_friction)
__global__ void __launch_bounds__(kNcBlock) k_nc_floor_friction(NodeContactArrays C, float4* __restrict__ vel, const uint32_t* __restrict__ nstatic,
                                                                const uint32_t* __restrict__ usedBits, float friction, float staticThreshold) {
  const uint32_t i = blockIdx.x * kNcBlock + threadIdx.x;
  if (i >= C.n || C.cnt[i] == 0u) return;
  if (usedBits && ((usedBits[i >> 5] >> (i & 31u)) & 1u)) return;
  const uint32_t ns = nstatic[i];
  if (ns == 0u) return;
  const float4 v = vel[i];
  float vx = v.x, vy = v.y, vz = v.z;
  floor_friction(vx, vy, vz, ns, friction, staticThreshold);
  vel[i] = make_float4(vx, vy, vz, v.w);
}

static inline dim3 nc_grid(uint32_t n) { return dim3((n + kNcBlock - 1) / kNcBlock); }

uint32_t launch_nc_detect(hipStream_t st, const HashArrays& H, const NodeContactArrays& C, const NodeArrays& nd, const float* kdiag,
                          float* cdiag, float* dinv) {
  if (C.n == 0) return 0;
  const uint32_t blocks = std::max(nc_grid(C.n).x, (kNcCtlWords + kNcBlock - 1) / kNcBlock);
  hipLaunchKernelGGL(k_nc_detect, dim3(blocks), dim3(kNcBlock), 0, st, H, C, nd.pos, nd.radius, kdiag, cdiag, dinv);
  return 1;
}
uint32_t launch_nc_rhs(hipStream_t st, const NodeContactArrays& C, const NodeArrays& nd, float4* rhs) {
  if (C.n == 0) return 0;
  hipLaunchKernelGGL(k_nc_rhs, nc_grid(C.n), dim3(kNcBlock), 0, st, C, nd.pos, nd.radius, rhs);
  return 1;
}
uint32_t launch_nc_friction(hipStream_t st, const NodeContactArrays& C, const HashArrays& H, const NodeArrays& nd, const uint32_t* nstatic,
                            const uint32_t* usedBits, float friction, float staticThreshold) {
  (void)H;
  if (C.n == 0) return 0;
  for (uint32_t r = 0; r < C.rounds; ++r)
    hipLaunchKernelGGL(k_nc_friction_round, nc_grid(C.n), dim3(kNcBlock), 0, st, C, nd.pos, nd.vel, nd.radius, r, friction, staticThreshold);
  hipLaunchKernelGGL(k_nc_friction_tail, dim3(1), dim3(1024), 0, st, C, nd.pos, nd.vel, nd.radius, friction, staticThreshold);
  hipLaunchKernelGGL(k_nc_floor_friction, nc_grid(C.n), dim3(kNcBlock), 0, st, C, nd.vel, nstatic, usedBits, friction, staticThreshold);
  return C.rounds + 2u;
}

}  // namespace pies
