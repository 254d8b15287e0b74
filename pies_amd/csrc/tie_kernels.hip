// Ties (tie_kernels.h; the rule is stated in pies_hip.h, lives in tie_rule.h and is restated in numpy by tests/test_ties.py).
//  k_tie_evaluate  one lane per TIE of the set's own order.  The groups (at most 64 x 20 bytes) are staged in LDS; a lane reads its
//                  record (four uint4), maps the four host ids through P.inv and gathers four velocities - the gathers are element
//                  granular and served by L2: a seam's nodes are few beside the cache.  The FIRST iteration also gathers the four
//                  positions, forms x, W and den, decides broken and live, and leaves (x, den) and (q - pivot, group | live bit) in
//                  the tie's scratch, so a later iteration reads no position.  Every iteration writes the change of J with the live
//                  word beside it and the running J beside the stretch; the LAST writes the torque entry k_anchor_sums reads.  A
//                  record of five words per group makes neighbouring groups start on different banks.
//  k_tie_scatter   one lane per TIED node (the set's compact list of host ids): it walks the node's row - (tie, coefficient) pairs,
//                  consecutive, ascending tie index - eight at a time, adds the live entries' changes from 0.0f in the row's order
//                  and stores the velocity in place.  No lane reads a velocity in this launch, so there is no scratch variant.
//                  One lane per node: a row of hundreds of entries is one lane's serial walk (DESIGN.md section 8m has the length
//                  from which it dominates the call).
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written in tie_rule.h.
#include "tie_kernels.h"

#include "tie_rule.h"
#include "node_edit_device.h"

namespace pies {
namespace {

constexpr uint32_t kTieBatch = 8;  // entries of a row in flight in k_tie_scatter

PIES_DEV uint32_t tie_device_index(const PropPass& P, uint32_t host) { return P.inv ? P.inv[host] : host; }

template <bool kFirst>
__global__ void __launch_bounds__(kPropTile) k_tie_evaluate(TiePass A, bool last) {
  __shared__ pies_tie_group_t groups[PIES_TIE_GROUP_MAX];
  const PropPass& P = A.base;
  stage_records(groups, A.groups, P.nProps);
  __syncthreads();
  const uint32_t i = blockIdx.x * kPropTile + threadIdx.x;
  if (i >= A.nTies) return;  // (no barrier follows)
  const TieRecord R = A.records[i];
  const pies_tie_group_t& g = groups[R.group];
  const float h = A.dt;
  const uint32_t na = tie_device_index(P, R.node), n0 = tie_device_index(P, R.to[0]), n1 = tie_device_index(P, R.to[1]),
                 n2 = tie_device_index(P, R.to[2]);

  V3 x, arm;
  float den, stretch;
  uint32_t word;
  V3 J{0.0f, 0.0f, 0.0f};
  if (kFirst) {
    const float4 pa = P.nd.pos[na], p0 = P.nd.pos[n0], p1 = P.nd.pos[n1], p2 = P.nd.pos[n2];
    const V3 q = tie_carried(xyz(p0), xyz(p1), xyz(p2), R.weight);
    x = sub(xyz(pa), q);
    stretch = sqrtf(dot(x, x));
    const float W = tie_inverse_mass(R, pa.w, p0.w, p1.w, p2.w);
    den = tie_den(tie_spring(R, g.strength, h), h, W);
    arm = sub(q, load3(g.pivot));
    const bool was = A.broken[i] != 0;
    const bool broken = was || tie_breaks(stretch, g.break_stretch);
    if (broken && !was) A.broken[i] = 1;
    word = R.group | (tie_live(broken, g.strength, W) ? kAnchorLiveBit : 0u);
    A.scratch[2 * i] = make_float4(x.x, x.y, x.z, den);
    A.scratch[2 * i + 1] = make_float4(arm.x, arm.y, arm.z, __uint_as_float(word));
  } else {
    const float4 s0 = A.scratch[2 * i], s1 = A.scratch[2 * i + 1];
    x = xyz(s0);
    den = s0.w;
    arm = xyz(s1);
    word = __float_as_uint(s1.w);
    const float4 j4 = A.impulse[i];
    J = xyz(j4);
    stretch = j4.w;
  }
  const bool live = (word & kAnchorLiveBit) != 0;

  if (live && h > 0.0f) {  // (h: uniform)
    const float4 va = P.nd.vel[na], v0 = P.nd.vel[n0], v1 = P.nd.vel[n1], v2 = P.nd.vel[n2];
    const V3 r = sub(xyz(va), tie_carried(xyz(v0), xyz(v1), xyz(v2), R.weight));
    const V3 dJ = tie_delta(tie_spring(R, g.strength, h), x, r, h, J, den);
    J = add(J, dJ);
    A.delta[i] = make_float4(dJ.x, dJ.y, dJ.z, __uint_as_float(1u));
    A.impulse[i] = make_float4(J.x, J.y, J.z, stretch);
  } else if (kFirst) {  // (a later iteration leaves what the first wrote)
    A.delta[i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0u));
    A.impulse[i] = make_float4(0.0f, 0.0f, 0.0f, stretch);
  }
  if (last && A.torque) {  // (uniform: kernel arguments)
    V3 tq{0.0f, 0.0f, 0.0f};
    if (live) tq = cross(arm, J);
    A.torque[i] = make_float4(tq.x, tq.y, tq.z, __uint_as_float(word));
  }
}

__global__ void __launch_bounds__(kPropTile) k_tie_scatter(TiePass A) {
  const PropPass& P = A.base;
  const uint32_t a = blockIdx.x * kPropTile + threadIdx.x;
  if (a >= A.nNodes) return;
  const uint32_t i = tie_device_index(P, A.nodes[a]);
  const float w = P.nd.pos[i].w;
  if (w == 0.0f) return;
  V3 sum{0.0f, 0.0f, 0.0f};
  bool any = false;
  // kTieBatch entries and then their changes are requested together, so a long row waits for one round trip per batch and not per
  // entry; the sum keeps the row's order
  for (uint32_t e = A.offsets[a], end = A.offsets[a + 1]; e < end; e += kTieBatch) {
    const uint32_t m = min(kTieBatch, end - e);
    TieEntry E[kTieBatch];
    float4 d[kTieBatch];
#pragma unroll
    for (uint32_t j = 0; j < kTieBatch; ++j) E[j] = A.entries[e + (j < m ? j : 0u)];
#pragma unroll
    for (uint32_t j = 0; j < kTieBatch; ++j) d[j] = A.delta[E[j].tie];
#pragma unroll
    for (uint32_t j = 0; j < kTieBatch; ++j) {
      if (j >= m || __float_as_uint(d[j].w) == 0u) continue;  // past the row's end, or not live
      sum = add(sum, scale(xyz(d[j]), E[j].coefficient));
      any = true;
    }
  }
  if (!any) return;
  const float4 v4 = P.nd.vel[i];
  const V3 v1 = add(xyz(v4), scale(sum, w));
  P.nd.vel[i] = make_float4(v1.x, v1.y, v1.z, v4.w);
}

}  // namespace

void launch_tie_evaluate(hipStream_t st, const TiePass& P, bool first, bool last) {
  if (!P.base.nd.n || !P.nTies || !P.base.nProps || P.base.nProps > PIES_TIE_GROUP_MAX || !P.groups || !P.records || !P.broken ||
      !P.delta || !P.impulse || !P.scratch)
    return;
  if (first) hipLaunchKernelGGL(k_tie_evaluate<true>, dim3(anchor_tiles(P.nTies)), dim3(kPropTile), 0, st, P, last);
  else hipLaunchKernelGGL(k_tie_evaluate<false>, dim3(anchor_tiles(P.nTies)), dim3(kPropTile), 0, st, P, last);
}

void launch_tie_scatter(hipStream_t st, const TiePass& P) {
  if (!P.base.nd.n || !P.nNodes || !P.nodes || !P.offsets || !P.entries || !P.delta) return;
  hipLaunchKernelGGL(k_tie_scatter, dim3(anchor_tiles(P.nNodes)), dim3(kPropTile), 0, st, P);
}

void launch_tie_sums(hipStream_t st, const TiePass& P) {
  AnchorPass S;
  S.base = P.base;
  S.nAnchors = P.nTies;
  S.impulse = P.impulse;
  S.torque = P.torque;
  launch_anchor_sums(st, S);
}

}  // namespace pies
