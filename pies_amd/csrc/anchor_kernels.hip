// Anchors (anchor_kernels.h; the rule is stated in pies_hip.h, lives in anchor_rule.h and is restated in numpy by
// tests/test_anchors.py).
//  k_anchor_evaluate  one lane per ANCHORED node (the set's compact list of host ids; edit_lane_at gives the device index under
//                     renumbering).  The frames (at most 64 x 88 bytes) are staged in LDS and read as broadcasts; a lane walks its
//                     node's records (32 bytes each, consecutive in the sorted list) once for A and G, solves, and stores the
//                     velocity in place - no lane reads another node, so there is no scratch variant.  A pin stores position,
//                     previous position and velocity.  When the host asked for anything back the lane walks the records a second
//                     time from the state it loaded - the same functions on the same operands, the same bits - and writes j,
//                     stretch, torque and (frame | live bit) of EVERY anchor, live or not, at the anchor's index in the set's
//                     own order.
//  k_anchor_sums      one workgroup per tile of 256 anchor indices: the tile's entries go to LDS (eight words per anchor, so the
//                     seven lanes of a frame read seven banks), a 64-bit word collects the frames present, and one lane per
//                     (present frame, component) adds the tile's entries of that frame in ascending index - another frame's
//                     anchor would add 0, which changes no bit of a sum that started at +0.  k_prop_fold folds the tiles.
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written in anchor_rule.h.
#include "anchor_kernels.h"

#include "anchor_rule.h"
#include "node_edit_device.h"

namespace pies {
namespace {

__global__ void __launch_bounds__(kPropTile) k_anchor_evaluate(AnchorPass A) {
  __shared__ pies_anchor_frame_t frames[PIES_ANCHOR_FRAME_MAX];
  const PropPass& P = A.base;
  stage_records(frames, A.frames, P.nProps);
  __syncthreads();
  const uint32_t a = blockIdx.x * kPropTile + threadIdx.x;
  const bool mine = a < A.nNodes;
  EditLane L = edit_lane_at(P, mine ? A.nodes[a] : 0u, mine);
  if (!L.live) return;  // (no barrier follows)
  const uint32_t first = A.offsets[a], end = A.offsets[a + 1];
  const float h = A.dt;

  // ---- first walk: the edit ----
  float sumA = 0.0f;
  V3 sumG{0.0f, 0.0f, 0.0f}, e{0.0f, 0.0f, 0.0f};
  bool springs = false;
  for (uint32_t r = first; r < end; ++r) {
    const AnchorRecord R = A.records[r];
    const pies_anchor_frame_t& f = frames[R.frame];
    if (!anchor_live(L.w, f.strength)) continue;
    need_velocity(P, L);
    const AnchorTarget T = anchor_target(f, R.local, L.p);
    if (R.flags & PIES_ANCHOR_PIN) {  // (the node's only anchor)
      P.nd.pos[L.i] = make_float4(T.t.x, T.t.y, T.t.z, L.w);
      P.nd.prev[L.i] = make_float4(T.t.x, T.t.y, T.t.z, 0.0f);  // (.w unused: 0 as the predict kernels and the upload write it)
      P.nd.vel[L.i] = make_float4(T.u.x, T.u.y, T.u.z, L.velW);
    } else {
      const AnchorSpring S = anchor_spring(R.stiffness, R.damping, f.strength, h, T, L.v);
      sumA = sumA + S.a;
      sumG = add(sumG, S.g);
      springs = true;
    }
  }
  if (springs) {
    e = anchor_solve(sumG, sumA, h, L.w);
    const V3 v1 = add(L.v, e);
    P.nd.vel[L.i] = make_float4(v1.x, v1.y, v1.z, L.velW);
  }
  if (!A.impulse) return;  // (uniform: a kernel argument)

  // ---- second walk: every anchor's entry, from the state the lane loaded ----
  for (uint32_t r = first; r < end; ++r) {
    const AnchorRecord R = A.records[r];
    const pies_anchor_frame_t& f = frames[R.frame];
    const AnchorTarget T = anchor_target(f, R.local, L.p);
    const bool live = anchor_live(L.w, f.strength);
    V3 j{0.0f, 0.0f, 0.0f}, tq{0.0f, 0.0f, 0.0f};
    if (live) {
      j = (R.flags & PIES_ANCHOR_PIN) ? anchor_pin_impulse(T.u, L.v, L.w)
                                      : anchor_spring_impulse(anchor_spring(R.stiffness, R.damping, f.strength, h, T, L.v), e, h);
      tq = cross(T.arm, j);
    }
    A.impulse[R.index] = make_float4(j.x, j.y, j.z, T.stretch);
    A.torque[R.index] = make_float4(tq.x, tq.y, tq.z, __uint_as_float(R.frame | (live ? kAnchorLiveBit : 0u)));
  }
}

__global__ void __launch_bounds__(kPropTile) k_anchor_sums(const float4* __restrict__ impulse, const float4* __restrict__ torque,
                                                           uint32_t nAnchors, uint32_t nFrames, uint64_t* __restrict__ tileMask,
                                                           float* __restrict__ tileSums) {
  __shared__ float4 stage[kPropTile][2];  // per anchor of the tile: (j, stretch), (torque, frame | live bit)
  __shared__ uint64_t waveSet[kPropWaves];
  const uint32_t tid = threadIdx.x, tile = blockIdx.x, i = tile * kPropTile + tid;
  uint64_t set = 0;
  if (i < nAnchors) {
    const float4 t4 = torque[i];
    stage[tid][0] = impulse[i];
    stage[tid][1] = t4;
    set = 1ull << (__float_as_uint(t4.w) & 63u);  // (a frame's index is below PIES_ANCHOR_FRAME_MAX = 64)
  }
  for (int offset = 32; offset > 0; offset >>= 1) set |= __shfl_xor(set, offset);
  if ((tid & 63u) == 0) waveSet[tid >> 6] = set;
  __syncthreads();
  set = 0;
  for (uint32_t w = 0; w < kPropWaves; ++w) set |= waveSet[w];
  if (tid == 0) tileMask[tile] = set;
  const uint32_t count = min(kPropTile, nAnchors - tile * kPropTile);
  const uint32_t items = 7u * __builtin_popcountll(set);
  const uint32_t* words = reinterpret_cast<const uint32_t*>(&stage[0][0]);  // anchor j: words[8 j ..]: j x y z, stretch, torque x y z, the word
  for (uint32_t item = tid; item < items; item += kPropTile) {
    const uint32_t slot = item / 7u, c = item % 7u;
    uint64_t m = set;
    for (uint32_t k = 0; k < slot; ++k) m &= m - 1;
    const uint32_t f = __builtin_ctzll(m);
    uint32_t* record = reinterpret_cast<uint32_t*>(tileSums) + (static_cast<size_t>(tile) * nFrames + f) * kPropSumWords;
    if (c < 6) {
      const uint32_t src = c < 3 ? c : c + 1;
      float sum = 0.0f;
#pragma unroll 8
      for (uint32_t j = 0; j < count; ++j)  // (another frame's anchor adds +0: the reads do not wait for the sum)
        sum = sum + ((words[8 * j + 7] & ~kAnchorLiveBit) == f ? __uint_as_float(words[8 * j + src]) : 0.0f);
      record[c] = __float_as_uint(sum);
    } else {
      uint32_t live = 0;
#pragma unroll 8
      for (uint32_t j = 0; j < count; ++j) live += words[8 * j + 7] == (f | kAnchorLiveBit);
      record[6] = live;
    }
  }
}

}  // namespace

void launch_anchor_evaluate(hipStream_t st, const AnchorPass& P) {
  if (!P.base.nd.n || !P.nNodes || !P.base.nProps || P.base.nProps > PIES_ANCHOR_FRAME_MAX || !P.frames || !P.records) return;
  hipLaunchKernelGGL(k_anchor_evaluate, dim3(anchor_tiles(P.nNodes)), dim3(kPropTile), 0, st, P);
}

void launch_anchor_sums(hipStream_t st, const AnchorPass& P) {
  if (!P.nAnchors || !P.impulse || !P.torque || !P.base.tileMask || !P.base.tileSums) return;
  hipLaunchKernelGGL(k_anchor_sums, dim3(anchor_tiles(P.nAnchors)), dim3(kPropTile), 0, st, P.impulse, P.torque, P.nAnchors,
                     P.base.nProps, P.base.tileMask, P.base.tileSums);
}

}  // namespace pies
