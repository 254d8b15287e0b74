// Anchors (extensions, pies_hip.h): pies_add_anchors, pies_get_anchors and pies_apply_anchors.  Host side only: argument checks, the
// host copy of every set (pies_solver::h_anchors) sorted by node, the device copies and the call's buffers (RayBuffers,
// solver_state.h) and the launches (anchor_kernels.h).  The call goes through edit_prelude and prop_open_pass like the other edits
// of node state (props.cpp); it closes by itself, because its tiles are tiles of anchor indices and it hands back one entry per
// anchor.  The edit goes to dev.nd outside the captured substep: no graph, no schedule and no launch count
// changes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>

#include "capi_internal.h"
#include "anchor_kernels.h"

using namespace pies;

namespace {

constexpr uint32_t kAnchorMax = 1u << 24;  // anchors per set

// nullptr, or what is wrong with the record
const char* anchor_fault(const pies_solver* s, const pies_anchor_t& a, uint32_t nFrames) {
  if (a.node >= s->nodeCount()) return "node id out of range";
  if (a.frame >= nFrames) return "frame must be below n_frames";
  if (!finite_all(a.local, 3)) return "local must be finite";
  if (!(a.stiffness >= 0.0f) || !std::isfinite(a.stiffness) || !(a.damping >= 0.0f) || !std::isfinite(a.damping))
    return "stiffness and damping must be finite and >= 0";
  if (a.flags & ~static_cast<uint32_t>(PIES_ANCHOR_PIN)) return "unknown flag";
  return nullptr;
}

const char* frame_fault(const pies_anchor_frame_t& f) {
  if (!finite_all(f.origin, 3) || !finite_all(f.axes, 9) || !finite_all(f.velocity, 3) || !finite_all(f.angular, 3) ||
      !finite_all(f.pivot, 3))
    return "origin, axes, velocity, angular and pivot must be finite";
  if (!(f.strength >= 0.0f) || !std::isfinite(f.strength)) return "strength must be finite and >= 0";
  return nullptr;
}

// The device copy of set `id`, staged from the host copy when the handle holds none (the first use, or after free_device).
int stage_set(pies_solver* s, uint32_t id, AnchorSetDevice* out) {
  AnchorSetDevice& D = s->ray.anchorSets[id];
  if (!D.records) {
    const HostAnchorSet& H = s->h_anchors[id];  // (outlives the call)
    if (int rc = ray_grow(s, H.nodes.size(), &D.nodes)) return rc;
    if (int rc = ray_grow(s, H.offsets.size(), &D.offsets)) return rc;
    AnchorRecord* records = nullptr;
    if (int rc = ray_grow(s, H.records.size(), &records)) return rc;
    HIP_TRY(s, hipMemcpyAsync(D.nodes, H.nodes.data(), H.nodes.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(s, hipMemcpyAsync(D.offsets, H.offsets.data(), H.offsets.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(s, hipMemcpyAsync(records, H.records.data(), H.records.size() * sizeof(AnchorRecord), hipMemcpyHostToDevice, s->stream));
    D.records = records;  // (last: a failure above leaves the set unstaged)
  }
  *out = D;
  return PIES_OK;
}

}  // namespace

extern "C" {

int pies_add_anchors(pies_solver_t* s, uint32_t n, const pies_anchor_t* anchors, uint32_t n_frames, uint32_t* set) {
  if (!s) return PIES_ERR_INVALID;
  const std::string who = "pies_add_anchors: ";
  if (!anchors || n == 0) return fail(s, PIES_ERR_INVALID, who + "anchors is NULL or n is 0");
  if (n > kAnchorMax) return fail(s, PIES_ERR_UNSUPPORTED, who + "more than 2^24 anchors");
  if (s->h_anchors.size() >= PIES_ANCHOR_SET_MAX) return fail(s, PIES_ERR_UNSUPPORTED, who + "more than PIES_ANCHOR_SET_MAX (64) sets");
  if (n_frames == 0 || n_frames > PIES_ANCHOR_FRAME_MAX)
    return fail(s, PIES_ERR_INVALID, who + "n_frames must be 1 .. PIES_ANCHOR_FRAME_MAX (64)");
  for (uint32_t i = 0; i < n; ++i)
    if (const char* what = anchor_fault(s, anchors[i], n_frames)) return fail(s, PIES_ERR_INVALID, who + "anchor " + std::to_string(i) + ": " + what);

  HostAnchorSet H;
  H.anchors.assign(anchors, anchors + n);
  H.nFrames = n_frames;
  std::vector<uint32_t> order(n);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return anchors[a].node < anchors[b].node; });  // (node, anchor index)
  H.records.resize(n);
  for (uint32_t r = 0; r < n; ++r) {
    const pies_anchor_t& a = anchors[order[r]];
    if (r == 0 || a.node != anchors[order[r - 1]].node) {
      H.nodes.push_back(a.node);
      H.offsets.push_back(r);
    }
    H.records[r] = AnchorRecord{a.frame, {a.local[0], a.local[1], a.local[2]}, a.stiffness, a.damping, a.flags, order[r]};
    H.pins = H.pins || (a.flags & PIES_ANCHOR_PIN);
  }
  H.offsets.push_back(n);
  for (size_t a = 0; a + 1 < H.offsets.size(); ++a)
    for (uint32_t r = H.offsets[a]; r < H.offsets[a + 1] && H.offsets[a + 1] - H.offsets[a] > 1; ++r)
      if (H.records[r].flags & PIES_ANCHOR_PIN)
        return fail(s, PIES_ERR_INVALID,
                    who + "anchor " + std::to_string(H.records[r].index) + ": node " + std::to_string(H.nodes[a]) +
                        " carries a pin and another anchor of the set");
  if (set) *set = static_cast<uint32_t>(s->h_anchors.size());
  s->h_anchors.push_back(std::move(H));
  return PIES_OK;
}

int pies_get_anchors(const pies_solver_t* s, uint32_t set, pies_anchor_t* anchors, uint32_t capacity, uint32_t* n, uint32_t* n_frames) {
  if (!s) return PIES_ERR_INVALID;
  pies_solver* m = const_cast<pies_solver*>(s);  // (the error text is the handle's)
  if (set >= s->h_anchors.size()) return fail(m, PIES_ERR_INVALID, "pies_get_anchors: unknown set id");
  const HostAnchorSet& H = s->h_anchors[set];
  if (anchors && capacity < H.anchors.size()) return fail(m, PIES_ERR_INVALID, "pies_get_anchors: capacity is below the set's anchor count");
  if (anchors) std::memcpy(anchors, H.anchors.data(), H.anchors.size() * sizeof(pies_anchor_t));
  if (n) *n = static_cast<uint32_t>(H.anchors.size());
  if (n_frames) *n_frames = H.nFrames;
  return PIES_OK;
}

int pies_apply_anchors(pies_solver_t* s, uint32_t set, uint32_t n_frames, const pies_anchor_frame_t* frames, float dt,
                       float* out_impulse, float* out_torque, uint32_t* out_live, float* out_anchor) {
  if (!s) return PIES_ERR_INVALID;
  if (set >= s->h_anchors.size()) return fail(s, PIES_ERR_INVALID, "pies_apply_anchors: unknown set id");
  if (n_frames != s->h_anchors[set].nFrames)
    return fail(s, PIES_ERR_INVALID, "pies_apply_anchors: n_frames must be the set's (" + std::to_string(s->h_anchors[set].nFrames) + ")");
  if (int rc = edit_prelude(s, {"pies_apply_anchors", "frame", "anchors", PIES_ANCHOR_FRAME_MAX, "PIES_ANCHOR_FRAME_MAX"}, n_frames,
                            frames, [&](uint32_t k) { return frame_fault(frames[k]); }, &dt, false, {out_impulse, out_torque, out_live});
      rc != kEditGo) {
    if (rc == PIES_OK && out_anchor)  // (a scene without nodes holds no set; kept for the prelude's contract)
      std::fill(out_anchor, out_anchor + 4ull * s->h_anchors[set].anchors.size(), 0.0f);
    return rc;
  }
  const HostAnchorSet& H = s->h_anchors[set];  // (pies_internal_ensure_ready leaves the sets alone)
  const uint32_t n = static_cast<uint32_t>(H.anchors.size()), tiles = anchor_tiles(n);
  const bool reaction = out_impulse || out_torque || out_live;
  const bool entries = reaction || out_anchor;

  AnchorPass P;
  if (int rc = prop_open_pass(s, n_frames, false, false, &P.base)) return rc;  // (nd, inv, propOut; the tiles below are of anchors)
  RayBuffers& B = s->ray;
  AnchorSetDevice D;
  if (int rc = stage_set(s, set, &D)) return rc;
  if (!B.anchorFrames)
    if (int rc = ray_grow(s, PIES_ANCHOR_FRAME_MAX, &B.anchorFrames)) return rc;
  if (entries && B.anchorOutCap < n) {  // (two buffers under one capacity)
    B.anchorOutCap = 0;
    if (int rc = ray_grow(s, n, &B.anchorImpulse)) return rc;
    if (int rc = ray_grow(s, n, &B.anchorTorque)) return rc;
    B.anchorOutCap = n;
  }
  if (reaction) {
    if (int rc = ray_reserve(s, tiles, &B.propTileMask, &B.propTileCap)) return rc;
    if (int rc = ray_reserve(s, static_cast<size_t>(tiles) * n_frames, &B.propTileSums, &B.propSumCap, kPropSumWords)) return rc;
    P.base.tileMask = B.propTileMask;
    P.base.tileSums = B.propTileSums;
  }
  HIP_TRY(s, hipMemcpyAsync(B.anchorFrames, frames, n_frames * sizeof(pies_anchor_frame_t), hipMemcpyHostToDevice, s->stream));
  P.frames = B.anchorFrames;
  P.dt = dt;
  P.nAnchors = n;
  P.nNodes = static_cast<uint32_t>(H.nodes.size());
  P.nodes = D.nodes;
  P.offsets = D.offsets;
  P.records = D.records;
  P.impulse = entries ? B.anchorImpulse : nullptr;
  P.torque = entries ? B.anchorTorque : nullptr;
  launch_anchor_evaluate(s->stream, P);
  if (reaction) {
    launch_anchor_sums(s->stream, P);
    launch_prop_fold_tiles(s->stream, P.base.tileMask, P.base.tileSums, tiles, n_frames, B.propOut);
  }
  HIP_TRY(s, hipGetLastError());
  s->stale |= H.pins ? 7u : 4u;  // the host mirror is older than HBM: velocities, and what a pin moves (nothing is uploaded)
  float folded[PIES_ANCHOR_FRAME_MAX * kPropSumWords];
  if (reaction) HIP_TRY(s, hipMemcpyAsync(folded, B.propOut, n_frames * kPropSumWords * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  if (out_anchor) HIP_TRY(s, hipMemcpyAsync(out_anchor, B.anchorImpulse, n * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  for (uint32_t k = 0; reaction && k < n_frames; ++k) {
    const float* f = folded + k * kPropSumWords;
    if (out_impulse) std::memcpy(out_impulse + 3ull * k, f, 3 * sizeof(float));
    if (out_torque) std::memcpy(out_torque + 3ull * k, f + 3, 3 * sizeof(float));
    if (out_live) std::memcpy(out_live + k, f + 6, sizeof(uint32_t));
  }
  return PIES_OK;
}

}  // extern "C"
