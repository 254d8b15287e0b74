// Ties (extensions, pies_hip.h): pies_add_ties, pies_get_ties, pies_apply_ties, pies_get_tie_state and pies_reset_ties.  Host side
// only: argument checks, the host copy of every set (pies_solver::h_ties) - the records with the set's counts and the CSR from tied
// node to its entries -, the device copies and the call's buffers (RayBuffers, solver_state.h) and the launches (tie_kernels.h).
// The call goes through edit_prelude and the node half of prop_open_pass like the anchors (anchors.cpp) and closes by itself: two
// launches per iteration, then the anchors' sums over tiles of tie indices.  The edit goes to dev.nd.vel
// outside the captured substep: no graph, no schedule and no launch count changes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "capi_internal.h"
#include "tie_kernels.h"

using namespace pies;

namespace {

constexpr uint32_t kTieMax = 1u << 24;        // ties per set
constexpr uint32_t kTieIterationsMax = 64;

bool finite_nonnegative(float v) { return v >= 0.0f && std::isfinite(v); }

// nullptr, or what is wrong with the record
const char* tie_fault(const pies_solver* s, const pies_tie_t& t, uint32_t nGroups) {
  const uint32_t n = s->nodeCount();
  if (t.node >= n || t.to[0] >= n || t.to[1] >= n || t.to[2] >= n) return "node id out of range";
  if (!finite_all(t.weight, 3)) return "weights must be finite";
  if (t.weight[0] == 0.0f && t.weight[1] == 0.0f && t.weight[2] == 0.0f) return "all three weights are 0";
  if (!finite_nonnegative(t.stiffness) || !finite_nonnegative(t.damping)) return "stiffness and damping must be finite and >= 0";
  if (t.group >= nGroups) return "group must be below n_groups";
  for (int j = 0; j < 3; ++j) {
    if (t.weight[j] == 0.0f) continue;
    if (t.to[j] == t.node) return "node and the carrier's nodes must be pairwise distinct";
    for (int l = 0; l < j; ++l)
      if (t.weight[l] != 0.0f && t.to[l] == t.to[j]) return "node and the carrier's nodes must be pairwise distinct";
  }
  return nullptr;
}

const char* group_fault(const pies_tie_group_t& g) {
  if (!finite_all(g.pivot, 3)) return "pivot must be finite";
  if (!finite_nonnegative(g.strength)) return "strength must be finite and >= 0";
  if (!finite_nonnegative(g.break_stretch)) return "break_stretch must be finite and >= 0";
  return nullptr;
}

template <class T> int stage(pies_solver* s, const std::vector<T>& h, T** d) {
  if (int rc = ray_grow(s, h.size(), d)) return rc;
  if (!h.empty()) HIP_TRY(s, hipMemcpyAsync(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s->stream));
  return PIES_OK;
}

// The device copy of set `id`, staged from the host copy when the handle holds none (the first use, or after free_device); the
// broken bytes again after pies_reset_ties.
int stage_set(pies_solver* s, uint32_t id, TieSetDevice* out) {
  TieSetDevice& D = s->ray.tieSets[id];
  HostTieSet& H = s->h_ties[id];  // (outlives the call)
  if (!D.records) {
    TieRecord* records = nullptr;
    if (int rc = stage(s, H.nodes, &D.nodes)) return rc;
    if (int rc = stage(s, H.offsets, &D.offsets)) return rc;
    if (int rc = stage(s, H.entries, &D.entries)) return rc;
    if (int rc = stage(s, H.broken, &D.broken)) return rc;
    if (int rc = stage(s, H.records, &records)) return rc;
    D.records = records;  // (last: a failure above leaves the set unstaged)
  } else if (H.brokenChanged) {
    HIP_TRY(s, hipMemcpyAsync(D.broken, H.broken.data(), H.broken.size(), hipMemcpyHostToDevice, s->stream));
  }
  H.brokenChanged = false;
  *out = D;
  return PIES_OK;
}

}  // namespace

extern "C" {

int pies_add_ties(pies_solver_t* s, uint32_t n, const pies_tie_t* ties, uint32_t n_groups, uint32_t* set) {
  if (!s) return PIES_ERR_INVALID;
  const std::string who = "pies_add_ties: ";
  if (!ties || n == 0) return fail(s, PIES_ERR_INVALID, who + "ties is NULL or n is 0");
  if (n > kTieMax) return fail(s, PIES_ERR_UNSUPPORTED, who + "more than 2^24 ties");
  if (s->h_ties.size() >= PIES_TIE_SET_MAX) return fail(s, PIES_ERR_UNSUPPORTED, who + "more than PIES_TIE_SET_MAX (64) sets");
  if (n_groups == 0 || n_groups > PIES_TIE_GROUP_MAX)
    return fail(s, PIES_ERR_INVALID, who + "n_groups must be 1 .. PIES_TIE_GROUP_MAX (64)");
  for (uint32_t i = 0; i < n; ++i)
    if (const char* what = tie_fault(s, ties[i], n_groups)) return fail(s, PIES_ERR_INVALID, who + "tie " + std::to_string(i) + ": " + what);

  HostTieSet H;
  H.ties.assign(ties, ties + n);
  H.nGroups = n_groups;
  H.broken.assign(n, 0);
  // the counts, and with them the rows' lengths: an entry per (tie, counted slot), in ascending tie index, slot order a 0 1 2
  std::vector<uint32_t> cnt(s->nodeCount(), 0u);
  const auto each_entry = [&](auto&& visit) {
    for (uint32_t i = 0; i < n; ++i) {
      visit(ties[i].node, i, 1.0f);
      for (int j = 0; j < 3; ++j)
        if (ties[i].weight[j] != 0.0f) visit(ties[i].to[j], i, -ties[i].weight[j]);
    }
  };
  each_entry([&](uint32_t node, uint32_t, float) { ++cnt[node]; });
  std::vector<uint32_t> row(cnt.size(), UINT32_MAX);  // node -> its row
  uint32_t total = 0;  // (at most 4 x 2^24 entries)
  for (uint32_t v = 0; v < cnt.size(); ++v)
    if (cnt[v]) {
      row[v] = static_cast<uint32_t>(H.nodes.size());
      H.nodes.push_back(v);
      H.offsets.push_back(total);
      total += cnt[v];
    }
  H.offsets.push_back(total);
  H.entries.resize(total);
  std::vector<uint32_t> next(H.offsets.begin(), H.offsets.end() - 1);
  each_entry([&](uint32_t node, uint32_t i, float c) { H.entries[next[row[node]]++] = TieEntry{i, c}; });
  H.records.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    const pies_tie_t& t = ties[i];
    TieRecord& R = H.records[i];
    R = TieRecord{};
    R.node = t.node;
    R.stiffness = t.stiffness;
    R.damping = t.damping;
    R.group = t.group;
    R.cntNode = static_cast<float>(cnt[t.node]);
    for (int j = 0; j < 3; ++j) {
      R.to[j] = t.to[j];
      R.weight[j] = t.weight[j];
      R.cntTo[j] = static_cast<float>(cnt[t.to[j]]);
    }
  }
  if (set) *set = static_cast<uint32_t>(s->h_ties.size());
  s->h_ties.push_back(std::move(H));
  return PIES_OK;
}

int pies_get_ties(const pies_solver_t* s, uint32_t set, pies_tie_t* ties, uint32_t capacity, uint32_t* n, uint32_t* n_groups) {
  if (!s) return PIES_ERR_INVALID;
  pies_solver* m = const_cast<pies_solver*>(s);  // (the error text is the handle's)
  if (set >= s->h_ties.size()) return fail(m, PIES_ERR_INVALID, "pies_get_ties: unknown set id");
  const HostTieSet& H = s->h_ties[set];
  if (ties && capacity < H.ties.size()) return fail(m, PIES_ERR_INVALID, "pies_get_ties: capacity is below the set's tie count");
  if (ties) std::memcpy(ties, H.ties.data(), H.ties.size() * sizeof(pies_tie_t));
  if (n) *n = static_cast<uint32_t>(H.ties.size());
  if (n_groups) *n_groups = H.nGroups;
  return PIES_OK;
}

int pies_get_tie_state(const pies_solver_t* s, uint32_t set, uint8_t* broken, uint32_t capacity, uint32_t* n_broken) {
  if (!s) return PIES_ERR_INVALID;
  pies_solver* m = const_cast<pies_solver*>(s);
  if (set >= s->h_ties.size()) return fail(m, PIES_ERR_INVALID, "pies_get_tie_state: unknown set id");
  const HostTieSet& H = s->h_ties[set];
  if (broken && capacity < H.broken.size()) return fail(m, PIES_ERR_INVALID, "pies_get_tie_state: capacity is below the set's tie count");
  if (broken) std::memcpy(broken, H.broken.data(), H.broken.size());
  if (n_broken) *n_broken = static_cast<uint32_t>(std::count_if(H.broken.begin(), H.broken.end(), [](uint8_t b) { return b != 0; }));
  return PIES_OK;
}

int pies_reset_ties(pies_solver_t* s, uint32_t set) {
  if (!s) return PIES_ERR_INVALID;
  if (set >= s->h_ties.size()) return fail(s, PIES_ERR_INVALID, "pies_reset_ties: unknown set id");
  HostTieSet& H = s->h_ties[set];
  std::fill(H.broken.begin(), H.broken.end(), uint8_t{0});
  H.brokenChanged = true;  // (the device copy, if there is one, gets the bytes at the next call: every call ends synchronised)
  return PIES_OK;
}

int pies_apply_ties(pies_solver_t* s, uint32_t set, uint32_t n_groups, const pies_tie_group_t* groups, float dt, uint32_t iterations,
                    float* out_impulse, float* out_torque, uint32_t* out_live, float* out_tie) {
  if (!s) return PIES_ERR_INVALID;
  if (set >= s->h_ties.size()) return fail(s, PIES_ERR_INVALID, "pies_apply_ties: unknown set id");
  if (n_groups != s->h_ties[set].nGroups)
    return fail(s, PIES_ERR_INVALID, "pies_apply_ties: n_groups must be the set's (" + std::to_string(s->h_ties[set].nGroups) + ")");
  if (iterations == 0 || iterations > kTieIterationsMax) return fail(s, PIES_ERR_INVALID, "pies_apply_ties: iterations must be 1 .. 64");
  if (int rc = edit_prelude(s, {"pies_apply_ties", "group", "ties", PIES_TIE_GROUP_MAX, "PIES_TIE_GROUP_MAX"}, n_groups, groups,
                            [&](uint32_t k) { return group_fault(groups[k]); }, &dt, false, {out_impulse, out_torque, out_live});
      rc != kEditGo) {
    if (rc == PIES_OK && out_tie)  // (a scene without nodes holds no set; kept for the prelude's contract)
      std::fill(out_tie, out_tie + 4ull * s->h_ties[set].ties.size(), 0.0f);
    return rc;
  }
  HostTieSet& H = s->h_ties[set];  // (pies_internal_ensure_ready leaves the sets alone)
  const uint32_t n = static_cast<uint32_t>(H.ties.size()), tiles = anchor_tiles(n);
  const bool reaction = out_impulse || out_torque || out_live;
  const bool breaks = std::any_of(groups, groups + n_groups, [](const pies_tie_group_t& g) { return g.break_stretch > 0.0f; });
  const bool solve = dt > 0.0f;
  const uint32_t rounds = solve ? iterations : 1u;

  TiePass P;
  if (int rc = prop_open_pass(s, n_groups, false, false, &P.base)) return rc;  // (nd, inv, propOut; the tiles below are of ties)
  RayBuffers& B = s->ray;
  TieSetDevice D;
  if (int rc = stage_set(s, set, &D)) return rc;
  if (!B.tieGroups)
    if (int rc = ray_grow(s, PIES_TIE_GROUP_MAX, &B.tieGroups)) return rc;
  if (B.tieCap < n) {  // (four buffers under one capacity)
    B.tieCap = 0;
    if (int rc = ray_grow(s, n, &B.tieDelta)) return rc;
    if (int rc = ray_grow(s, n, &B.tieImpulse)) return rc;
    if (int rc = ray_grow(s, n, &B.tieTorque)) return rc;
    if (int rc = ray_grow(s, 2 * static_cast<size_t>(n), &B.tieScratch)) return rc;
    B.tieCap = n;
  }
  if (reaction) {
    if (int rc = ray_reserve(s, tiles, &B.propTileMask, &B.propTileCap)) return rc;
    if (int rc = ray_reserve(s, static_cast<size_t>(tiles) * n_groups, &B.propTileSums, &B.propSumCap, kPropSumWords)) return rc;
    P.base.tileMask = B.propTileMask;
    P.base.tileSums = B.propTileSums;
  }
  HIP_TRY(s, hipMemcpyAsync(B.tieGroups, groups, n_groups * sizeof(pies_tie_group_t), hipMemcpyHostToDevice, s->stream));
  P.groups = B.tieGroups;
  P.dt = dt;
  P.nTies = n;
  P.nNodes = static_cast<uint32_t>(H.nodes.size());
  P.records = D.records;
  P.broken = D.broken;
  P.nodes = D.nodes;
  P.offsets = D.offsets;
  P.entries = D.entries;
  P.delta = B.tieDelta;
  P.impulse = B.tieImpulse;
  P.scratch = B.tieScratch;
  P.torque = reaction ? B.tieTorque : nullptr;
  for (uint32_t t = 0; t < rounds; ++t) {
    launch_tie_evaluate(s->stream, P, t == 0, t + 1 == rounds);
    if (solve) launch_tie_scatter(s->stream, P);
  }
  if (reaction) {
    launch_tie_sums(s->stream, P);
    launch_prop_fold_tiles(s->stream, P.base.tileMask, P.base.tileSums, tiles, n_groups, B.propOut);
  }
  HIP_TRY(s, hipGetLastError());
  if (solve) s->stale |= 4u;  // the host mirror's velocities are older than HBM's (nothing is uploaded)
  float folded[PIES_TIE_GROUP_MAX * kPropSumWords];
  if (reaction) HIP_TRY(s, hipMemcpyAsync(folded, B.propOut, n_groups * kPropSumWords * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  if (out_tie) HIP_TRY(s, hipMemcpyAsync(out_tie, B.tieImpulse, n * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
  if (breaks) HIP_TRY(s, hipMemcpyAsync(H.broken.data(), D.broken, n, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  for (uint32_t k = 0; reaction && k < n_groups; ++k) {
    const float* f = folded + k * kPropSumWords;
    if (out_impulse) std::memcpy(out_impulse + 3ull * k, f, 3 * sizeof(float));
    if (out_torque) std::memcpy(out_torque + 3ull * k, f + 3, 3 * sizeof(float));
    if (out_live) std::memcpy(out_live + k, f + 6, sizeof(uint32_t));
  }
  return PIES_OK;
}

}  // extern "C"
