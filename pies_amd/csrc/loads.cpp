// pies_apply_surface_loads (an extension, pies_hip.h): a constant pressure, the pressure of an enclosed gas, hydrostatic pressure
// and fluid drag on ranges of the scene's triangles change the velocities where HBM holds them and hand back the reaction, the
// enclosed volume and the area per load.  Host side only: argument checks, the buffers (RayBuffers, solver_state.h), the tiles the
// ranges meet, the choice of the variant and the launches (load_kernels.h) between the open and close steps of a prop pass
// (props.cpp).  Volume, gas pressure and the edit are chained on the stream: the only synchronisation is the close step's.  The
// edit goes to dev.nd.vel outside the captured substep: no graph, no schedule and no launch count changes.
#include <algorithm>
#include <cmath>
#include <utility>

#include "capi_internal.h"
#include "load_kernels.h"

using namespace pies;

namespace {

// nullptr, or what is wrong with the record in a container of nTris triangles
const char* load_fault(const pies_surface_load_t& L, uint32_t nTris) {
  if (L.type != PIES_LOAD_PRESSURE && L.type != PIES_LOAD_GAS && L.type != PIES_LOAD_FLUID) return "unknown type";
  if (L.flags & ~static_cast<uint32_t>(PIES_LOAD_INWARD)) return "unknown flag";
  if (L.first > nTris || (L.count != UINT32_MAX && L.count > nTris - L.first)) return "the range leaves the container";
  if (!std::isfinite(L.strength) || !std::isfinite(L.rest_volume) || !std::isfinite(L.drag) || !finite_all(L.point, 3) ||
      !finite_all(L.up, 3) || !finite_all(L.velocity, 3))
    return "every member must be finite";
  if (L.type == PIES_LOAD_GAS && !(L.rest_volume > 0.0f)) return "a gas needs rest_volume > 0";
  if (!(L.drag >= 0.0f)) return "drag must be >= 0";
  return nullptr;
}

}  // namespace

extern "C" {

int pies_apply_surface_loads(pies_solver_t* s, uint32_t n_loads, const pies_surface_load_t* loads, float dt, float* out_impulse,
                             float* out_torque, uint32_t* out_nodes, float* out_volume, float* out_area) {
  if (!s) return PIES_ERR_INVALID;
  const uint32_t nTris = static_cast<uint32_t>(s->h_triangles.size() / 3);
  if (int rc = edit_prelude(s, {"pies_apply_surface_loads", "load", "surface loads", PIES_LOAD_MAX, "PIES_LOAD_MAX"}, n_loads, loads,
                            [&](uint32_t k) { return load_fault(loads[k], nTris); }, &dt, nTris == 0,
                            {out_impulse, out_torque, out_nodes, nullptr, out_volume, out_area});
      rc != kEditGo)
    return rc;
  const bool reaction = out_impulse || out_torque || out_nodes;

  // ---- the records with their ranges resolved, the variant and the tiles of 256 triangles the ranges meet ----
  pies_surface_load_t records[PIES_LOAD_MAX];  // (alive until the close step has synchronised)
  bool drag = false;
  RayBuffers& B = s->ray;
  std::vector<uint32_t>& tiles = B.loadTilesHost;
  tiles.clear();
  std::pair<uint32_t, uint32_t> spans[PIES_LOAD_MAX];  // first and last tile of every range that is not empty
  uint32_t nSpans = 0;
  for (uint32_t k = 0; k < n_loads; ++k) {
    pies_surface_load_t& L = records[k];
    L = loads[k];
    if (L.count == UINT32_MAX) L.count = nTris - L.first;
    drag = drag || (L.type == PIES_LOAD_FLUID && L.drag != 0.0f);
    if (L.count) spans[nSpans++] = {L.first / kLoadTile, (L.first + (L.count - 1)) / kLoadTile};
  }
  std::sort(spans, spans + nSpans);
  for (uint32_t i = 0, next = 0; i < nSpans; ++i)  // the union of the spans, ascending
    for (uint32_t u = std::max(spans[i].first, next); u <= spans[i].second; ++u, next = u) tiles.push_back(u);
  bool scratch = drag;  // a drag reads its neighbours' velocities, so its list goes through the scratch array
  if (int rc = edit_variant(s, "PIES_LOAD_VARIANT", "pies_apply_surface_loads", &scratch)) return rc;

  LoadPass P;
  if (int rc = prop_open_pass(s, n_loads, reaction, false, &P.base)) return rc;
  if (!B.loadRecords) {
    if (int rc = ray_grow(s, PIES_LOAD_MAX, &B.loadRecords)) return rc;
    if (int rc = ray_grow_bytes(s, PIES_LOAD_MAX * sizeof(LoadState), &B.loadState)) return rc;
  }
  if (int rc = ray_reserve(s, tiles.size(), &B.loadTiles, &B.loadTileCap)) return rc;
  if (int rc = ray_reserve(s, tiles.size() * n_loads, &B.loadTileSums, &B.loadSumCap)) return rc;
  if (scratch)
    if (int rc = edit_velocity_scratch(s, &P.scratch)) return rc;
  RayTarget T;
  if (int rc = ray_open_target(s, PIES_RAY_SCENE_TRIANGLES, 0, &T)) return rc;
  if (int rc = ray_build_incidence(s)) return rc;
  P.surface = SurfaceIncidence{T.tri, T.nTris, B.incPtr, B.inc};
  HIP_TRY(s, hipMemcpyAsync(B.loadRecords, records, n_loads * sizeof(pies_surface_load_t), hipMemcpyHostToDevice, s->stream));
  if (!tiles.empty())
    HIP_TRY(s, hipMemcpyAsync(B.loadTiles, tiles.data(), tiles.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  P.loads = B.loadRecords;
  P.dt = dt;
  P.tiles = B.loadTiles;
  P.nSlots = static_cast<uint32_t>(tiles.size());
  P.tileSums = B.loadTileSums;
  P.state = static_cast<LoadState*>(B.loadState);
  launch_load_measure(s->stream, P);
  launch_load_fold(s->stream, P);
  launch_load_evaluate(s->stream, P);
  launch_velocity_commit(s->stream, P.base.nd, P.base.inv, P.scratch);
  LoadState state[PIES_LOAD_MAX];
  if (out_volume || out_area)
    HIP_TRY(s, hipMemcpyAsync(state, P.state, n_loads * sizeof(LoadState), hipMemcpyDeviceToHost, s->stream));
  if (int rc = prop_close_pass(s, P.base, out_impulse, out_torque, out_nodes, nullptr, 4u)) return rc;  // (the velocities alone are stale)
  for (uint32_t k = 0; k < n_loads; ++k) {
    if (out_volume) out_volume[k] = state[k].volume;
    if (out_area) out_area[k] = state[k].area;
  }
  return PIES_OK;
}

}  // extern "C"
