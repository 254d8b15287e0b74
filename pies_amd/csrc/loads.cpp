// pies_apply_surface_loads (an extension, pies_hip.h): a constant pressure, the pressure of an enclosed gas, hydrostatic pressure
// and fluid drag on ranges of the scene's triangles change the velocities where HBM holds them and hand back the reaction, the
// enclosed volume and the area per load.  Host side only: argument checks, the buffers (RayBuffers, solver_state.h), the tiles the
// ranges meet, the choice of the variant and the launches (load_kernels.h) between the open and close steps of a prop pass
// (props.cpp).  Volume, gas pressure and the edit are chained on the stream: the only synchronisation is the close step's.  The
// edit goes to dev.nd.vel outside the captured substep: no graph, no schedule and no launch count changes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>

#include "capi_internal.h"
#include "load_kernels.h"

using namespace pies;

namespace {

bool finite_all(const float* v, int n) {
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

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
  if (n_loads && !loads) return fail(s, PIES_ERR_INVALID, "pies_apply_surface_loads: loads is NULL");
  if (n_loads > PIES_LOAD_MAX) return fail(s, PIES_ERR_UNSUPPORTED, "pies_apply_surface_loads: more than PIES_LOAD_MAX (64) loads");
  const uint32_t nTris = static_cast<uint32_t>(s->h_triangles.size() / 3);
  for (uint32_t k = 0; k < n_loads; ++k)
    if (const char* what = load_fault(loads[k], nTris))
      return fail(s, PIES_ERR_INVALID, "pies_apply_surface_loads: load " + std::to_string(k) + ": " + what);
  if (!(dt >= 0.0f) || !std::isfinite(dt)) return fail(s, PIES_ERR_INVALID, "pies_apply_surface_loads: dt must be finite and >= 0");
  if (n_loads == 0) return PIES_OK;
  if (s->device == PIES_DEVICE_NONE)
    return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): surface loads meet the nodes on the device");
  if (int rc = pies_internal_ensure_ready(s)) return rc;
  const uint32_t n = s->dev.nd.n;
  const bool reaction = out_impulse || out_torque || out_nodes;
  if (n == 0 || nTris == 0) {  // nothing to load: the call still waits for the queued work
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    if (out_impulse) std::fill(out_impulse, out_impulse + 3ull * n_loads, 0.0f);
    if (out_torque) std::fill(out_torque, out_torque + 3ull * n_loads, 0.0f);
    if (out_nodes) std::fill(out_nodes, out_nodes + n_loads, 0u);
    if (out_volume) std::fill(out_volume, out_volume + n_loads, 0.0f);
    if (out_area) std::fill(out_area, out_area + n_loads, 0.0f);
    return PIES_OK;
  }

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
  if (const char* e = tuning_env("PIES_LOAD_VARIANT")) {
    if (std::strcmp(e, "scratch") == 0) scratch = true;
    else if (std::strcmp(e, "inplace") != 0)
      return fail(s, PIES_ERR_INVALID, "pies_apply_surface_loads: PIES_LOAD_VARIANT must be inplace or scratch");
  }

  LoadPass P;
  if (int rc = prop_open_pass(s, n_loads, reaction, false, &P.base)) return rc;
  if (!B.loadRecords) {
    if (int rc = ray_grow(s, PIES_LOAD_MAX, &B.loadRecords)) return rc;
    if (int rc = ray_grow_bytes(s, PIES_LOAD_MAX * sizeof(LoadState), &B.loadState)) return rc;
  }
  if (B.loadTileCap < tiles.size()) {
    B.loadTileCap = 0;
    if (int rc = ray_grow(s, tiles.size(), &B.loadTiles)) return rc;
    B.loadTileCap = tiles.size();
  }
  const size_t sums = tiles.size() * n_loads;
  if (B.loadSumCap < sums) {
    B.loadSumCap = 0;
    if (int rc = ray_grow(s, sums, &B.loadTileSums)) return rc;
    B.loadSumCap = sums;
  }
  if (scratch && B.forceVelCap < n) {  // (the forces' scratch array: one call runs at a time)
    B.forceVelCap = 0;
    if (int rc = ray_grow(s, n, &B.forceVel)) return rc;
    if (int rc = ray_grow(s, static_cast<size_t>(prop_tiles(n)) * kForceWaves, &B.forceAffected)) return rc;
    B.forceVelCap = n;
  }
  RayTarget T;
  if (int rc = ray_open_target(s, PIES_RAY_SCENE_TRIANGLES, 0, &T)) return rc;
  if (int rc = ray_build_incidence(s)) return rc;
  P.tri = T.tri;
  P.nTris = T.nTris;
  P.incPtr = B.incPtr;
  P.inc = B.inc;
  HIP_TRY(s, hipMemcpyAsync(B.loadRecords, records, n_loads * sizeof(pies_surface_load_t), hipMemcpyHostToDevice, s->stream));
  if (!tiles.empty())
    HIP_TRY(s, hipMemcpyAsync(B.loadTiles, tiles.data(), tiles.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  P.loads = B.loadRecords;
  P.dt = dt;
  P.tiles = B.loadTiles;
  P.nSlots = static_cast<uint32_t>(tiles.size());
  P.tileSums = B.loadTileSums;
  P.state = static_cast<LoadState*>(B.loadState);
  if (scratch) {
    P.newVel = B.forceVel;
    P.affected = B.forceAffected;
  }
  launch_load_measure(s->stream, P);
  launch_load_fold(s->stream, P);
  launch_load_evaluate(s->stream, P);
  launch_load_commit(s->stream, P);
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
