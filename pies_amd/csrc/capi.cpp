// C ABI (include/pies_hip.h): handle lifetime, pies_finalize, tick, state access (the steps that build a scene in HBM and
// free_device: device_scene.cpp; the launch sequence of a substep and its graph capture: substep_graph.cpp; timing passes:
// profiling.cpp; pies_set_tuning: tuning.cpp).
// The substep itself is Solver::tickPBD (Src/Solver.cpp:40-160) / tickPD (:162-486) re-expressed as a
// fixed sequence of kernel launches captured once into a hipGraph: at 100k particles a conflict-free
// batch runs for a few microseconds, so un-graphed launches would be host-bound.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "capi_internal.h"
#include "layer_rest.h"

#include <numeric>

using namespace pies;

extern "C" {

int pies_abi_version(void) { return PIES_ABI_VERSION; }

void pies_default_options(pies_options_t* o) {
  if (!o) return;
  o->fixedTimestepSize = 0.012f;
  o->timeSubsteps = 1;
  o->iterations = 4;
  o->collisionStabilizationIterations = 4;
  o->collisionThresholdDistance = 0.1f;
  o->collisionThickness = 0.05f;
  o->gravity = 10.0f;
  o->damping = 0.006f;
  o->friction = 0.01f;
  o->staticFrictionThreshold = 0.f;
  o->floorHeight = 0.0f;
  o->gridSpacing = 2.0f;
  o->threadCount = 8;
  o->solver = PIES_SOLVER_PD;
}

// PIES_SCHEDULE overrides PIES_SCHEDULE_DEFAULT for new handles (not an explicit pies_set_schedule)
static void apply_schedule_environment(pies_solver* s) {
  if (const char* e = tuning_env("PIES_PCG_OVERFLOW")) s->pcgOverflow = e[0] != '0';
  if (const char* e = tuning_env("PIES_PD_LOCAL_PACKED")) s->pdLocalPacked = e[0] != '0';
  if (const char* e = tuning_env("PIES_PD_CG_SINGLE")) s->pdSingleCg = e[0] != '0';
  if (const char* e = tuning_env("PIES_PD_FUSE_RHS")) s->pdFuseRhs = e[0] != '0';
  if (const char* e = tuning_env("PIES_PD_CG_SINGLE_ROWS")) s->pdSingleCgRows = e[0] != '0';
  if (const char* e = tuning_env("PIES_PCG_BUDGET")) {  // diagnostics: the captured CG iterations, never adapted
    const int v = std::atoi(e);
    if (v >= 1 && v <= 4096) { s->pcgPinned = true; s->pcgPinnedBudget = static_cast<uint32_t>(v); s->pcgBudget = std::min(s->pcgMaxIters, s->pcgPinnedBudget); }
  }
  if (const char* e = std::getenv("PIES_SCHEDULE")) {
    if (!std::strcmp(e, "exact")) s->schedule = PIES_SCHEDULE_EXACT;
    else if (!std::strcmp(e, "coloured")) s->schedule = PIES_SCHEDULE_COLOURED;
    else if (!std::strcmp(e, "layered")) s->schedule = PIES_SCHEDULE_LAYERED;
  }
}

int pies_create(const pies_options_t* options, int device, pies_solver_t** out) {
  if (!out) return PIES_ERR_INVALID;
  *out = nullptr;
  if (device == PIES_DEVICE_NONE) {  // scene/plan inspection only: every call that would compute fails
    pies_solver* s = new pies_solver();
    if (options) s->opt = *options; else pies_default_options(&s->opt);
    if (s->opt.timeSubsteps == 0) s->opt.timeSubsteps = 1;
    s->device = PIES_DEVICE_NONE;
    apply_schedule_environment(s);
    *out = s;
    return PIES_OK;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return PIES_ERR_HIP;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return PIES_ERR_HIP;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return PIES_ERR_HIP;  // kernels are built for gfx950 only
  if (hipSetDevice(device) != hipSuccess) return PIES_ERR_HIP;
  pies_solver* s = new pies_solver();
  if (options) s->opt = *options; else pies_default_options(&s->opt);
  if (s->opt.timeSubsteps == 0) s->opt.timeSubsteps = 1;
  s->device = device;
  apply_schedule_environment(s);
  if (ledger::stream_create(&s->stream, hipStreamNonBlocking) != hipSuccess ||
      ledger::stream_create(&s->sideStream, hipStreamNonBlocking) != hipSuccess ||
      ledger::event_create(&s->evFork, hipEventDisableTiming) != hipSuccess ||
      ledger::event_create(&s->evJoin, hipEventDisableTiming) != hipSuccess) {
    if (s->evFork) (void)ledger::event_destroy(s->evFork);
    if (s->sideStream) (void)ledger::stream_destroy(s->sideStream);
    if (s->stream) (void)ledger::stream_destroy(s->stream);
    delete s;
    return PIES_ERR_HIP;
  }
  *out = s;
  return PIES_OK;
}

int pies_destroy(pies_solver_t* s) {
  if (!s) return PIES_OK;
  if (s->device == PIES_DEVICE_NONE) { delete s; return PIES_OK; }
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  if (s->sideStream) (void)hipStreamSynchronize(s->sideStream);
  if (s->copyStream) (void)hipStreamSynchronize(s->copyStream);
  free_device(s);
  if (s->h_stage) (void)ledger::host_free(s->h_stage);
  if (s->h_skinStage) (void)ledger::host_free(s->h_skinStage);
  if (s->d_skinExport) (void)ledger::dev_free(s->d_skinExport);
  for (int b = 0; b < 2; ++b) {
    if (s->h_skinExport[b]) (void)ledger::host_free(s->h_skinExport[b]);
    if (s->h_export[b]) (void)ledger::host_free(s->h_export[b]);
    if (s->evTick[b]) (void)ledger::event_destroy(s->evTick[b]);
    if (s->evCopied[b]) (void)ledger::event_destroy(s->evCopied[b]);
  }
  if (s->evIoIn) (void)ledger::event_destroy(s->evIoIn);
  if (s->evIoOut) (void)ledger::event_destroy(s->evIoOut);
  if (s->d_export) (void)ledger::dev_free(s->d_export);
  if (s->copyStream) (void)ledger::stream_destroy(s->copyStream);
  if (s->evFork) (void)ledger::event_destroy(s->evFork);
  if (s->evJoin) (void)ledger::event_destroy(s->evJoin);
  if (s->sideStream) (void)ledger::stream_destroy(s->sideStream);
  if (s->stream) (void)ledger::stream_destroy(s->stream);
  delete s;
  return PIES_OK;
}

int pies_clear(pies_solver_t* s) {
  if (!s) return PIES_ERR_INVALID;
  s->h_skins.clear();
  s->skinDirty = false;
  s->h_fields.clear();  // (their device copies go with free_device below)
  s->h_anchors.clear();  // (the same)
  s->h_ties.clear();  // (the same)
  s->h_actuators.clear();  // (the same)
  s->restStale = 0;  // (the constraints whose rest data HBM held newer go too)
  if (s->device != PIES_DEVICE_NONE) {
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    free_device(s);
    // the pinned staging buffers were sized for the scene that goes (the export buffers stay: a frame may be acquired)
    (void)ledger::host_free(s->h_stage);
    s->h_stage = nullptr;
    s->h_stage_n = 0;
    (void)ledger::host_free(s->h_skinStage);
    s->h_skinStage = nullptr;
    s->h_skinStage_n = 0;
  }
  s->h_pos.clear(); s->h_prev.clear(); s->h_vel.clear(); s->h_radius.clear(); s->h_invMass.clear();
  s->h_position.clear(); s->h_distance.clear(); s->h_tet.clear(); s->h_volume.clear(); s->h_bend.clear(); s->h_nodePair.clear();
  s->h_triangles.clear(); s->h_lines.clear();
  s->h_shape.clear(); s->h_goal.clear();  // like the reference, the fixed-region list survives clear() (Solver.cpp:488-507)
  for (Plan& p : s->plan) { p.order.clear(); p.batches.clear(); }
  s->constraintId = 0;
  s->nodeOrder = NodeOrder{};
  s->sceneDirty = true;
  s->stale = 0;
  s->hostNodesDirty = false;
  return PIES_OK;  // like the reference, the failure latch is not reset (Solver.cpp:488-507)
}

const char* pies_last_error(const pies_solver_t* s) { return s ? s->error.c_str() : "null handle"; }

int pies_get_options(const pies_solver_t* s, pies_options_t* out) {
  if (!s || !out) return PIES_ERR_INVALID;
  *out = s->opt;
  return PIES_OK;
}

int pies_set_flag(pies_solver_t* s, int flag, int value) {
  if (!s) return PIES_ERR_INVALID;
  if (flag == PIES_FLAG_REFERENCE_COLLISION_ORDER || flag == PIES_FLAG_COLLISION_ORDER) {
    int v = value;
    if (flag == PIES_FLAG_REFERENCE_COLLISION_ORDER) v = value != 0 ? PIES_COLLISION_ORDER_REFERENCE : PIES_COLLISION_ORDER_PAIRS;
    if (v != PIES_COLLISION_ORDER_REFERENCE && v != PIES_COLLISION_ORDER_GROUPS && v != PIES_COLLISION_ORDER_PAIRS)
      return fail(s, PIES_ERR_INVALID, "pies_set_flag: unknown collision order");
    if (s->collisionOrderFlag != v) {
      s->collisionOrderFlag = v;
      if (!s->sceneDirty) s->graphDirty = true;  // same buffers, another resolve kernel in the captured substep
    }
    return PIES_OK;
  }
  bool* target = flag == PIES_FLAG_RELEASE_HINGE       ? &s->releaseHinge
                 : flag == PIES_FLAG_NODE_COLLISIONS   ? &s->nodeCollisions
                 : flag == PIES_FLAG_TRIANGLE_COLLISIONS ? &s->triangleCollisions
                 : flag == PIES_FLAG_RENUMBER_NODES    ? &s->renumberNodes
                 : flag == PIES_FLAG_PD_NODE_CONTACTS  ? &s->pdNodeContacts
                                                         : nullptr;
  if (!target) return fail(s, PIES_ERR_INVALID, "pies_set_flag: unknown flag");
  if (*target != (value != 0)) {
    *target = value != 0;
    // releaseHinge only drops the position-constraint launches (Solver.cpp:59): with per-container batches (COLOURED,
    // LAYERED, PD) the plans and buffers stay valid and the substep is captured again; schedule EXACT bakes the
    // position constraints into its dependency levels, and the collision flags decide which buffers exist
    const bool captureOnly = flag == PIES_FLAG_RELEASE_HINGE && !s->sceneDirty && (s->opt.solver == PIES_SOLVER_PD || !s->wave.active);
    if (captureOnly) s->graphDirty = true;
    else {
      if (int rc = scene_sync_host(s)) return rc;
      s->sceneDirty = true;
    }
  }
  return PIES_OK;
}

int pies_set_solver(pies_solver_t* s, int solver) {
  if (!s) return PIES_ERR_INVALID;
  if (solver != PIES_SOLVER_PBD && solver != PIES_SOLVER_PD) return fail(s, PIES_ERR_INVALID, "pies_set_solver: unknown solver");
  if (solver != s->opt.solver) {
    if (int rc = scene_sync_host(s)) return rc;
    s->opt.solver = solver;
    s->sceneDirty = true;
  }
  return PIES_OK;
}

int pies_set_schedule(pies_solver_t* s, int schedule) {
  if (!s) return PIES_ERR_INVALID;
  if (schedule != PIES_SCHEDULE_EXACT && schedule != PIES_SCHEDULE_COLOURED && schedule != PIES_SCHEDULE_LAYERED) return fail(s, PIES_ERR_INVALID, "unknown schedule");
  if (schedule != s->schedule) {
    if (int rc = scene_sync_host(s)) return rc;
    s->schedule = schedule;
    s->collisionOrderFlag = -1;  // the node-node order follows the schedule again
    s->sceneDirty = true;
  }
  return PIES_OK;
}

int pies_set_pcg(pies_solver_t* s, float rel_tol, uint32_t max_iters) {
  if (!s || !(rel_tol >= 0.0f) || max_iters == 0 || max_iters > 4096) return fail(s, PIES_ERR_INVALID, "pies_set_pcg: bad argument");
  s->pcgCeilingSet = true;
  if (rel_tol != s->pcgTol || max_iters != s->pcgMaxIters) {
    s->pcgTol = rel_tol;
    s->pcgMaxIters = max_iters;
    s->pcgBudget = std::min(max_iters, s->pcgPinned ? s->pcgPinnedBudget : 32u);
    s->graphDirty = true;  // the captured launch sequence changes, nothing else
  }
  return PIES_OK;
}

int pies_set_pcg_retry(pies_solver_t* s, int enabled) {
  if (!s) return PIES_ERR_INVALID;
  s->pcgRetry = enabled != 0;
  return PIES_OK;
}

// the words of CgArrays::stats (CgStat), zeros where there is no PD system on a device
static int download_pcg_stats(pies_solver* s, float st[kStatWords]) {
  std::fill(st, st + kStatWords, 0.0f);
  if (s->opt.solver != PIES_SOLVER_PD || !s->dev.pd.cg.stats) return PIES_OK;
  HIP_TRY(s, hipSetDevice(s->device));
  HIP_TRY(s, hipMemcpyAsync(st, s->dev.pd.cg.stats, kStatWords * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return PIES_OK;
}

int pies_get_pcg_stats(pies_solver_t* s, float* max_rel_residual, uint32_t* max_iters_used, uint32_t* solves) {
  if (!s) return PIES_ERR_INVALID;
  float st[kStatWords];
  if (int rc = download_pcg_stats(s, st)) return rc;
  if (max_rel_residual) *max_rel_residual = std::sqrt(st[kStatWorst]);
  if (max_iters_used) *max_iters_used = static_cast<uint32_t>(st[kStatIters]);
  if (solves) *solves = static_cast<uint32_t>(st[kStatSolves]);
  return PIES_OK;
}

int pies_get_pcg_health(pies_solver_t* s, uint64_t* short_solves, uint64_t* solves_total, uint32_t* substeps_retried, uint32_t* budget) {
  if (!s) return PIES_ERR_INVALID;
  float st[kStatWords];
  if (int rc = download_pcg_stats(s, st)) return rc;
  // kStatLife: solves left above the tolerance / solves run by the substeps whose result was kept (a substep that pies_tick ran
  // again takes its counts back), since the buffers were built
  uint64_t life[2];
  std::memcpy(life, st + kStatLife, sizeof(life));
  if (short_solves) *short_solves = life[0];
  if (solves_total) *solves_total = life[1];
  if (substeps_retried) *substeps_retried = s->pcgRetries;
  if (budget) *budget = s->pcgBudget;
  return PIES_OK;
}

// The contacts of the last substep as (a, b) pairs of device ids, a < b, in the order the friction pass ran them (ascending pair key
// of the host's ids)
static int nc_download(pies_solver* s, std::vector<uint32_t>* pairs, uint32_t* count) {
  const NodeContactArrays& C = s->dev.nc;
  const bool perm = C.hostId != nullptr && s->nodeOrder.order.size() == C.n;
  auto host = [&](uint32_t i) { return perm ? s->nodeOrder.order[i] : i; };
  std::vector<uint32_t> cnt(C.n);
  HIP_TRY(s, hipSetDevice(s->device));
  HIP_TRY(s, hipMemcpyAsync(cnt.data(), C.cnt, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  uint64_t total = 0;
  for (uint32_t c : cnt) total += c;
  if (count) *count = static_cast<uint32_t>(total / 2);
  if (!pairs) return PIES_OK;
  std::vector<uint32_t> part(static_cast<size_t>(C.n) * C.cap);
  HIP_TRY(s, hipMemcpyAsync(part.data(), C.part, part.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  std::vector<std::pair<uint64_t, uint64_t>> list;
  for (uint32_t i = 0; i < C.n; ++i)
    for (uint32_t k = 0; k < std::min(cnt[i], C.cap); ++k) {
      const uint32_t j = part[static_cast<size_t>(i) * C.cap + k];
      if (i < j) list.push_back({pair_mix(host(i), host(j)), static_cast<uint64_t>(i) << 32 | j});
    }
  std::sort(list.begin(), list.end());
  pairs->resize(2 * list.size());
  for (size_t k = 0; k < list.size(); ++k) {
    (*pairs)[2 * k] = static_cast<uint32_t>(list[k].second >> 32);
    (*pairs)[2 * k + 1] = static_cast<uint32_t>(list[k].second);
  }
  return PIES_OK;
}

int pies_get_node_contacts(pies_solver_t* s, uint32_t* ids, uint32_t capacity, uint32_t* count) {
  if (!s || !count) return PIES_ERR_INVALID;
  *count = 0;
  if (s->device == PIES_DEVICE_NONE || !s->dev.ncActive || s->dev.nd.n == 0) return PIES_OK;
  std::vector<uint32_t> pairs;
  if (int rc = nc_download(s, &pairs, nullptr)) return rc;
  const uint32_t m = static_cast<uint32_t>(pairs.size() / 2);
  *count = m;
  if (ids && m) {
    if (m > capacity) return fail(s, PIES_ERR_INVALID, "pies_get_node_contacts: capacity too small");
    const bool perm = s->nodeOrder.active();  // a renumbered scene: host ids
    for (size_t k = 0; k < pairs.size(); ++k) ids[k] = perm && pairs[k] < s->nodeOrder.order.size() ? s->nodeOrder.order[pairs[k]] : pairs[k];
  }
  return PIES_OK;
}

int pies_finalize(pies_solver_t* s) {
  if (!s) return PIES_ERR_INVALID;
  if (s->device == PIES_DEVICE_NONE) {  // host-only handle: plans can be inspected, nothing is uploaded
    if (s->sceneDirty) {
      decide_node_order(s);
      build_plans(s, s->opt.solver == PIES_SOLVER_PD ? -1 : s->schedule);
      if (s->layer.active && s->opt.solver != PIES_SOLVER_PD) layer_rest_dictionary(s, kLayerLdsBytes, nullptr, nullptr);
    }
    s->sceneDirty = false;
    return PIES_OK;
  }
  HIP_TRY(s, hipSetDevice(s->device));
  if (!s->sceneDirty) return s->hostNodesDirty ? upload_nodes(s) : PIES_OK;
  const bool isPD = s->opt.solver == PIES_SOLVER_PD;
  const bool collide = s->nodeCollisions && !isPD;
  const bool ncOn = isPD && s->pdNodeContacts;  // PIES_FLAG_PD_NODE_CONTACTS: the node grid, for the PD contacts
  // The parallel visiting order of the node-node pass needs ranges of at most 2 cells per axis (true for the reference
  // defaults r = 0.5, spacing 2); other scenes run the pass in the reference's own order (one sequential chain, any range
  // up to the reference's 50 cells per axis).
  s->collideFast = true;
  if (collide) { uint64_t e; collision_grid_bound(s, e, s->collideFast); }
  if (int rc = download_nodes(s)) return rc;
  if (int rc = download_rest(s)) return rc;  // (driven rest lengths and angles survive the rebuild)
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  free_device(s);

  const uint32_t n = s->nodeCount();
  // node numbering (node_order.cpp): from here on the host containers hold the device's numbering, until this returns
  decide_node_order(s);
  InternalNumbering internal(s);
  build_plans(s, isPD ? -1 : s->schedule);  // (PD's local step is order independent: one batch per container, host order)
  // the steps, device_scene.cpp
  if (int rc = alloc_nodes(s)) return rc;
  if (int rc = upload_constraints(s)) return rc;
  if (isPD && !s->h_nodePair.empty())
    if (int rc = upload_node_pairs(s)) return rc;
  if (s->layer.active && !isPD)
    if (int rc = upload_layer_tables(s)) return rc;
  if (s->wave.active && !isPD)
    if (int rc = upload_wave_index(s)) return rc;
  if ((collide || ncOn) && n)
    if (int rc = alloc_node_grid(s, collide)) return rc;
  if (ncOn && n)
    if (int rc = nc_build(s)) return rc;
  if (isPD) {
    if (int rc = pd_rest_dictionary(s)) return rc;
    if (int rc = pd_build(s)) return rc;
    if (int rc = alloc_pd_snapshots(s)) return rc;
  }
  pcg_ceiling_rule(s);
  if (int rc = capture_graph(s)) return rc;
  s->sceneDirty = false;
  s->graphDirty = false;
  if (!s->h_skins.empty())  // the skins' records, in the numbering just decided
    if (int rc = skin_upload(s)) return rc;
  return PIES_OK;
}

// Brings HBM and the captured graph up to date with the host-side scene.
int pies_internal_ensure_ready(pies_solver* s) {
  if (s->sceneDirty || s->hostNodesDirty)
    if (int rc = pies_finalize(s)) return rc;
  HIP_TRY(s, hipSetDevice(s->device));
  if (s->graphDirty) {
    HIP_TRY(s, hipStreamSynchronize(s->stream));  // the old graph may still be running
    if (int rc = capture_graph(s)) return rc;
    s->graphDirty = false;
  }
  if (s->skinDirty)  // a skin was added to a finalized scene: its records only
    if (int rc = skin_upload(s)) return rc;
  return PIES_OK;
}

static int launch_substep(pies_solver* s) {
  if (s->graphExec) {
    HIP_TRY(s, hipGraphLaunch(s->graphExec, s->stream));
  } else {  // PIES_NO_GRAPH=1: eager launches (debug / tracing)
    enqueue_substep(s, nullptr);
    HIP_TRY(s, hipGetLastError());
  }
  return PIES_OK;
}

int pies_tick_async(pies_solver_t* s) {
  if (!s) return PIES_ERR_INVALID;
  if (s->device == PIES_DEVICE_NONE) return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): there is no CPU solver");
  if (s->simFailed) return PIES_OK;  // Solver.cpp:26-28
  if (int rc = pies_internal_ensure_ready(s)) return rc;
  if (s->dev.nd.n == 0) return PIES_OK;
  if (s->opt.solver == PIES_SOLVER_PD) {
    // The captured CG budget can only follow the solves at a host synchronisation.  A caller that queues tick after tick
    // without one gets one here every 16 ticks (the queue drains once, ~50 us of idle device): measured without it, 150
    // queued ticks of a contact scene whose budget had settled at 8 ran short when the contacts re-bound (14 iterations
    // needed), the unconverged positions fed the next tick, and the simulation ended in the failure latch.
    if (s->asyncSinceSync >= 16) {
      if (int rc = pies_synchronize(s)) return rc;
      if (s->simFailed) return PIES_OK;
    }
    ++s->asyncSinceSync;
    if (s->goalDirty)
      if (int rc = pd_upload_goals(s)) return rc;
    if (s->asyncSinceSync == 1) HIP_TRY(s, hipMemsetAsync(s->dev.pd.cg.stats, 0, kStatTickWords * sizeof(float), s->stream));
  } else if (s->nodeCollisions && s->dev.hash.counters) {
    // The node grid's captured radix passes hold the scene's cell box plus five key bits, and the host can only follow a
    // growing box at a synchronisation (adapt_sort_passes): a caller that queues PBD ticks blindly gets one every 16 ticks,
    // like the PD path above, so that a burst that spreads the particles never outruns the captured passes.
    if (s->asyncSinceSync >= 16) {
      if (int rc = pies_synchronize(s)) return rc;
      if (s->simFailed) return PIES_OK;
    }
    ++s->asyncSinceSync;
  }
  for (uint32_t sub = 0; sub < s->opt.timeSubsteps; ++sub)
    if (int rc = launch_substep(s)) return rc;
  if (under_profiler()) HIP_TRY(s, hipStreamSynchronize(s->stream));
  s->stale = 7u;
  return PIES_OK;
}

int pies_synchronize(pies_solver_t* s) {
  if (!s) return PIES_ERR_INVALID;
  if (s->device == PIES_DEVICE_NONE) return PIES_OK;
  HIP_TRY(s, hipSetDevice(s->device));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  s->asyncSinceSync = 0;
  return after_synchronize(s);
}

// Projective Dynamics, synchronous tick: the reference's global step is a direct solve (Solver.cpp:258-262, 356), the
// device's a CG with a captured iteration budget.  A substep in which a solve ends above the tolerance (new contacts
// stiffen the system from one substep to the next) is therefore not kept: the node state is put back and the substep
// runs again with four times the budget, up to the ceiling of pies_set_pcg.
static int pd_tick_checked(pies_solver* s) {
  const uint32_t n = s->dev.nd.n;
  float before[kStatWords], after[kStatWords];
  HIP_TRY(s, hipMemsetAsync(s->dev.pd.cg.stats, 0, kStatTickWords * sizeof(float), s->stream));
  for (uint32_t sub = 0; sub < s->opt.timeSubsteps; ++sub) {
    HIP_TRY(s, hipMemcpyAsync(before, s->dev.pd.cg.stats, sizeof(before), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipMemcpyAsync(s->dev.snapPos, s->dev.nd.pos, n * sizeof(float4), hipMemcpyDeviceToDevice, s->stream));
    HIP_TRY(s, hipMemcpyAsync(s->dev.snapPrev, s->dev.nd.prev, n * sizeof(float4), hipMemcpyDeviceToDevice, s->stream));
    HIP_TRY(s, hipMemcpyAsync(s->dev.snapVel, s->dev.nd.vel, n * sizeof(float4), hipMemcpyDeviceToDevice, s->stream));
    if (s->dev.snapQuat)
      HIP_TRY(s, hipMemcpyAsync(s->dev.snapQuat, s->dev.pd.shape.quat, 4ull * s->dev.pd.shape.count * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    for (;;) {
      if (int rc = launch_substep(s)) return rc;
      HIP_TRY(s, hipMemcpyAsync(after, s->dev.pd.cg.stats, sizeof(after), hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(s, hipStreamSynchronize(s->stream));
      const bool ranShort = after[kStatShort] > before[kStatShort];
      if (!ranShort || s->pcgBudget >= s->pcgMaxIters || s->pcgPinned) {
        if (ranShort) s->pcgShortSolves += static_cast<uint64_t>(after[kStatShort] - before[kStatShort]);
        break;
      }
      // put the substep's input back (the statistics too: the attempt does not count) and capture a larger budget
      HIP_TRY(s, hipMemcpyAsync(s->dev.nd.pos, s->dev.snapPos, n * sizeof(float4), hipMemcpyDeviceToDevice, s->stream));
      HIP_TRY(s, hipMemcpyAsync(s->dev.nd.prev, s->dev.snapPrev, n * sizeof(float4), hipMemcpyDeviceToDevice, s->stream));
      HIP_TRY(s, hipMemcpyAsync(s->dev.nd.vel, s->dev.snapVel, n * sizeof(float4), hipMemcpyDeviceToDevice, s->stream));
      if (s->dev.snapQuat)
        HIP_TRY(s, hipMemcpyAsync(s->dev.pd.shape.quat, s->dev.snapQuat, 4ull * s->dev.pd.shape.count * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
      HIP_TRY(s, hipMemcpyAsync(s->dev.pd.cg.stats, before, sizeof(before), hipMemcpyHostToDevice, s->stream));
      HIP_TRY(s, hipStreamSynchronize(s->stream));
      s->pcgBudget = pcg_ran_short(s, s->pcgBudget);
      ++s->pcgRetries;
      if (const char* e = std::getenv("PIES_PCG_DEBUG"); e && e[0] == '1')
        std::fprintf(stderr, "[pies] pcg: substep ran short (residual^2 %.3g): again with budget %u\n", after[kStatWorst], s->pcgBudget);
      if (int rc = s->pdLadder.empty() ? capture_graph(s) : select_pd_graph(s)) return rc;
    }
  }
  return PIES_OK;
}

int pies_tick(pies_solver_t* s) {
  if (!s) return PIES_ERR_INVALID;
  if (s->simFailed) return PIES_OK;
  if (s->opt.solver == PIES_SOLVER_PD && s->pcgRetry && s->device != PIES_DEVICE_NONE && !under_profiler()) {
    if (int rc = pies_internal_ensure_ready(s)) return rc;
    if (s->dev.nd.n == 0) return PIES_OK;
    if (s->goalDirty)
      if (int rc = pd_upload_goals(s)) return rc;
    if (int rc = pd_tick_checked(s)) return rc;
    s->stale = 7u;
  } else {
    if (int rc = pies_tick_async(s)) return rc;
  }
  const uint32_t n = s->dev.nd.n;
  if (n == 0) return PIES_OK;
  // Solver.cpp:157 : _vertices[i].position = position -- one D2H copy per tick; the host mirror's positions are
  // current afterwards (pies_read_nodes / pies_read_positions_strided copy from it without touching the device)
  if (int rc = download_nodes(s, 1u)) return rc;
  return after_synchronize(s);
}

// ---- render-state export: frame k leaves through a copy stream while frame k+1 computes -----------------------
static int export_prepare(pies_solver* s) {
  const uint32_t n = s->dev.nd.n;
  if (!s->copyStream) {
    HIP_TRY(s, ledger::stream_create(&s->copyStream, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
      HIP_TRY(s, ledger::event_create(&s->evTick[b], hipEventDisableTiming));
      HIP_TRY(s, ledger::event_create(&s->evCopied[b], hipEventDisableTiming));
    }
  }
  if (s->h_export_n < n || !s->d_export) {
    HIP_TRY(s, hipStreamSynchronize(s->copyStream));
    for (int b = 0; b < 2; ++b) {
      if (s->h_export[b]) (void)ledger::host_free(s->h_export[b]);
      s->h_export[b] = nullptr;
      HIP_TRY(s, ledger::host_malloc((void**)&s->h_export[b], std::max<size_t>(n, 1) * sizeof(float4), hipHostMallocDefault));
    }
    if (s->d_export) (void)ledger::dev_free(s->d_export);
    s->d_export = nullptr;
    HIP_TRY(s, ledger::dev_malloc((void**)&s->d_export, std::max<size_t>(n, 1) * sizeof(float4)));
    s->h_export_n = n;
  }
  const size_t nv = s->skin.nVerts;  // skins: positions and normals of every skin, one device buffer and one pinned buffer per frame
  if (nv && (s->skinExport_n < nv || !s->d_skinExport)) {
    HIP_TRY(s, hipStreamSynchronize(s->copyStream));
    for (int b = 0; b < 2; ++b) {
      if (s->h_skinExport[b]) (void)ledger::host_free(s->h_skinExport[b]);
      s->h_skinExport[b] = nullptr;
      s->frameSkinVerts[b] = 0;
    }
    if (s->d_skinExport) (void)ledger::dev_free(s->d_skinExport);
    s->d_skinExport = nullptr;
    s->skinExport_n = 0;
    for (int b = 0; b < 2; ++b) HIP_TRY(s, ledger::host_malloc((void**)&s->h_skinExport[b], 6 * nv * sizeof(float), hipHostMallocDefault));
    HIP_TRY(s, ledger::dev_malloc((void**)&s->d_skinExport, 6 * nv * sizeof(float)));
    s->skinExport_n = nv;
  }
  return PIES_OK;
}

int pies_tick_begin(pies_solver_t* s, uint64_t* frame) {
  if (!s || !frame) return PIES_ERR_INVALID;
  *frame = 0;
  if (s->device == PIES_DEVICE_NONE) return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): there is no CPU solver");
  const uint64_t f = s->frameBegun + 1;
  if (s->frameAcquired && s->frameAcquired + 2 <= f)
    return fail(s, PIES_ERR_STATE, "pies_tick_begin: the frame two ticks back is still acquired (pies_export_release it first)");
  if (int rc = pies_tick_async(s)) return rc;  // a failed simulation still hands out (unchanged) frames
  if (int rc = export_prepare(s)) return rc;
  const uint32_t n = s->dev.nd.n;
  const int b = static_cast<int>(f & 1u);
  if (n) {
    // d_export is free once the previous frame's D2H copy has read it; by now that copy finished long ago
    if (f > 1) HIP_TRY(s, hipStreamWaitEvent(s->stream, s->evCopied[b ^ 1], 0));
    if (s->dev.d_nodeInv) {  // a renumbered scene: the frame in host numbering
      launch_gather_nodes(s->stream, s->dev.nd.pos, s->d_export, s->dev.d_nodeInv, n);
      HIP_TRY(s, hipGetLastError());
    } else {
      HIP_TRY(s, hipMemcpyAsync(s->d_export, s->dev.nd.pos, n * sizeof(float4), hipMemcpyDeviceToDevice, s->stream));
    }
  }
  const uint32_t nv = n ? s->skin.nVerts : 0u;  // skins: evaluated behind the position copy (d_skinExport is free like d_export)
  if (nv) {
    launch_skin_positions(s->stream, s->skin, s->dev.nd.pos, s->d_skinExport, 0, nv);
    launch_skin_normals(s->stream, s->skin, s->d_skinExport, s->d_skinExport + 3ull * nv, 0, nv);
    HIP_TRY(s, hipGetLastError());
  }
  HIP_TRY(s, hipEventRecord(s->evTick[b], s->stream));
  HIP_TRY(s, hipStreamWaitEvent(s->copyStream, s->evTick[b], 0));
  if (n) HIP_TRY(s, hipMemcpyAsync(s->h_export[b], s->d_export, n * sizeof(float4), hipMemcpyDeviceToHost, s->copyStream));
  if (nv) HIP_TRY(s, hipMemcpyAsync(s->h_skinExport[b], s->d_skinExport, 6ull * nv * sizeof(float), hipMemcpyDeviceToHost, s->copyStream));
  s->frameSkinVerts[b] = nv;
  HIP_TRY(s, hipEventRecord(s->evCopied[b], s->copyStream));
  s->frameBegun = f;
  *frame = f;
  return PIES_OK;
}

int pies_export_acquire(pies_solver_t* s, uint64_t frame, const float** pos4, uint32_t* n) {
  if (!s || !pos4) return PIES_ERR_INVALID;
  *pos4 = nullptr;
  if (n) *n = 0;
  if (frame == 0 || frame > s->frameBegun || frame + 2 <= s->frameBegun)
    return fail(s, PIES_ERR_STATE, "pies_export_acquire: only the last two frames begun are held");
  HIP_TRY(s, hipSetDevice(s->device));
  HIP_TRY(s, hipEventSynchronize(s->evCopied[frame & 1u]));
  s->frameAcquired = frame;
  *pos4 = reinterpret_cast<const float*>(s->h_export[frame & 1u]);
  if (n) *n = s->dev.nd.n;
  return PIES_OK;
}

int pies_export_release(pies_solver_t* s, uint64_t frame) {
  if (!s) return PIES_ERR_INVALID;
  if (s->frameAcquired == frame) s->frameAcquired = 0;
  return PIES_OK;
}

int pies_read_positions_strided(pies_solver_t* s, void* dst, uint64_t stride_bytes, uint32_t n) {
  if (!s || (!dst && n) || stride_bytes < 3 * sizeof(float)) return PIES_ERR_INVALID;
  if (n != s->nodeCount()) return fail(s, PIES_ERR_INVALID, "pies_read_positions_strided: n does not match the node count");
  if (s->device != PIES_DEVICE_NONE) {
    HIP_TRY(s, hipSetDevice(s->device));
    if (int rc = download_nodes(s, 1u)) return rc;
  }
  char* out = static_cast<char*>(dst);
  for (uint32_t i = 0; i < n; ++i) std::memcpy(out + static_cast<size_t>(i) * stride_bytes, &s->h_pos[3 * static_cast<size_t>(i)], 3 * sizeof(float));
  return PIES_OK;
}

int pies_failed(pies_solver_t* s, int* failed) {
  if (!s || !failed) return PIES_ERR_INVALID;
  if (int rc = poll_failure(s)) return rc;
  *failed = s->simFailed ? 1 : 0;
  return PIES_OK;
}

int pies_get_tri_grid_stats(pies_solver_t* s, uint32_t out[8]) {
  if (!s || !out) return PIES_ERR_INVALID;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  if (s->device == PIES_DEVICE_NONE || !s->dev.pd.tri.counters) return PIES_OK;
  HIP_TRY(s, hipSetDevice(s->device));
  uint32_t c[kTriCounterWords];
  HIP_TRY(s, hipMemcpyAsync(c, s->dev.pd.tri.counters, sizeof(c), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  uint32_t lists[64 * 16];
  HIP_TRY(s, hipMemcpyAsync(lists, s->dev.pd.tri.workCnt, sizeof(lists), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  for (int i = 0; i < 64; ++i) out[0] += lists[16 * i];
  out[1] = c[kTriCtrHitRecords];
  for (int k = 0; k < 3; ++k) { out[2 + k] = c[kTriCtrLongest + k]; out[5 + k] = c[kTriCtrListed + k]; }
  return PIES_OK;
}

int pies_get_tri_contacts(pies_solver_t* s, uint32_t* ids, uint32_t capacity, uint32_t* count) {
  if (!s || !count) return PIES_ERR_INVALID;
  *count = 0;
  if (s->device == PIES_DEVICE_NONE || !s->dev.pd.tri.counters) return PIES_OK;
  HIP_TRY(s, hipSetDevice(s->device));
  uint32_t m = 0;
  HIP_TRY(s, hipMemcpyAsync(&m, s->dev.pd.tri.counters + kTriCtrContacts, sizeof(m), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  *count = m;
  if (ids && m) {
    if (m > capacity) return fail(s, PIES_ERR_INVALID, "pies_get_tri_contacts: capacity too small");
    HIP_TRY(s, hipMemcpyAsync(ids, s->dev.pd.tri.ids, static_cast<size_t>(m) * sizeof(uint4), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    if (s->dev.d_nodeInv)  // a renumbered scene: the device lists internal ids
      for (size_t k = 0; k < 4ull * m; ++k)
        if (ids[k] < s->nodeOrder.order.size()) ids[k] = s->nodeOrder.order[ids[k]];
  }
  return PIES_OK;
}

int pies_collision_pairs(pies_solver_t* s, uint64_t* pairs) {
  if (!s || !pairs) return PIES_ERR_INVALID;
  *pairs = 0;
  if (!s->dev.hash.counters) return PIES_OK;
  uint32_t v = 0;
  HIP_TRY(s, hipSetDevice(s->device));
  HIP_TRY(s, hipMemcpyAsync(&v, s->dev.hash.counters + kCounterPairs, sizeof(v), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  HIP_TRY(s, hipMemsetAsync(s->dev.hash.counters + kCounterPairs, 0, sizeof(v), s->stream));
  *pairs = v;
  return PIES_OK;
}

int pies_debug_pair_state(pies_solver_t* s, float* slack, float* excursion, uint32_t* degree, uint32_t n) {
  if (!s || !s->dev.pairs.ctl || n != s->dev.pairs.n) return PIES_ERR_INVALID;
  std::vector<float4> node(4ull * n);
  HIP_TRY(s, hipSetDevice(s->device));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  HIP_TRY(s, hipMemcpy(node.data(), s->dev.pairs.node, node.size() * sizeof(float4), hipMemcpyDeviceToHost));
  if (excursion) HIP_TRY(s, hipMemcpy(excursion, s->dev.pairs.exc, n * sizeof(float), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) {
    if (slack) slack[i] = node[4ull * i + 2].w;
    if (degree) std::memcpy(&degree[i], &node[4ull * i + 3].y, sizeof(uint32_t));
  }
  return PIES_OK;
}
int pies_set_collision_rounds(pies_solver_t* s, uint32_t rounds) {
  if (!s) return PIES_ERR_INVALID;
  if (rounds > 4096) return fail(s, PIES_ERR_INVALID, "pies_set_collision_rounds: at most 4096");
  s->pairRoundsPinned = true;  // an explicit count is kept (the library follows the passes by itself otherwise)
  if (rounds != s->pairRounds) {
    s->pairRounds = rounds;
    if (!s->sceneDirty) s->graphDirty = true;
  }
  return PIES_OK;
}

int pies_get_collision_health(pies_solver_t* s, uint32_t* rounds, uint32_t* pairs_listed, uint32_t* passes_repeated, uint32_t* passes_inexact) {
  if (!s) return PIES_ERR_INVALID;
  uint32_t v[kPairWords] = {0};
  if (s->dev.pairs.ctl) {
    HIP_TRY(s, hipSetDevice(s->device));
    HIP_TRY(s, hipMemcpyAsync(v, s->dev.pairs.ctl, sizeof(v), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
  }
  if (rounds) *rounds = v[kPairRounds];
  if (pairs_listed) *pairs_listed = v[kPairEdges] / 2;
  if (passes_repeated) *passes_repeated = v[kPairRetries];
  if (passes_inexact) *passes_inexact = v[kPairInexact];
  return PIES_OK;
}

int pies_get_collision_fallbacks(pies_solver_t* s, uint32_t* passes) {
  if (!s || !passes) return PIES_ERR_INVALID;
  *passes = 0;
  if (s->dev.pairs.ctl) {
    HIP_TRY(s, hipSetDevice(s->device));
    HIP_TRY(s, hipMemcpyAsync(passes, s->dev.pairs.ctl + kPairFallbacks, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
  }
  return PIES_OK;
}

int pies_collision_stats(pies_solver_t* s, uint64_t* pairs, uint64_t* candidates) {
  if (!s) return PIES_ERR_INVALID;
  if (pairs) *pairs = 0;
  if (candidates) *candidates = 0;
  if (!s->dev.hash.counters) return PIES_OK;
  uint32_t v[kHashCounters];
  HIP_TRY(s, hipSetDevice(s->device));
  HIP_TRY(s, hipMemcpyAsync(v, s->dev.hash.counters, sizeof(v), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  HIP_TRY(s, hipMemsetAsync(s->dev.hash.counters + kCounterPairs, 0, sizeof(uint32_t), s->stream));
  HIP_TRY(s, hipMemsetAsync(s->dev.hash.counters + kCounterCandidates, 0, 2 * sizeof(uint32_t), s->stream));
  if (pairs) *pairs = v[kCounterPairs];
  if (candidates) *candidates = static_cast<uint64_t>(v[kCounterCandidates]) | (static_cast<uint64_t>(v[kCounterCandidates + 1]) << 32);
  return PIES_OK;
}

int pies_layer_rest_pack(const uint32_t* ids, uint32_t set, uint32_t* words) {
  if (!ids || !words || set >= 4096u) return PIES_ERR_INVALID;
  for (int k = 0; k < 4; ++k)
    if (ids[k] > kLayerRestIdMask) return PIES_ERR_INVALID;
  layer_rest_pack(ids, set, words);
  return PIES_OK;
}
int pies_layer_rest_unpack(const uint32_t* words, uint32_t* ids, uint32_t* set) {
  if (!words || !ids || !set) return PIES_ERR_INVALID;
  layer_rest_unpack(words, ids, set);
  return PIES_OK;
}
int pies_layer_rest_usable(uint32_t sets, uint32_t count, uint32_t max_group_nodes, uint32_t lds_bytes) {
  if (lds_bytes == 0) lds_bytes = kLayerLdsBytes;
  return layer_rest_usable(sets, count, max_group_nodes, layer_lds_bytes(max_group_nodes, 0), layer_lds_bytes(max_group_nodes, sets), lds_bytes) ? 1 : 0;
}

int pies_resource_counts(uint64_t out[16]) {
  if (!out) return PIES_ERR_INVALID;
  static_assert(2 * ledger::KINDS == 16, "pies_resource_counts: sixteen words");
  ledger::counts(out);
  return PIES_OK;
}

int pies_count(const pies_solver_t* s, int what, uint32_t* out) {
  if (!s || !out) return PIES_ERR_INVALID;
  switch (what) {
    case PIES_POSITION: *out = (uint32_t)s->h_position.size(); break;
    case PIES_DISTANCE: *out = (uint32_t)s->h_distance.size(); break;
    case PIES_TET: *out = (uint32_t)s->h_tet.size(); break;
    case PIES_VOLUME: *out = (uint32_t)s->h_volume.size(); break;
    case PIES_BEND: *out = (uint32_t)s->h_bend.size(); break;
    case PIES_NODE_PAIRS: *out = (uint32_t)s->h_nodePair.size(); break;
    case PIES_SHAPE: *out = (uint32_t)s->h_shape.size(); break;
    case PIES_GOAL: *out = (uint32_t)s->h_goal.size(); break;
    case PIES_TRIANGLES: *out = (uint32_t)(s->h_triangles.size() / 3); break;
    case PIES_LINES: *out = (uint32_t)s->h_lines.size(); break;
    case PIES_NODES: *out = s->nodeCount(); break;
    case PIES_SYSTEM_NNZ: *out = s->pd_nnz; break;
    case PIES_REST_SETS: *out = s->pdLocalPacked && s->dev.d_pairDictIndex ? s->dev.pairDictSets : 0u; break;
    case PIES_ROW_STENCILS: *out = s->dev.pd.cg.rowStencil ? s->dev.pdRowStencils : 0u; break;
    case PIES_PD_TILES: *out = s->dev.pd.tiles.ntiles; break;
    case PIES_PD_TILE_RECORDS: *out = s->dev.pd.tiles.ntiles ? s->pdTileRecords : 0u; break;
    case PIES_PD_CG_SINGLE: *out = s->opt.solver == PIES_SOLVER_PD && pd_single_cg(s) ? 1u : 0u; break;
    case PIES_PD_WINDOW_ENTRIES: *out = s->dev.pd.cg.wRows ? s->pdWindowEntries : 0u; break;
    case PIES_PD_WINDOW_HALO: *out = s->dev.pd.cg.wRows ? s->pdWindowHalo : 0u; break;
    case PIES_NODES_RENUMBERED: *out = s->nodeOrder.active() ? 1u : 0u; break;
    case PIES_LAYER_REST_SETS: *out = s->layer.active ? s->layer.restSets : 0u; break;
    case PIES_PD_CG_BLOCKS: *out = s->opt.solver == PIES_SOLVER_PD && s->dev.pd.cg.n ? s->dev.pd.cg.nparts : 0u; break;
    case PIES_LAYER_MAX_TILES: {
      *out = 0;
      if (s->layer.active)
        for (int ph = 0; ph < 4; ++ph) *out = std::max<uint32_t>(*out, (uint32_t)s->layer.tiles[ph].size());
      break;
    }
    case PIES_LAYER_MAX_CLASS: {
      *out = 0;
      if (s->layer.active)
        for (const LayerKind& K : s->layer.kind) *out = std::max<uint32_t>(*out, K.maxClass);
      break;
    }
    case PIES_SKINS: *out = (uint32_t)s->h_skins.size(); break;
    case PIES_SKIN_VERTICES: {
      *out = 0;
      for (const HostSkin& k : s->h_skins) *out += k.vertexCount();
      break;
    }
    case PIES_NODE_CONTACTS: {
      *out = 0;
      if (s->device != PIES_DEVICE_NONE && s->dev.ncActive && s->dev.nd.n)
        if (int rc = nc_download(const_cast<pies_solver*>(s), nullptr, out)) return rc;
      break;
    }
    default: return PIES_ERR_INVALID;
  }
  return PIES_OK;
}

int pies_read_nodes(pies_solver_t* s, int what, float* out, uint32_t n) {
  if (!s || (!out && n)) return PIES_ERR_INVALID;
  if (n != s->nodeCount()) return fail(s, PIES_ERR_INVALID, "pies_read_nodes: n does not match the node count");
  if (s->device != PIES_DEVICE_NONE && what >= PIES_NODE_POSITION && what <= PIES_NODE_VELOCITY) {
    HIP_TRY(s, hipSetDevice(s->device));
    if (int rc = download_nodes(s, 1u << what)) return rc;  // the requested array only
  }
  const std::vector<float>* src = nullptr;
  switch (what) {
    case PIES_NODE_POSITION: src = &s->h_pos; break;
    case PIES_NODE_PREV_POSITION: src = &s->h_prev; break;
    case PIES_NODE_VELOCITY: src = &s->h_vel; break;
    case PIES_NODE_RADIUS: src = &s->h_radius; break;
    case PIES_NODE_INV_MASS: src = &s->h_invMass; break;
    default: return fail(s, PIES_ERR_INVALID, "pies_read_nodes: unknown selector");
  }
  if (!src->empty()) std::memcpy(out, src->data(), src->size() * sizeof(float));
  return PIES_OK;
}

int pies_write_nodes(pies_solver_t* s, int what, const float* in, uint32_t n) {
  if (!s || (!in && n)) return PIES_ERR_INVALID;
  if (n != s->nodeCount()) return fail(s, PIES_ERR_INVALID, "pies_write_nodes: n does not match the node count");
  if (int rc = scene_sync_host(s)) return rc;
  std::vector<float>* dst = nullptr;
  switch (what) {
    case PIES_NODE_POSITION: dst = &s->h_pos; break;
    case PIES_NODE_PREV_POSITION: dst = &s->h_prev; break;
    case PIES_NODE_VELOCITY: dst = &s->h_vel; break;
    case PIES_NODE_RADIUS: dst = &s->h_radius; break;
    case PIES_NODE_INV_MASS: dst = &s->h_invMass; break;
    default: return fail(s, PIES_ERR_INVALID, "pies_write_nodes: unknown selector");
  }
  // Projective Dynamics: the system matrix K = diag(1 / (invMass h^2)) + sum w A^T A, its preconditioner, the SELL rows and the
  // row dictionary are built from the masses in pies_finalize (pd_build), and k_pd_predict forms M s_n / h^2 from pos.w: new
  // masses in pos.w alone would leave the two sides of the solve with different M.  PBD keeps mass in pos.w only.  (A host
  // that writes back the masses it read - a full state restore every frame - keeps its scene.)
  if (what == PIES_NODE_INV_MASS && s->opt.solver == PIES_SOLVER_PD && !dst->empty() &&
      std::memcmp(dst->data(), in, dst->size() * sizeof(float)) != 0)
    s->sceneDirty = true;
  if (!dst->empty()) std::memcpy(dst->data(), in, dst->size() * sizeof(float));
  s->hostNodesDirty = true;
  if (what == PIES_NODE_RADIUS && s->dev.hash.counters && !s->sceneDirty) {  // the collision grid is sized from the radii
    uint64_t entries;
    bool fast;
    collision_grid_bound(s, entries, fast);
    if (entries + 64 > s->dev.hash.maxEntries || fast != s->collideFast) s->sceneDirty = true;
  }
  return PIES_OK;
}

int pies_get_ids(const pies_solver_t* s, int type, uint32_t* out, uint32_t capacity) {
  if (!s || !out) return PIES_ERR_INVALID;
  size_t k = 0;
  auto put = [&](uint32_t v) { if (k < capacity) out[k] = v; ++k; };
  switch (type) {
    case PIES_POSITION: for (auto& c : s->h_position) put(c.id); break;
    case PIES_DISTANCE: for (auto& c : s->h_distance) { put(c.ids[0]); put(c.ids[1]); } break;
    case PIES_TET: for (auto& c : s->h_tet) for (uint32_t v : c.ids) put(v); break;
    case PIES_VOLUME: for (auto& c : s->h_volume) for (uint32_t v : c.ids) put(v); break;
    case PIES_BEND: for (auto& c : s->h_bend) for (uint32_t v : c.ids) put(v); break;
    case PIES_NODE_PAIRS: for (auto& c : s->h_nodePair) { put(c.ids[0]); put(c.ids[1]); } break;
    case PIES_TRIANGLES: for (uint32_t v : s->h_triangles) put(v); break;
    case PIES_LINES: for (uint32_t v : s->h_lines) put(v); break;
    default: return PIES_ERR_INVALID;
  }
  return k <= capacity ? PIES_OK : PIES_ERR_INVALID;
}

int pies_get_group(const pies_solver_t* s, int type, uint32_t index, uint32_t* ids, uint32_t capacity, uint32_t* count) {
  if (!s || !count || (type != PIES_SHAPE && type != PIES_GOAL)) return PIES_ERR_INVALID;
  const std::vector<uint32_t>* v = nullptr;
  if (type == PIES_SHAPE && index < s->h_shape.size()) v = &s->h_shape[index].ids;
  if (type == PIES_GOAL && index < s->h_goal.size()) v = &s->h_goal[index].ids;
  if (!v) return PIES_ERR_INVALID;
  *count = static_cast<uint32_t>(v->size());
  if (ids) {
    if (v->size() > capacity) return PIES_ERR_INVALID;
    std::copy(v->begin(), v->end(), ids);
  }
  return PIES_OK;
}

int pies_get_rest(const pies_solver_t* s, int type, float* out, uint32_t capacity) {
  if (!s || !out) return PIES_ERR_INVALID;
  if (s->restStale)  // a pies_drive_actuators since the mirror held the truth: the driven values are what the scene has
    if (int rc = download_rest(const_cast<pies_solver*>(s))) return rc;
  size_t k = 0;
  auto put = [&](float v) { if (k < capacity) out[k] = v; ++k; };
  switch (type) {
    case PIES_DISTANCE: for (auto& c : s->h_distance) put(c.target); break;
    case PIES_TET: for (auto& c : s->h_tet) for (float v : c.qinv) put(v); break;
    case PIES_VOLUME: for (auto& c : s->h_volume) for (float v : c.qinv) put(v); break;
    case PIES_BEND: for (auto& c : s->h_bend) put(c.angle); break;
    default: return PIES_ERR_INVALID;
  }
  return k <= capacity ? PIES_OK : PIES_ERR_INVALID;
}

int pies_get_order(pies_solver_t* s, int type, uint32_t* order, uint32_t capacity) {
  if (!s || !order || type < PIES_POSITION || type > PIES_BEND) return PIES_ERR_INVALID;
  if (s->sceneDirty)
    if (int rc = pies_finalize(s)) return rc;
  const Plan& pl = s->plan[type];
  if (pl.order.size() > capacity) return fail(s, PIES_ERR_INVALID, "pies_get_order: capacity too small");
  if (!pl.order.empty()) std::memcpy(order, pl.order.data(), pl.order.size() * sizeof(uint32_t));
  return PIES_OK;
}

int pies_get_batches(pies_solver_t* s, int type, uint32_t* offs, uint32_t capacity, uint32_t* n_batches) {
  if (!s || !n_batches || type < PIES_POSITION || type > PIES_BEND) return PIES_ERR_INVALID;
  if (s->sceneDirty)
    if (int rc = pies_finalize(s)) return rc;
  const Plan& pl = s->plan[type];
  *n_batches = (uint32_t)pl.batches.size();
  if (offs) {
    if (pl.batches.size() + 1 > capacity) return fail(s, PIES_ERR_INVALID, "pies_get_batches: capacity too small");
    for (size_t b = 0; b < pl.batches.size(); ++b) offs[b] = pl.batches[b].start;
    offs[pl.batches.size()] = pl.batches.empty() ? 0 : pl.batches.back().start + pl.batches.back().count;
  }
  return PIES_OK;
}

// The tile plan of the PD strain + volume local step (pd_tiles.cpp), from the host-side scene alone: works on host-only handles.
int pies_get_pd_tile_plan(pies_solver_t* s, uint32_t* n_tiles, uint32_t* info, uint32_t* node, uint32_t* elem, uint32_t* local, uint16_t* nptr,
                          uint16_t* inc, uint32_t tile_capacity) {
  if (!s || !n_tiles) return PIES_ERR_INVALID;
  PdTilePlan plan;
  bool ok = false;
  {
    InternalNumbering internal(s);  // the plan of the numbering the device holds; its node ids are mapped back below
    const bool paired = s->tetVolumePaired;
    s->tetVolumePaired = tet_volume_pairs(s);
    ok = pd_plan_tiles(s, plan);
    s->tetVolumePaired = paired;
    if (ok && s->internalIds)
      for (uint32_t& v : plan.node) v = s->nodeOrder.order[v];
  }
  *n_tiles = ok ? static_cast<uint32_t>(plan.info.size()) : 0u;
  if (!ok || !info) return PIES_OK;
  if (plan.info.size() > tile_capacity) return fail(s, PIES_ERR_INVALID, "pies_get_pd_tile_plan: capacity too small");
  std::memcpy(info, plan.info.data(), plan.info.size() * sizeof(uint32_t));
  if (node) std::memcpy(node, plan.node.data(), plan.node.size() * sizeof(uint32_t));
  if (elem) std::memcpy(elem, plan.elem.data(), plan.elem.size() * sizeof(uint32_t));
  if (local) std::memcpy(local, plan.local.data(), plan.local.size() * sizeof(uint32_t));
  if (nptr) std::memcpy(nptr, plan.nptr.data(), plan.nptr.size() * sizeof(uint16_t));
  if (inc) std::memcpy(inc, plan.inc.data(), plan.inc.size() * sizeof(uint16_t));
  return PIES_OK;
}

int pies_get_node_order(pies_solver_t* s, uint32_t* order, uint32_t capacity) {
  if (!s || !order) return PIES_ERR_INVALID;
  if (s->sceneDirty)
    if (int rc = pies_finalize(s)) return rc;
  const uint32_t n = s->nodeCount();
  if (n > capacity) return fail(s, PIES_ERR_INVALID, "pies_get_node_order: capacity too small");
  if (s->nodeOrder.active() && s->nodeOrder.order.size() == n) std::memcpy(order, s->nodeOrder.order.data(), n * sizeof(uint32_t));
  else std::iota(order, order + n, 0u);
  return PIES_OK;
}

int pies_launch_counts(pies_solver_t* s, uint32_t* out) {
  if (!s || !out) return PIES_ERR_INVALID;
  if (s->sceneDirty)
    if (int rc = pies_finalize(s)) return rc;
  std::memcpy(out, s->launchCounts, sizeof(s->launchCounts));
  return PIES_OK;
}
}  // extern "C"


#ifdef PIES_BOUNDS
// The diagnostic build's record of device-side bounds violations (dev_math.h PIES_IN_BOUNDS), per kernel file: out[2 k] = the first
// failing site, out[2 k + 1] = how many, for k = layer, pd, cg1.  Reading clears.  tests/conftest.py asks after the session.
extern "C" int pies_exp_bounds_layer(unsigned int*);
extern "C" int pies_exp_bounds_pd(unsigned int*);
extern "C" int pies_exp_bounds_cg1(unsigned int*);
extern "C" int pies_exp_bounds_report(unsigned int* out6) {
  return pies_exp_bounds_layer(out6) | pies_exp_bounds_pd(out6 + 2) | pies_exp_bounds_cg1(out6 + 4);
}
#endif
