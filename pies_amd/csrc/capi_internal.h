// Internals shared by the translation units behind the C ABI (capi.cpp: handle lifetime, pies_finalize, tick, state access;
// device_scene.cpp: the steps of pies_finalize that build the scene in HBM, free_device, node upload and read-back;
// substep_graph.cpp: the substep as a launch sequence, graph capture, the adaptations that follow the scene; profiling.cpp: the
// timing passes; tuning.cpp: the registry of pies_set_tuning).
#pragma once
#include <cmath>
#include <vector>

#include "device_util.h"

namespace pies {

// argument checks: every one of n floats is finite
inline bool finite_all(const float* v, size_t n) {
  for (size_t k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

// ---- substep_graph.cpp ----
bool under_profiler();              // PIES_PROFILER_SAFE=1
void destroy_graph(pies_solver* s);
void collision_grid_bound(const pies_solver* s, uint64_t& entries, bool& fast);
void enqueue_pbd_substep(pies_solver* s, int only, uint32_t* counts, uint64_t* units = nullptr);
bool pd_single_cg(const pies_solver* s);
void enqueue_pd_substep(pies_solver* s, int only = -1, uint32_t* counts = nullptr, uint64_t* units = nullptr);
void enqueue_substep(pies_solver* s, uint32_t* counts);
int select_pd_graph(pies_solver* s);
int capture_graph(pies_solver* s);
uint32_t pcg_ran_short(pies_solver* s, uint32_t budget);  // a solve ran out of iterations: the budget to go on with, no shrinking for 24 synchronisations
uint32_t sort_passes_for(uint32_t keyBits);
int poll_failure(pies_solver* s);
int after_synchronize(pies_solver* s);  // poll_failure, then the adaptations that follow the scene
// ---- device_scene.cpp ----
bool tet_volume_pairs(const pies_solver* s);
void free_device(pies_solver* s);  // the captured graph, the skins' records, every allocation of s->dev; s->dev starts over
int upload_nodes(pies_solver* s);
int download_nodes(pies_solver* s, uint32_t mask = 7u);
int download_rest(pies_solver* s);     // host mirror <- HBM: the rest lengths and angles a pies_drive_actuators left stale
int scene_sync_host(pies_solver* s);  // brings the host mirror up to date before a scene edit
int build_plans(pies_solver* s, int sched);
// the steps of pies_finalize, in its order; each returns a PIES_* code
int alloc_nodes(pies_solver* s);          // node arrays, the read-back stage, the node state, the inverse numbering
int upload_constraints(pies_solver* s);   // position, distance, strain and bend records in plan order
int upload_node_pairs(pies_solver* s);    // the node-pair extension: ids, bitmap, node list
int upload_layer_tables(pies_solver* s);  // schedule LAYERED
// schedule LAYERED: decides the tetrahedral rest dictionary (s->layer.restSets) for a device whose workgroups have maxLds bytes of LDS
void layer_rest_dictionary(pies_solver* s, size_t maxLds, std::vector<uint16_t>* index, std::vector<float4>* table);
int upload_wave_index(pies_solver* s);    // schedule EXACT
int alloc_node_grid(pies_solver* s, bool collide);  // ... and, with `collide`, the pair-order lists
int nc_build(pies_solver* s);             // PIES_FLAG_PD_NODE_CONTACTS
int pd_rest_dictionary(pies_solver* s);   // PD: volume records and the rest dictionary (before pd_build)
int alloc_pd_snapshots(pies_solver* s);   // PD: the retry snapshots (after pd_build)
void pcg_ceiling_rule(pies_solver* s);

// ---- node_io.cpp : the stream rule of the device-pointer entry points (pies_write_nodes_device states it) ----
// `bytes` at p are device memory of the handle's device (p == nullptr: nothing to check)
int check_device_range(pies_solver* s, const char* call, const void* p, size_t bytes);
// The caller's stream must not be capturing (PIES_ERR_STATE); then the solver's stream waits for what the caller has queued so far.
int io_begin(pies_solver* s, const char* call, hipStream_t caller);
// ... and the caller's stream waits for the call's launches; PIES_IO_HOST_SYNC: the host too
int io_end(pies_solver* s, hipStream_t caller, uint32_t flags);

}  // namespace pies

// brings HBM and the captured graph up to date with the host-side scene (capi.cpp; C linkage like its callers, not part of the ABI)
extern "C" int pies_internal_ensure_ready(pies_solver* s);
