// The device side of one scene (DeviceScene, solver_state.h): what pies_finalize (capi.cpp) builds in HBM, one function per step in
// the order it calls them, free_device that takes it all down again, and the node state's way across the bus in both directions.
// Host code that runs once per scene: nothing here decides what a substep launches (substep_graph.cpp).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>

#include "capi_internal.h"
#include "layer_rest.h"

namespace pies {

// Distinct sets of N rest constants, compared by bytes (-0.0 and +0.0 are two sets) and numbered in order of first appearance:
// the rest dictionaries of the PD local step and of schedule LAYERED's tetrahedral container.
template <int N>
struct RestSets {
  static_assert(N % 4 == 0, "a set is stored as float4");
  struct Set { float v[N]; bool operator<(const Set& o) const { return std::memcmp(v, o.v, sizeof(v)) < 0; } };
  std::map<Set, uint32_t> ids;
  std::vector<float4> table;  // N / 4 per set
  // the number of `key`'s set, a new one if need be; -1 when that would be set number `cap`
  int find_or_add(const Set& key, size_t cap) {
    auto it = ids.find(key);
    if (it == ids.end()) {
      if (ids.size() >= cap) return -1;
      it = ids.emplace(key, static_cast<uint32_t>(ids.size())).first;
      for (int q = 0; q < N; q += 4) table.push_back(make_float4(key.v[q], key.v[q + 1], key.v[q + 2], key.v[q + 3]));
    }
    return static_cast<int>(it->second);
  }
};

void free_device(pies_solver* s) {
  destroy_graph(s);
  skin_free_device(s);
  ray_free_device(s);
  for (void* p : s->dev.allocations) (void)ledger::dev_free(p);
  s->dev = DeviceScene{};
}

int upload_nodes(pies_solver* s) {
  const uint32_t n = s->nodeCount();
  // a renumbered scene: device index k holds host node order[k] (inside pies_finalize the host arrays are already translated)
  const bool perm = s->nodeOrder.active() && !s->internalIds && s->nodeOrder.order.size() == n;
  std::vector<float4> pos(n), prev(n), vel(n);
  std::vector<float> radius;
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t i = perm ? s->nodeOrder.order[k] : k;
    pos[k] = make_float4(s->h_pos[3 * i], s->h_pos[3 * i + 1], s->h_pos[3 * i + 2], s->h_invMass[i]);
    prev[k] = make_float4(s->h_prev[3 * i], s->h_prev[3 * i + 1], s->h_prev[3 * i + 2], 0.f);
    vel[k] = make_float4(s->h_vel[3 * i], s->h_vel[3 * i + 1], s->h_vel[3 * i + 2], 0.f);
  }
  if (perm) {
    radius.resize(n);
    for (uint32_t k = 0; k < n; ++k) radius[k] = s->h_radius[s->nodeOrder.order[k]];
  }
  if (n) {
    HIP_TRY(s, hipMemcpyAsync(s->dev.nd.pos, pos.data(), n * sizeof(float4), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(s, hipMemcpyAsync(s->dev.nd.prev, prev.data(), n * sizeof(float4), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(s, hipMemcpyAsync(s->dev.nd.vel, vel.data(), n * sizeof(float4), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(s, hipMemcpyAsync(s->dev.nd.radius, perm ? radius.data() : s->h_radius.data(), n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    std::vector<float> lrad;
    if (s->dev.d_layer.lrad && s->layer.nodeList.size() == n) {  // schedule LAYERED keeps the radii in level order as well
      lrad.resize(n);
      for (uint32_t i = 0; i < n; ++i) lrad[i] = s->h_radius[s->layer.nodeList[i]];
      HIP_TRY(s, hipMemcpyAsync(s->dev.d_layer.lrad, lrad.data(), n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    }
    HIP_TRY(s, hipStreamSynchronize(s->stream));  // the staging vectors die with this scope
  }
  s->hostNodesDirty = false;
  s->stale = 0;
  return PIES_OK;
}

// Host mirror <- HBM: the arrays of `mask` (bit 0 positions, 1 previous positions, 2 velocities) that are stale, one
// copy each through the pinned staging buffer.
int download_nodes(pies_solver* s, uint32_t mask) {
  const uint32_t n = s->dev.nd.n;
  mask &= s->stale;
  if (n == 0 || !s->h_stage || !s->dev.d_pack) { s->stale = 0; return PIES_OK; }
  float* dst[3] = {s->h_pos.data(), s->h_prev.data(), s->h_vel.data()};
  const float4* src[3] = {s->dev.nd.pos, s->dev.nd.prev, s->dev.nd.vel};
  for (int a = 0; a < 3; ++a) {
    if (!(mask & (1u << a))) continue;
    // packed on the device: 12 bytes per node cross the bus, and the mirror is one memcpy from the pinned stage (measured on
    // config 2: 654 ticks/s against 637 with four floats per node and an unpacking loop; the asynchronous export stays the
    // fast way out, 680)
    launch_pack_xyz(s->stream, src[a], s->dev.d_pack, n, s->dev.d_nodeInv);  // (a renumbered scene: packed in host numbering)
    HIP_TRY(s, hipMemcpyAsync(s->h_stage, s->dev.d_pack, 3ull * n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    std::memcpy(dst[a], s->h_stage, 3ull * n * sizeof(float));
    s->stale &= ~(1u << a);
  }
  return PIES_OK;
}

// Host mirror <- HBM: the rest lengths and rest angles, when pies_drive_actuators (actuators.cpp) has written them since the mirror
// held the truth.  Slot k of the device's records is constraint plan.order[k] - the plan the records were uploaded by, which
// only pies_finalize replaces, after it has called this.  The rule of the drive is not restated here: the words are copied.
int download_rest(pies_solver* s) {
  if (!s->restStale) return PIES_OK;
  if (s->device == PIES_DEVICE_NONE) { s->restStale = 0; return PIES_OK; }
  HIP_TRY(s, hipSetDevice(s->device));
  std::vector<float2> words;
  for (int k = 0; k < 2; ++k) {
    if (!(s->restStale & (1u << k))) continue;
    const float2* src = k == 0 ? s->dev.d_dc_rw : s->dev.d_bc_aw;
    const std::vector<uint32_t>& order = s->plan[k == 0 ? PIES_DISTANCE : PIES_BEND].order;
    if (src && !order.empty()) {
      words.resize(order.size());
      HIP_TRY(s, hipMemcpyAsync(words.data(), src, words.size() * sizeof(float2), hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(s, hipStreamSynchronize(s->stream));
      for (size_t q = 0; q < order.size(); ++q) {
        if (k == 0 && order[q] < s->h_distance.size()) s->h_distance[order[q]].target = words[q].x;
        if (k == 1 && order[q] < s->h_bend.size()) s->h_bend[order[q]].angle = words[q].x;
      }
    }
    s->restStale &= ~(1u << k);
  }
  return PIES_OK;
}

int scene_sync_host(pies_solver* s) {
  if (s->device == PIES_DEVICE_NONE) return PIES_OK;
  if (hipSetDevice(s->device) != hipSuccess) return fail(s, PIES_ERR_HIP, "hipSetDevice failed");
  if (int rc = download_rest(s)) return rc;
  return download_nodes(s);
}

int build_plans(pies_solver* s, int sched) {
  const uint32_t n = s->nodeCount();
  s->layer = LayerPlan{};
  s->wave = WavePlan{};
  if (sched == PIES_SCHEDULE_LAYERED) {
    if (build_layer_plan(s)) return PIES_OK;
    sched = PIES_SCHEDULE_COLOURED;  // wide bodies (two levels do not fit in LDS), scenes without constraints
  }
  std::vector<uint32_t> ids;
  ids.resize(s->h_position.size());
  for (size_t i = 0; i < ids.size(); ++i) ids[i] = s->h_position[i].id;
  build_plan({ids.data(), 1, (uint32_t)s->h_position.size(), 0x1}, n, sched, s->plan[PIES_POSITION]);
  ids.resize(2 * s->h_distance.size());
  for (size_t i = 0; i < s->h_distance.size(); ++i) { ids[2 * i] = s->h_distance[i].ids[0]; ids[2 * i + 1] = s->h_distance[i].ids[1]; }
  // a distance projection moves node a only (Constraints.cpp:34-36); node b is read
  std::vector<uint16_t> hint(s->h_distance.size());
  for (size_t i = 0; i < hint.size(); ++i) hint[i] = s->h_distance[i].hint;
  build_plan({ids.data(), 2, (uint32_t)s->h_distance.size(), 0x1, hint.data()}, n, sched, s->plan[PIES_DISTANCE]);
  ids.resize(4 * s->h_tet.size());
  for (size_t i = 0; i < s->h_tet.size(); ++i) std::memcpy(&ids[4 * i], s->h_tet[i].ids, 16);
  hint.resize(s->h_tet.size());
  for (size_t i = 0; i < hint.size(); ++i) hint[i] = s->h_tet[i].hint;
  build_plan({ids.data(), 4, (uint32_t)s->h_tet.size(), 0xF, hint.data()}, n, sched, s->plan[PIES_TET]);
  ids.resize(4 * s->h_bend.size());
  for (size_t i = 0; i < s->h_bend.size(); ++i) std::memcpy(&ids[4 * i], s->h_bend[i].ids, 16);
  build_plan({ids.data(), 4, (uint32_t)s->h_bend.size(), 0xF}, n, sched, s->plan[PIES_BEND]);
  const char* noWave = tuning_env("PIES_NO_WAVEFRONT");
  if (sched == PIES_SCHEDULE_EXACT && !(noWave && noWave[0] == '1')) build_wave_plan(s, s->wave);
  return PIES_OK;
}

// ---- the steps of pies_finalize, in the order it runs them (the host containers hold the device's numbering throughout) ----

int alloc_nodes(pies_solver* s) {
  const uint32_t n = s->nodeCount();
  DeviceScene& d = s->dev;
  if (n) {
    if (int rc = dev_alloc(s, n, &d.nd.pos)) return rc;
    if (int rc = dev_alloc(s, n, &d.nd.prev)) return rc;
    if (int rc = dev_alloc(s, n, &d.nd.vel)) return rc;
    if (int rc = dev_alloc(s, n, &d.nd.radius)) return rc;
    if (int rc = dev_alloc(s, 3ull * n, &d.d_pack)) return rc;
    d.nd.n = n;
    if (s->h_stage_n < n) {
      if (s->h_stage) (void)ledger::host_free(s->h_stage);
      s->h_stage = nullptr;
      HIP_TRY(s, ledger::host_malloc((void**)&s->h_stage, n * sizeof(float4), hipHostMallocDefault));
      s->h_stage_n = n;
    }
  }
  if (int rc = upload_nodes(s)) return rc;
  return s->nodeOrder.active() ? upload(s, s->nodeOrder.inv, &d.d_nodeInv) : PIES_OK;
}

// TetrahedralConstraint and VolumeConstraint records share a layout: the ids and the rest data in three float4.
// Slot k holds c[order[k]] (order == nullptr: c[k]).
static int upload_tets(pies_solver* s, const std::vector<HostTet>& c, const uint32_t* order, size_t count, uint4** ids, float4** q0,
                       float4** q1, float4** q2) {
  std::vector<uint4> id(count);
  std::vector<float4> a(count), b(count), e(count);
  for (size_t k = 0; k < count; ++k) {
    const HostTet& t = c[order ? order[k] : k];
    id[k] = make_uint4(t.ids[0], t.ids[1], t.ids[2], t.ids[3]);
    a[k] = make_float4(t.qinv[0], t.qinv[1], t.qinv[2], t.qinv[3]);
    b[k] = make_float4(t.qinv[4], t.qinv[5], t.qinv[6], t.qinv[7]);
    e[k] = make_float4(t.qinv[8], t.lo, t.hi, t.w);
  }
  if (int rc = upload(s, id, ids)) return rc;
  if (int rc = upload(s, a, q0)) return rc;
  if (int rc = upload(s, b, q1)) return rc;
  return upload(s, e, q2);
}

// constraint records, in plan order
int upload_constraints(pies_solver* s) {
  DeviceScene& d = s->dev;
  {
    const Plan& pl = s->plan[PIES_POSITION];
    std::vector<uint32_t> id(pl.order.size());
    std::vector<float4> tw(pl.order.size());
    for (size_t k = 0; k < pl.order.size(); ++k) {
      const HostPosition& c = s->h_position[pl.order[k]];
      id[k] = c.id;
      tw[k] = make_float4(c.target[0], c.target[1], c.target[2], c.w);
    }
    if (int rc = upload(s, id, &d.d_pc_id)) return rc;
    if (int rc = upload(s, tw, &d.d_pc_tw)) return rc;
  }
  {
    const Plan& pl = s->plan[PIES_DISTANCE];
    std::vector<uint2> id(pl.order.size());
    std::vector<float2> rw(pl.order.size());
    for (size_t k = 0; k < pl.order.size(); ++k) {
      const HostDistance& c = s->h_distance[pl.order[k]];
      id[k] = make_uint2(c.ids[0], c.ids[1]);
      rw[k] = make_float2(c.target, c.w);
    }
    if (int rc = upload(s, id, &d.d_dc_ids)) return rc;
    if (int rc = upload(s, rw, &d.d_dc_rw)) return rc;
  }
  const std::vector<uint32_t>& to = s->plan[PIES_TET].order;
  if (int rc = upload_tets(s, s->h_tet, to.data(), to.size(), &d.d_tc_ids, &d.d_tc_q0, &d.d_tc_q1, &d.d_tc_q2)) return rc;
  const Plan& pl = s->plan[PIES_BEND];
  std::vector<uint4> id(pl.order.size());
  std::vector<float2> aw(pl.order.size());
  for (size_t k = 0; k < pl.order.size(); ++k) {
    const HostBend& c = s->h_bend[pl.order[k]];
    id[k] = make_uint4(c.ids[0], c.ids[1], c.ids[2], c.ids[3]);
    aw[k] = make_float2(c.angle, c.w);
  }
  if (int rc = upload(s, id, &d.d_bc_ids)) return rc;
  return upload(s, aw, &d.d_bc_aw);
}

// the node-pair extension (container order: a pair's slot is its index)
int upload_node_pairs(pies_solver* s) {
  std::vector<uint2> id(s->h_nodePair.size());
  for (size_t k = 0; k < id.size(); ++k) id[k] = make_uint2(s->h_nodePair[k].ids[0], s->h_nodePair[k].ids[1]);
  if (int rc = upload(s, id, &s->dev.d_np_ids)) return rc;
  // the pairs' nodes (ids in device numbering here): the velocity kernel leaves their floor friction to
  // launch_pd_node_pair_floor_friction, which runs after the pairs' friction (Solver.cpp:398-428 before :473-484)
  const uint32_t n = s->nodeCount();
  std::vector<uint32_t> bits((n + 31u) / 32u, 0u), nodes;
  for (const uint2& p : id)
    for (uint32_t i : {p.x, p.y})
      if (i < n) bits[i >> 5] |= 1u << (i & 31u);
  for (uint32_t i = 0; i < n; ++i)
    if ((bits[i >> 5] >> (i & 31u)) & 1u) nodes.push_back(i);
  if (int rc = upload(s, bits, &s->dev.d_np_bits)) return rc;
  if (int rc = upload(s, nodes, &s->dev.d_np_nodes)) return rc;
  s->dev.npNodes = (uint32_t)nodes.size();
  return PIES_OK;
}

// schedule LAYERED: the rest dictionary of the tetrahedral container (layer_rest.h).  On a createTetBox lattice the 48 bytes of
// rest constants are the same for every element of one orientation, and k_layer reads them from a table in LDS instead of
// streaming them from HBM colour after colour.  All or nothing per scene: sets L.restSets and fills index (per slot) and table, or
// leaves L.restSets 0 (PIES_LAYER_REST_DICT=0, too many sets, no compression, no room in LDS: the per-element arrays are read).
void layer_rest_dictionary(pies_solver* s, size_t maxLds, std::vector<uint16_t>* index, std::vector<float4>* table) {
  LayerPlan& L = s->layer;
  L.restSets = 0;
  const std::vector<uint32_t>& order = s->plan[PIES_TET].order;
  const size_t count = L.kind[PIES_TET].local.size() / 4;
  const char* de = tuning_env("PIES_LAYER_REST_DICT");
  if (!L.active || count == 0 || order.size() != count || (de && de[0] == '0')) return;
  RestSets<12> sets;
  std::vector<uint16_t> idx(count);
  const size_t cap = std::min<size_t>(kLayerRestMaxSets, count / 16);  // (more sets than that are no real compression)
  for (size_t k = 0; k < count; ++k) {
    const HostTet& a = s->h_tet[order[k]];
    RestSets<12>::Set key;
    std::memcpy(key.v, a.qinv, 9 * sizeof(float));
    key.v[9] = a.lo; key.v[10] = a.hi; key.v[11] = a.w;
    const int set = sets.find_or_add(key, cap);
    if (set < 0) return;
    idx[k] = static_cast<uint16_t>(set);
  }
  const uint32_t n = static_cast<uint32_t>(sets.ids.size());
  if (!layer_rest_usable(n, count, L.maxGroupNodes, layer_lds_bytes(L.maxGroupNodes, 0), layer_lds_bytes(L.maxGroupNodes, n), maxLds)) return;
  L.restSets = n;
  if (index) index->swap(idx);
  if (table) table->swap(sets.table);
}

// schedule LAYERED: the level-ordered node list, the tiles and the tile-local ids of every container
int upload_layer_tables(pies_solver* s) {
  LayerPlan& L = s->layer;
  LayerDevice& d = s->dev.d_layer;
  int maxLds = 0;
  HIP_TRY(s, hipDeviceGetAttribute(&maxLds, hipDeviceAttributeMaxSharedMemoryPerBlock, s->device));
  if (static_cast<size_t>(L.maxGroupNodes) * 20 + 4096 > static_cast<size_t>(maxLds))
    return fail(s, PIES_ERR_UNSUPPORTED, "schedule LAYERED: the device's LDS is smaller than this build assumes");
  std::vector<uint16_t> restIndex;
  std::vector<float4> restTable;
  layer_rest_dictionary(s, static_cast<size_t>(maxLds), &restIndex, &restTable);
  HIP_TRY(s, layer_prepare(L.maxGroupNodes, L.restSets));
  if (L.restSets) {  // the table, then the table once more with every row in the row-pair form's order (layer_rest.h)
    const size_t n = restTable.size();
    restTable.resize(2 * n);
    for (uint32_t k = 0; k < L.restSets; ++k)
      layer_rest_row_permute(reinterpret_cast<const float*>(&restTable[3 * k]), reinterpret_cast<float*>(&restTable[n + 3 * k]));
    if (int rc = upload(s, restTable, &d.restTable)) return rc;
  }
  if (int rc = upload(s, L.nodeList, &d.nodeList)) return rc;
  if (int rc = dev_alloc(s, L.nodeList.size(), &d.lpos, true)) return rc;
  {
    std::vector<float> lrad(L.nodeList.size());
    for (size_t i = 0; i < lrad.size(); ++i) lrad[i] = s->h_radius[L.nodeList[i]];
    if (int rc = upload(s, lrad, &d.lrad)) return rc;
  }
  for (int ph = 0; ph < 4; ++ph)
    if (int rc = upload(s, L.tiles[ph], &d.tiles[ph])) return rc;
  for (int k = 0; k < 5; ++k)
    for (int ph = 0; ph < 4; ++ph)
      if (int rc = upload(s, L.kind[k].colOff[ph], &d.colOff[k][ph])) return rc;
  if (int rc = upload(s, L.kind[PIES_POSITION].local, &d.pc_lid)) return rc;
  {
    const std::vector<uint32_t>& l = L.kind[PIES_DISTANCE].local;
    std::vector<uint32_t> packed(l.size() / 2);
    for (size_t k = 0; k < packed.size(); ++k) packed[k] = l[2 * k] | (l[2 * k + 1] << 16);
    if (int rc = upload(s, packed, &d.dc_lid)) return rc;
  }
  for (int k : {PIES_TET, PIES_BEND}) {
    const std::vector<uint32_t>& l = L.kind[k].local;
    std::vector<uint2> packed(l.size() / 4);
    for (size_t c = 0; c < packed.size(); ++c) packed[c] = make_uint2(l[4 * c] | (l[4 * c + 1] << 16), l[4 * c + 2] | (l[4 * c + 3] << 16));
    if (k == PIES_TET && L.restSets)  // 13-bit ids, the set index in their spare bits
      for (size_t c = 0; c < packed.size(); ++c) {
        uint32_t w[2];
        layer_rest_pack(&l[4 * c], restIndex[c], w);
        packed[c] = make_uint2(w[0], w[1]);
      }
    if (int rc = upload(s, packed, k == PIES_TET ? &d.tc_lid : &d.bc_lid)) return rc;
  }
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return PIES_OK;
}

// schedule EXACT: the items of the whole-substep levels
int upload_wave_index(pies_solver* s) {
  if (int rc = upload(s, s->wave.index, &s->dev.d_waveIndex)) return rc;
  std::vector<uint32_t>().swap(s->wave.index);  // the levels (offsets, counts) stay on the host; the items live in HBM
  return PIES_OK;
}

// pair order: every node's list of partners (in pools), the frontier of the level launches
static int alloc_pair_lists(pies_solver* s) {
  const uint32_t n = s->nodeCount();
  PairArrays& P = s->dev.pairs;
  P.n = n;
  // list entries: 96 per node on average (BASELINE config 4 lists 15-50), in kPairPools pools; a small scene may list every
  // pair (a body that has collapsed into a few cells: quirk Q2 does that to a tetrahedral PBD body within a tick)
  // (only a small scene: the n * n floor used to apply to every scene of 8 192 nodes and more - 270 MB per handle)
  const uint64_t everyPair = n <= 8192u ? static_cast<uint64_t>(n) * n : 0ull;
  P.poolCap = static_cast<uint32_t>(std::min<uint64_t>((std::max<uint64_t>(96ull * n, everyPair) + 65536) / kPairPools + 4096, 0x7fff0000ull / kPairPools));
  if (int rc = dev_alloc(s, 4ull * n, &P.node, true)) return rc;
  if (int rc = dev_alloc(s, n, &P.vel0)) return rc;
  if (int rc = dev_alloc(s, n, &P.exc, true)) return rc;
  if (int rc = dev_alloc(s, n, &P.turnCnt, true)) return rc;
  if (int rc = dev_alloc(s, static_cast<size_t>(P.poolCap) * kPairPools, &P.nbr)) return rc;
  if (!s->collideFast)  // ranges wider than two cells per axis: the shared-cell count of an entry does not fit its four bits
    if (int rc = dev_alloc(s, static_cast<size_t>(P.poolCap) * kPairPools, &P.nbrM)) return rc;
  P.frCap = n / 32 + 256;  // a chunk of 64 lanes appends at most 128 nodes to the one sub-list it is dealt to
  for (int b = 0; b < 2; ++b)
    if (int rc = dev_alloc(s, static_cast<size_t>(P.frCap) * kPairLists, &P.fr[b])) return rc;
  if (int rc = dev_alloc(s, 3ull * kPairLists * kPairPad, &P.frCount, true)) return rc;
  if (int rc = dev_alloc(s, static_cast<size_t>(kPairStripes) * kPairPad, &P.hitStripe, true)) return rc;
  if (int rc = dev_alloc(s, n, &P.bq)) return rc;
  if (int rc = dev_alloc(s, 64ull * kPairPad, &P.stat, true)) return rc;
  if (int rc = dev_alloc(s, 4ull * n, &P.grp)) return rc;
  if (int rc = dev_alloc(s, n, &P.spill)) return rc;
  if (int rc = dev_alloc(s, n, &P.left, true)) return rc;
  if (int rc = dev_alloc(s, static_cast<size_t>(kPairPools) * kPairPad, &P.pool, true)) return rc;
  return dev_alloc(s, kPairWords, &P.ctl, true);
}

// sort passes to start with: from the cell box of the scene as it stands (adapt_sort_passes follows it from there)
static uint32_t first_sort_passes(const pies_solver* s, uint32_t n) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  float rmax = 0.0f;
  for (float r : s->h_radius) if (std::isfinite(r)) rmax = std::max(rmax, r);
  const size_t stride = s->h_pos.size() / std::max<size_t>(1, n);
  for (size_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const float v = s->h_pos[i * stride + a];
      if (std::isfinite(v)) { lo[a] = std::min(lo[a], v); hi[a] = std::max(hi[a], v); }
    }
  uint32_t bits = 0;
  for (int a = 0; a < 3; ++a) {
    const double cells = hi[a] >= lo[a] ? (static_cast<double>(hi[a]) - lo[a] + 2.0 * (rmax + 0.5)) / s->opt.gridSpacing + 2.0 : 1.0;
    uint64_t ext = static_cast<uint64_t>(std::min(cells, 4.0e9));
    while (ext) { ++bits; ext >>= 1; }
  }
  return sort_passes_for(bits);
}

// the node grid: node-node collisions of PBD (`collide`), node-node contacts of PD
int alloc_node_grid(pies_solver* s, bool collide) {
  const uint32_t n = s->nodeCount();
  HashArrays& H = s->dev.hash;
  H.n = n;
  uint64_t entries = 0;
  bool fast = true;
  collision_grid_bound(s, entries, fast);
  if (n >= (1u << 25)) return fail(s, PIES_ERR_UNSUPPORTED, "node-node collisions: more than 2^25 nodes");
  if (entries > 0x7fff0000ull) return fail(s, PIES_ERR_UNSUPPORTED, "node-node collisions: more than 2^31 (cell, node) entries (gridSpacing is tiny against the radii)");
  H.maxEntries = static_cast<uint32_t>(entries + 64);
  s->sortPasses = first_sort_passes(s, n);
  s->sortCalm = 0;
  uint32_t cap = 1024;
  const uint64_t want = (collide ? s->collideFast : fast) ? 16ull * n : 2ull * H.maxEntries;  // distinct cells <= 8n resp. <= entries: load factor <= 0.5
  while (cap < want && cap < (1u << 30)) cap <<= 1;
  H.capacity = cap;
  H.mask = cap - 1;
  if (int rc = dev_alloc(s, n, &H.rng, true)) return rc;
  if (int rc = dev_alloc(s, n + 1ull, &H.entCount, true)) return rc;
  if (int rc = dev_alloc(s, n + 1ull, &H.entOff, true)) return rc;
  if (int rc = dev_alloc(s, (n + 1ull) / 2048 + 2, &H.scanSums, true)) return rc;
  if (int rc = dev_alloc(s, 6ull * ((n + 1ull + 255) / 256), &H.boxPart, true)) return rc;
  for (int b = 0; b < 2; ++b) {
    if (int rc = dev_alloc(s, H.maxEntries, &H.key[b], true)) return rc;
    if (int rc = dev_alloc(s, H.maxEntries, &H.val[b], true)) return rc;
  }
  if (int rc = dev_alloc(s, 2048ull * ((H.maxEntries + kRadixTile - 1) / kRadixTile) + 2048, &H.hist, true)) return rc;  // (digit, workgroup) counts of a pass + the digit totals
  if (int rc = dev_alloc(s, cap, &H.keys)) return rc;
  HIP_TRY(s, hipMemsetAsync(H.keys, 0xFF, static_cast<size_t>(cap) * sizeof(uint64_t), s->stream));
  if (int rc = dev_alloc(s, cap, &H.start, true)) return rc;
  if (int rc = dev_alloc(s, cap, &H.end, true)) return rc;
  if (int rc = dev_alloc(s, cap, &H.gcnt, true)) return rc;
  if (int rc = dev_alloc(s, cap, &H.done, true)) return rc;
  if (int rc = dev_alloc(s, std::min<uint64_t>(cap, H.maxEntries), &H.used, true)) return rc;
  if (int rc = dev_alloc(s, kHashCounters, &H.counters, true)) return rc;
  if (int rc = dev_alloc(s, 27ull * n, &H.passList, true)) return rc;
  if (collide)
    if (int rc = alloc_pair_lists(s)) return rc;
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return PIES_OK;
}

// PIES_FLAG_PD_NODE_CONTACTS: the element adjacency that excludes pairs from the contacts - per node, ascending, in the device's
// numbering (inside pies_finalize the host containers hold it) -, the partner lists and the friction pass's cursors and words
int nc_build(pies_solver* s) {
  const uint32_t n = s->nodeCount();
  std::vector<uint64_t> e;  // a << 32 | b, both directions
  auto join = [&](uint32_t a, uint32_t b) {
    if (a == b || a >= n || b >= n) return;
    e.push_back(static_cast<uint64_t>(a) << 32 | b);
    e.push_back(static_cast<uint64_t>(b) << 32 | a);
  };
  auto clique = [&](const uint32_t* ids, int k) {
    for (int a = 0; a < k; ++a)
      for (int b = a + 1; b < k; ++b) join(ids[a], ids[b]);
  };
  for (const HostDistance& c : s->h_distance) clique(c.ids, 2);
  for (const HostTet& c : s->h_tet) clique(c.ids, 4);
  for (const HostTet& c : s->h_volume) clique(c.ids, 4);
  for (const HostBend& c : s->h_bend) clique(c.ids, 4);
  for (size_t t = 0; t + 2 < s->h_triangles.size(); t += 3) clique(&s->h_triangles[t], 3);
  for (const HostNodePair& c : s->h_nodePair) clique(c.ids, 2);
  std::sort(e.begin(), e.end());
  e.erase(std::unique(e.begin(), e.end()), e.end());
  std::vector<uint32_t> adjPtr(n + 1ull, 0u), adj(e.size());
  for (size_t k = 0; k < e.size(); ++k) { ++adjPtr[(e[k] >> 32) + 1]; adj[k] = static_cast<uint32_t>(e[k]); }
  for (uint32_t i = 0; i < n; ++i) adjPtr[i + 1] += adjPtr[i];
  std::vector<uint64_t>().swap(e);
  NodeContactArrays& C = s->dev.nc;
  C.n = n;
  C.cap = kNcDefaultPartners;
  if (const char* v = tuning_env("PIES_PD_NODE_CONTACT_PARTNERS")) {
    const long k = std::strtol(v, nullptr, 10);
    if (k < 1 || k > 4096) return fail(s, PIES_ERR_INVALID, "PIES_PD_NODE_CONTACT_PARTNERS: 1 .. 4096");
    C.cap = static_cast<uint32_t>(k);
  }
  s->ncRounds = 8;
  if (const char* v = tuning_env("PIES_PD_NODE_CONTACT_ROUNDS")) {
    const long k = std::strtol(v, nullptr, 10);
    if (k >= 1 && k <= static_cast<long>(kNcMaxRounds)) s->ncRounds = static_cast<uint32_t>(k);
  }
  s->ncCalm = 0;
  C.rounds = s->ncRounds;
  uint32_t *adjPtrD = nullptr, *adjD = nullptr;
  if (int rc = upload(s, adjPtr, &adjPtrD)) return rc;
  if (adj.empty()) adj.push_back(0u);  // (a valid pointer; adjPtr says there is nothing)
  if (int rc = upload(s, adj, &adjD)) return rc;
  C.adjPtr = adjPtrD;
  C.adj = adjD;
  C.hostId = nullptr;
  if (s->nodeOrder.active() && s->nodeOrder.order.size() == n) {  // renumbered: the pair key stays the host's (pd_contact_kernels.h)
    uint32_t* hostIdD = nullptr;
    if (int rc = upload(s, s->nodeOrder.order, &hostIdD)) return rc;
    C.hostId = hostIdD;
  }
  if (int rc = dev_alloc(s, static_cast<size_t>(n) * C.cap, &C.part)) return rc;
  if (int rc = dev_alloc(s, n, &C.cnt, true)) return rc;
  for (int b = 0; b < 2; ++b)
    if (int rc = dev_alloc(s, n, &C.cur[b], true)) return rc;
  if (int rc = dev_alloc(s, kNcCtlWords, &C.ctl, true)) return rc;
  C.flags = s->dev.hash.counters + kCounterFlags;
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  s->dev.ncActive = true;
  return PIES_OK;
}

// strain and volume constraints added pairwise over the same elements (createTetBox and addTriMeshVolume add them that way,
// PrimitiveUtilities.cpp:401-514): one gather, one SVD, one tile plan for both
bool tet_volume_pairs(const pies_solver* s) {
  bool paired = !s->h_tet.empty() && s->h_tet.size() == s->h_volume.size();
  const bool planned = s->plan[PIES_TET].order.size() == s->h_tet.size();  // (PD: host order; a handle that has not been finalized has no plan yet)
  for (size_t k = 0; paired && k < s->h_tet.size(); ++k) {
    const HostTet &a = s->h_tet[planned ? s->plan[PIES_TET].order[k] : k], &b = s->h_volume[k];
    paired = std::memcmp(a.ids, b.ids, sizeof(a.ids)) == 0 && std::memcmp(a.qinv, b.qinv, sizeof(a.qinv)) == 0;
  }
  if (const char* e = tuning_env("PIES_NO_TET_PAIRS"); e && e[0] == '1') paired = false;
  return paired;
}

// PD: the volume records (host order) and, for elements that carry a strain and a volume constraint, the rest dictionary: the
// 64 bytes of constants of an element pair are the same for every element of one shape and material.  With few distinct sets (a
// createTetBox lattice: one per orientation) the local step reads a 16-bit index per element.
int pd_rest_dictionary(pies_solver* s) {
  DeviceScene& d = s->dev;
  const size_t count = s->h_volume.size();
  if (int rc = upload_tets(s, s->h_volume, nullptr, count, &d.d_vc_ids, &d.d_vc_q0, &d.d_vc_q1, &d.d_vc_q2)) return rc;
  // strain and volume constraints added pairwise over the same elements share one gather and one SVD
  s->tetVolumePaired = tet_volume_pairs(s);
  s->h_pairDictIndex.clear();
  const char* de = tuning_env("PIES_PD_REST_DICT");
  if (!s->tetVolumePaired || (de && de[0] == '0')) return PIES_OK;
  RestSets<16> sets;
  std::vector<uint16_t> index(count);
  const size_t cap = std::min<size_t>(4096, count / 16);  // more sets than that are no real compression: per-element arrays
  for (size_t k = 0; k < count; ++k) {
    const HostTet &a = s->h_tet[s->plan[PIES_TET].order[k]], &b = s->h_volume[k];
    RestSets<16>::Set key;
    std::memcpy(key.v, a.qinv, 9 * sizeof(float));
    key.v[9] = a.lo; key.v[10] = a.hi; key.v[11] = a.w;
    key.v[12] = b.qinv[8]; key.v[13] = b.lo; key.v[14] = b.hi; key.v[15] = b.w;
    const int set = sets.find_or_add(key, cap);
    if (set < 0) return PIES_OK;
    index[k] = static_cast<uint16_t>(set);
  }
  if (index.empty()) return PIES_OK;
  s->h_pairDictIndex = index;
  if (int rc = upload(s, index, &d.d_pairDictIndex)) return rc;
  if (int rc = upload(s, sets.table, &d.d_pairDictTable)) return rc;
  d.pairDictSets = static_cast<uint32_t>(sets.ids.size());
  return PIES_OK;
}

// PD: input of a substep, kept until its solves are known to have met the tolerance (pd_tick_checked)
int alloc_pd_snapshots(pies_solver* s) {
  const uint32_t n = s->nodeCount();
  DeviceScene& d = s->dev;
  if (!n) return PIES_OK;
  if (int rc = dev_alloc(s, n, &d.snapPos)) return rc;
  if (int rc = dev_alloc(s, n, &d.snapPrev)) return rc;
  if (int rc = dev_alloc(s, n, &d.snapVel)) return rc;
  if (d.pd.shape.count)
    if (int rc = dev_alloc(s, 4ull * d.pd.shape.count, &d.snapQuat)) return rc;
  return PIES_OK;
}

// node-node contacts stiffen the system (w = 1e5 per contact): a higher ceiling unless the host set one
void pcg_ceiling_rule(pies_solver* s) {
  if (s->pcgCeilingSet) return;
  const uint32_t ceiling = s->dev.ncActive ? 256u : 128u;
  if (s->pcgMaxIters != ceiling) { s->pcgMaxIters = ceiling; s->pcgBudget = std::min(s->pcgBudget, ceiling); }
}

}  // namespace pies
