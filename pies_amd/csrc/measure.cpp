// pies_measure_elements / pies_measure_nodes (extensions, pies_hip.h): strain, volume and momentum measures evaluated where HBM
// holds the body.  Host side only: argument checks, the lazily staged buffers (RayBuffers, solver_state.h) and the launches
// (measure_kernels.h).  Both calls are read-only: no node array is written, no stale mark is set, nothing is uploaded but the
// call's own records, and nothing here touches the substep - no captured graph, no schedule, no launch count.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "measure_kernels.h"

using namespace pies;

namespace {

// The container in HOST order with node ids in the numbering the device holds; staged once per pies_finalize (ray_free_device
// forgets it, so a pies_set_rest or an appended element is seen by the next call).
int measure_stage(pies_solver* s, int which) {
  RayBuffers& B = s->ray;
  if (B.measureStaged[which]) return PIES_OK;
  const std::vector<HostTet>& list = which ? s->h_volume : s->h_tet;  // host ids (the call is outside an InternalNumbering scope)
  const bool perm = s->nodeOrder.active() && s->nodeOrder.inv.size() == s->nodeCount();
  const size_t count = list.size();
  std::vector<uint4> id(count);
  std::vector<float4> q[3] = {std::vector<float4>(count), std::vector<float4>(count), std::vector<float4>(count)};
  for (size_t k = 0; k < count; ++k) {
    const HostTet& t = list[k];
    uint32_t ids[4];
    for (int c = 0; c < 4; ++c) ids[c] = perm ? s->nodeOrder.inv[t.ids[c]] : t.ids[c];
    id[k] = make_uint4(ids[0], ids[1], ids[2], ids[3]);
    q[0][k] = make_float4(t.qinv[0], t.qinv[1], t.qinv[2], t.qinv[3]);
    q[1][k] = make_float4(t.qinv[4], t.qinv[5], t.qinv[6], t.qinv[7]);
    q[2][k] = make_float4(t.qinv[8], t.lo, t.hi, t.w);
  }
  if (int rc = ray_grow(s, count, &B.measureIds[which])) return rc;
  for (int c = 0; c < 3; ++c)
    if (int rc = ray_grow(s, count, &B.measureQ[which][c])) return rc;
  if (count) {
    HIP_TRY(s, hipMemcpyAsync(B.measureIds[which], id.data(), count * sizeof(uint4), hipMemcpyHostToDevice, s->stream));
    for (int c = 0; c < 3; ++c)
      HIP_TRY(s, hipMemcpyAsync(B.measureQ[which][c], q[c].data(), count * sizeof(float4), hipMemcpyHostToDevice, s->stream));
  }
  HIP_TRY(s, hipStreamSynchronize(s->stream));  // the staging vectors die with this scope
  B.measureStaged[which] = true;
  return PIES_OK;
}

}  // namespace

extern "C" {

int pies_measure_elements(pies_solver_t* s, int type, uint32_t first, uint32_t n, pies_element_measure_t* out,
                          pies_element_summary_t* summary) {
  if (!s) return PIES_ERR_INVALID;
  if (type != PIES_TET && type != PIES_VOLUME) return fail(s, PIES_ERR_INVALID, "pies_measure_elements: type must be PIES_TET or PIES_VOLUME");
  const size_t size = type == PIES_TET ? s->h_tet.size() : s->h_volume.size();
  if (static_cast<uint64_t>(first) + n > size) return fail(s, PIES_ERR_INVALID, "pies_measure_elements: range beyond the container");
  if (summary) std::memset(summary, 0, sizeof(*summary));
  if (n == 0) return PIES_OK;
  if (s->device == PIES_DEVICE_NONE)
    return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): the elements are measured on the device");
  if (int rc = pies_internal_ensure_ready(s)) return rc;
  if (!out && !summary) {  // nothing asked for: the call still waits for the queued work
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    return PIES_OK;
  }
  const int which = type == PIES_VOLUME ? 1 : 0;
  if (int rc = measure_stage(s, which)) return rc;
  RayBuffers& B = s->ray;
  const uint32_t tiles = measure_tiles(first, n);
  if (out)
    if (int rc = ray_reserve(s, n, &B.measureOut, &B.measureOutCap)) return rc;
  if (summary)
    if (int rc = ray_reserve(s, tiles, &B.measureTileRecords, &B.measureTileCap, kMeasureTileWords)) return rc;
  if (summary && !B.measureSummary)
    if (int rc = ray_grow(s, kMeasureTileWords, &B.measureSummary)) return rc;

  ElementPass E;
  E.pos = s->dev.nd.pos;
  E.ids = B.measureIds[which];
  E.q0 = B.measureQ[which][0], E.q1 = B.measureQ[which][1], E.q2 = B.measureQ[which][2];
  E.first = first, E.n = n;
  E.volume = which == 1;
  E.out = out ? B.measureOut : nullptr;
  E.tileRecords = summary ? B.measureTileRecords : nullptr;
  launch_measure_elements(s->stream, E);
  if (summary) launch_measure_elements_fold(s->stream, E, B.measureSummary);
  HIP_TRY(s, hipGetLastError());
  uint32_t folded[kMeasureTileWords] = {};
  if (summary) HIP_TRY(s, hipMemcpyAsync(folded, B.measureSummary, sizeof(folded), hipMemcpyDeviceToHost, s->stream));
  if (out) HIP_TRY(s, hipMemcpyAsync(out, B.measureOut, static_cast<size_t>(n) * sizeof(*out), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  if (summary) {
    if (folded[10]) {  // an element counted: the extremes are set
      std::memcpy(&summary->volume, &folded[0], sizeof(float));
      std::memcpy(&summary->max_stretch, &folded[1], sizeof(float));
      std::memcpy(&summary->min_stretch, &folded[2], sizeof(float));
      std::memcpy(&summary->min_j, &folded[3], sizeof(float));
      std::memcpy(&summary->max_j, &folded[4], sizeof(float));
      std::memcpy(&summary->max_green, &folded[5], sizeof(float));
    }
    summary->inverted = folded[6], summary->over = folded[7], summary->under = folded[8], summary->nonfinite = folded[9];
  }
  return PIES_OK;
}

int pies_measure_nodes(pies_solver_t* s, uint32_t n_ranges, const uint32_t* ranges, const float* about, pies_node_sums_t* out) {
  if (!s) return PIES_ERR_INVALID;
  if (n_ranges > PIES_MEASURE_RANGE_MAX)
    return fail(s, PIES_ERR_UNSUPPORTED, "pies_measure_nodes: more than PIES_MEASURE_RANGE_MAX (64) ranges");
  if (n_ranges && (!ranges || !out)) return fail(s, PIES_ERR_INVALID, "pies_measure_nodes: ranges or out is NULL");
  const uint32_t nodes = s->nodeCount();
  MeasureRange records[PIES_MEASURE_RANGE_MAX];
  for (uint32_t r = 0; r < n_ranges; ++r) {
    MeasureRange& R = records[r];
    std::memset(&R, 0, sizeof(R));
    R.first = ranges[2 * r], R.count = ranges[2 * r + 1];
    if (static_cast<uint64_t>(R.first) + R.count > nodes)
      return fail(s, PIES_ERR_INVALID, "pies_measure_nodes: range " + std::to_string(r) + " leaves [0, nodes)");
    for (int c = 0; about && c < 3; ++c) {
      R.about[c] = about[3 * r + c];
      if (!std::isfinite(R.about[c])) return fail(s, PIES_ERR_INVALID, "pies_measure_nodes: about of range " + std::to_string(r) + " is not finite");
    }
  }
  if (n_ranges == 0) return PIES_OK;
  if (s->device == PIES_DEVICE_NONE)
    return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): the nodes are summed on the device");
  if (int rc = pies_internal_ensure_ready(s)) return rc;
  std::memset(out, 0, n_ranges * sizeof(*out));
  const uint32_t n = s->dev.nd.n;
  if (n == 0) {  // no nodes (every range is empty): the call still waits for the queued work
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    return PIES_OK;
  }
  RayBuffers& B = s->ray;
  if (!B.measureRanges)
    if (int rc = ray_grow(s, PIES_MEASURE_RANGE_MAX, &B.measureRanges)) return rc;
  if (!B.measureNodeOut)
    if (int rc = ray_grow(s, static_cast<size_t>(PIES_MEASURE_RANGE_MAX) * kNodeSumWords, &B.measureNodeOut)) return rc;
  const size_t tileRecords = static_cast<size_t>(prop_tiles(n)) * n_ranges;
  if (int rc = ray_reserve(s, tileRecords, &B.measureNodeTileSums, &B.measureNodeTileCap, kNodeSumWords)) return rc;
  HIP_TRY(s, hipMemcpyAsync(B.measureRanges, records, n_ranges * sizeof(MeasureRange), hipMemcpyHostToDevice, s->stream));
  NodeSumPass P;
  P.nd = s->dev.nd;
  P.inv = s->dev.d_nodeInv;
  P.ranges = B.measureRanges;
  P.nRanges = n_ranges;
  P.tileSums = B.measureNodeTileSums;
  launch_measure_nodes(s->stream, P);
  launch_measure_nodes_fold(s->stream, P, B.measureNodeOut);
  HIP_TRY(s, hipGetLastError());
  float folded[PIES_MEASURE_RANGE_MAX * kNodeSumWords];
  HIP_TRY(s, hipMemcpyAsync(folded, B.measureNodeOut, n_ranges * kNodeSumWords * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  for (uint32_t r = 0; r < n_ranges; ++r) std::memcpy(&out[r], folded + r * kNodeSumWords, sizeof(pies_node_sums_t));
  return PIES_OK;
}

}  // extern "C"
