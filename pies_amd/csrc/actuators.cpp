// Actuators (extensions, pies_hip.h): pies_add_actuators, pies_get_actuators, pies_drive_actuators and pies_drive_actuators_device.
// Host side only: argument checks, the host copy of every set (pies_solver::h_actuators), the device copies with their slot map and
// the call's buffers (RayBuffers, solver_state.h), the launches (actuator_kernels.h) and the stale mark on the mirror's rest data
// (download_rest, device_scene.cpp, brings it back).  A drive writes the .x of d_dc_rw / d_bc_aw outside the captured substep -
// the words every schedule's kernels and PD's local step read through a pointer -: no graph, no plan and no launch count changes
// (DESIGN.md section 8n).  The device form shares node_io.cpp's pointer checks and event bracket.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "capi_internal.h"
#include "actuator_kernels.h"

using namespace pies;

namespace {

constexpr uint32_t kActuatorMax = 1u << 24;  // actuators per set

size_t container_size(const pies_solver* s, int32_t type) { return type == PIES_DISTANCE ? s->h_distance.size() : s->h_bend.size(); }

// nullptr, or what is wrong with the record
const char* actuator_fault(const pies_solver* s, const pies_actuator_t& a, uint32_t nChannels) {
  if (a.type != PIES_DISTANCE && a.type != PIES_BEND) return "type must be PIES_DISTANCE or PIES_BEND";
  if (a.index >= container_size(s, a.type)) return "index beyond its container";
  if (a.channel >= nChannels) return "channel must be below n_channels";
  if (!std::isfinite(a.gain) || !std::isfinite(a.lo) || !std::isfinite(a.hi)) return "gain, lo and hi must be finite";
  if (!(a.lo <= a.hi)) return "lo must not exceed hi";
  if (a.type == PIES_DISTANCE && !(a.lo >= 0.0f)) return "lo of a distance actuator must be >= 0";
  if (a.flags & ~static_cast<uint32_t>(PIES_ACTUATOR_OFFSET)) return "unknown flag";
  return nullptr;
}

// The device copy of set `id`, staged from the host copy when the handle holds none (the first drive, or after free_device): the
// records with every host index replaced by its slot - the inverse of the plan's order, which is what upload_constraints filled
// the rest records by.
int stage_set(pies_solver* s, uint32_t id, const ActuatorRecord** out) {
  ActuatorRecord*& D = s->ray.actuatorSets[id];
  if (!D) {
    HostActuatorSet& H = s->h_actuators[id];  // (H.staged outlives the asynchronous copy)
    std::vector<uint32_t> slot[2];
    for (int k = 0; k < 2; ++k) {
      if (!(H.restBits & (1u << k))) continue;
      const std::vector<uint32_t>& order = s->plan[k == 0 ? PIES_DISTANCE : PIES_BEND].order;
      slot[k].assign(container_size(s, k == 0 ? PIES_DISTANCE : PIES_BEND), UINT32_MAX);
      for (size_t q = 0; q < order.size(); ++q)
        if (order[q] < slot[k].size()) slot[k][order[q]] = static_cast<uint32_t>(q);
    }
    H.staged.resize(H.actuators.size());
    for (size_t i = 0; i < H.actuators.size(); ++i) {
      const pies_actuator_t& a = H.actuators[i];
      const uint32_t q = slot[a.type == PIES_DISTANCE ? 0 : 1][a.index];
      if (q == UINT32_MAX) return fail(s, PIES_ERR_STATE, "pies_drive_actuators: the device's plan does not hold a constraint of the set");
      H.staged[i] = ActuatorRecord{a.type, q, a.channel, a.gain, a.lo, a.hi, a.base, a.flags};
    }
    ActuatorRecord* records = nullptr;
    if (int rc = ray_grow(s, H.staged.size(), &records)) return rc;
    HIP_TRY(s, hipMemcpyAsync(records, H.staged.data(), H.staged.size() * sizeof(ActuatorRecord), hipMemcpyHostToDevice, s->stream));
    D = records;
  }
  *out = D;
  return PIES_OK;
}

// Both drive calls.  caller == nullptr with device == false: the host-pointer form.
int drive(pies_solver* s, const char* call, uint32_t set, uint32_t n_channels, const void* activation, void* out_sums, void* out_live,
          void* out_actuator, bool device, hipStream_t caller, uint32_t flags) {
  const std::string who = std::string(call) + ": ";
  if (set >= s->h_actuators.size()) return fail(s, PIES_ERR_INVALID, who + "unknown set id");
  if (n_channels != s->h_actuators[set].nChannels)
    return fail(s, PIES_ERR_INVALID, who + "n_channels must be the set's (" + std::to_string(s->h_actuators[set].nChannels) + ")");
  if (!activation) return fail(s, PIES_ERR_INVALID, who + "activation is NULL");
  if (device) {
    for (const void* q : {activation, static_cast<const void*>(out_sums), static_cast<const void*>(out_live), static_cast<const void*>(out_actuator)})
      if (reinterpret_cast<uintptr_t>(q) & 3u) return fail(s, PIES_ERR_INVALID, who + "an array pointer is not 4-byte aligned");
  } else if (!finite_all(static_cast<const float*>(activation), n_channels)) {
    return fail(s, PIES_ERR_INVALID, who + "an activation is not finite");
  }
  if (s->device == PIES_DEVICE_NONE)
    return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): the rest records are driven where the device holds them");
  HIP_TRY(s, hipSetDevice(s->device));
  const uint32_t n = static_cast<uint32_t>(s->h_actuators[set].actuators.size()), tiles = actuator_tiles(n);
  if (device) {
    if (int rc = check_device_range(s, call, activation, sizeof(float) * n_channels)) return rc;
    if (int rc = check_device_range(s, call, out_sums, 2 * sizeof(float) * n_channels)) return rc;
    if (int rc = check_device_range(s, call, out_live, sizeof(uint32_t) * n_channels)) return rc;
    if (int rc = check_device_range(s, call, out_actuator, 2ull * sizeof(float) * n)) return rc;
  }
  if (int rc = pies_internal_ensure_ready(s)) return rc;
  const HostActuatorSet& H = s->h_actuators[set];  // (pies_internal_ensure_ready leaves the sets alone)
  if (device)
    if (int rc = io_begin(s, call, caller)) return rc;

  RayBuffers& B = s->ray;
  ActuatorPass P;
  if (int rc = stage_set(s, set, &P.records)) return rc;
  const bool sums = out_sums || out_live;
  if (sums)
    if (int rc = ray_reserve(s, static_cast<size_t>(tiles) * n_channels, &B.actuatorTileRecords, &B.actuatorTileCap, kActuatorTileWords)) return rc;
  float* dSums = static_cast<float*>(out_sums);
  uint32_t* dLive = static_cast<uint32_t*>(out_live);
  float2* dOut = static_cast<float2*>(out_actuator);
  if (!device) {  // the call's own buffers in HBM
    if (!B.actuatorActivation) {
      if (int rc = ray_grow(s, PIES_ACTUATOR_CHANNEL_MAX, &B.actuatorActivation)) return rc;
      if (int rc = ray_grow(s, 2 * PIES_ACTUATOR_CHANNEL_MAX, &B.actuatorSums)) return rc;
      if (int rc = ray_grow(s, PIES_ACTUATOR_CHANNEL_MAX, &B.actuatorLive)) return rc;
    }
    if (out_actuator)
      if (int rc = ray_reserve(s, n, &B.actuatorOut, &B.actuatorOutCap)) return rc;
    HIP_TRY(s, hipMemcpyAsync(B.actuatorActivation, activation, n_channels * sizeof(float), hipMemcpyHostToDevice, s->stream));
    dSums = out_sums ? B.actuatorSums : nullptr;
    dLive = out_live ? B.actuatorLive : nullptr;
    dOut = out_actuator ? B.actuatorOut : nullptr;
  }
  P.pos = s->dev.nd.pos;
  P.dcIds = s->dev.d_dc_ids;
  P.dcRw = s->dev.d_dc_rw;
  P.bcIds = s->dev.d_bc_ids;
  P.bcAw = s->dev.d_bc_aw;
  P.nActuators = n;
  P.nChannels = n_channels;
  P.activation = device ? static_cast<const float*>(activation) : B.actuatorActivation;
  P.outActuator = dOut;
  P.tileRecords = sums ? B.actuatorTileRecords : nullptr;
  if (((H.restBits & 1u) && (!P.dcIds || !P.dcRw)) || ((H.restBits & 2u) && (!P.bcIds || !P.bcAw)) || !P.pos)
    return fail(s, PIES_ERR_STATE, who + "the device holds no records for a constraint of the set");
  launch_actuator_drive(s->stream, P);
  if (sums) launch_actuator_fold(s->stream, P.tileRecords, tiles, n_channels, dSums, dLive);
  s->restStale |= H.restBits;  // the host mirror's rest data is older than HBM (nothing is uploaded)
  if (device) return io_end(s, caller, flags);
  HIP_TRY(s, hipGetLastError());
  if (out_sums) HIP_TRY(s, hipMemcpyAsync(out_sums, dSums, 2ull * n_channels * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  if (out_live) HIP_TRY(s, hipMemcpyAsync(out_live, dLive, n_channels * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
  if (out_actuator) HIP_TRY(s, hipMemcpyAsync(out_actuator, dOut, 2ull * n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return PIES_OK;
}

}  // namespace

extern "C" {

int pies_add_actuators(pies_solver_t* s, uint32_t n, const pies_actuator_t* actuators, uint32_t n_channels, uint32_t* set) {
  if (!s) return PIES_ERR_INVALID;
  const std::string who = "pies_add_actuators: ";
  if (!actuators || n == 0) return fail(s, PIES_ERR_INVALID, who + "actuators is NULL or n is 0");
  if (n > kActuatorMax) return fail(s, PIES_ERR_UNSUPPORTED, who + "more than 2^24 actuators");
  if (s->h_actuators.size() >= PIES_ACTUATOR_SET_MAX) return fail(s, PIES_ERR_UNSUPPORTED, who + "more than PIES_ACTUATOR_SET_MAX (64) sets");
  if (n_channels == 0 || n_channels > PIES_ACTUATOR_CHANNEL_MAX)
    return fail(s, PIES_ERR_INVALID, who + "n_channels must be 1 .. PIES_ACTUATOR_CHANNEL_MAX (64)");
  for (uint32_t i = 0; i < n; ++i)
    if (const char* what = actuator_fault(s, actuators[i], n_channels))
      return fail(s, PIES_ERR_INVALID, who + "actuator " + std::to_string(i) + ": " + what);
  std::vector<uint64_t> keys(n);  // (type, index): a constraint is driven by one actuator of a set
  for (uint32_t i = 0; i < n; ++i) keys[i] = static_cast<uint64_t>(actuators[i].type) << 32 | actuators[i].index;
  std::sort(keys.begin(), keys.end());
  if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return fail(s, PIES_ERR_INVALID, who + "a constraint is listed twice");
  if (int rc = download_rest(s)) return rc;  // base is the rest datum as it stands, driven or not

  HostActuatorSet H;
  H.actuators.assign(actuators, actuators + n);
  H.nChannels = n_channels;
  for (pies_actuator_t& a : H.actuators) {
    a.base = a.type == PIES_DISTANCE ? s->h_distance[a.index].target : s->h_bend[a.index].angle;
    H.restBits |= a.type == PIES_DISTANCE ? 1u : 2u;
  }
  if (set) *set = static_cast<uint32_t>(s->h_actuators.size());
  s->h_actuators.push_back(std::move(H));
  return PIES_OK;
}

int pies_get_actuators(const pies_solver_t* s, uint32_t set, pies_actuator_t* actuators, uint32_t capacity, uint32_t* n, uint32_t* n_channels) {
  if (!s) return PIES_ERR_INVALID;
  pies_solver* m = const_cast<pies_solver*>(s);  // (the error text is the handle's)
  if (set >= s->h_actuators.size()) return fail(m, PIES_ERR_INVALID, "pies_get_actuators: unknown set id");
  const HostActuatorSet& H = s->h_actuators[set];
  if (actuators && capacity < H.actuators.size())
    return fail(m, PIES_ERR_INVALID, "pies_get_actuators: capacity is below the set's actuator count");
  if (actuators) std::memcpy(actuators, H.actuators.data(), H.actuators.size() * sizeof(pies_actuator_t));
  if (n) *n = static_cast<uint32_t>(H.actuators.size());
  if (n_channels) *n_channels = H.nChannels;
  return PIES_OK;
}

int pies_drive_actuators(pies_solver_t* s, uint32_t set, uint32_t n_channels, const float* activation, float* out_sums, uint32_t* out_live,
                         float* out_actuator) {
  if (!s) return PIES_ERR_INVALID;
  return drive(s, "pies_drive_actuators", set, n_channels, activation, out_sums, out_live, out_actuator, false, nullptr, 0u);
}

int pies_drive_actuators_device(pies_solver_t* s, uint32_t set, uint32_t n_channels, const void* activation, void* out_sums, void* out_live,
                                void* out_actuator, void* stream, uint32_t flags) {
  if (!s) return PIES_ERR_INVALID;
  return drive(s, "pies_drive_actuators_device", set, n_channels, activation, out_sums, out_live, out_actuator, true,
               static_cast<hipStream_t>(stream), flags);
}

}  // extern "C"
