// pies_read_nodes_device / pies_write_nodes_device / pies_read_skin_device (extensions, pies_hip.h): node state and skins to and
// from device memory of the caller, ordered against the caller's stream by two events instead of a host synchronisation.  Host
// side only: argument checks, the pointer checks, the event bracket and the launches (node_io_kernels.h, skin_kernels.h).  A
// read leaves the handle as it found it; a write edits dev.nd.pos / prev / vel - the state every schedule and both solvers start a
// substep from - outside the captured substep and marks the host mirror stale, like the props (props.cpp): no graph, no schedule
// and no launch count changes.
#include <cstring>
#include <string>

#include "capi_internal.h"
#include "node_io_kernels.h"
#include "skin_kernels.h"

using namespace pies;

namespace pies {

// `bytes` at p are device memory of the handle's device (p == nullptr: nothing to check)
int check_device_range(pies_solver* s, const char* call, const void* p, size_t bytes) {
  if (!p || !bytes) return PIES_OK;
  hipPointerAttribute_t attr;
  std::memset(&attr, 0, sizeof(attr));
  const hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) (void)hipGetLastError();  // (an unknown pointer is the caller's mistake, not a latched runtime error)
  if (e != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != s->device)
    return fail(s, PIES_ERR_INVALID, std::string(call) + ": an array pointer is not device memory of the handle's device");
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
    (void)hipGetLastError();  // (memory the runtime does not describe as one range: the attributes above are what is known)
    return PIES_OK;
  }
  const uintptr_t lo = reinterpret_cast<uintptr_t>(base), at = reinterpret_cast<uintptr_t>(p);
  if (at < lo || at - lo > size || bytes > size - (at - lo))
    return fail(s, PIES_ERR_INVALID, std::string(call) + ": an array's allocation ends before the array does");
  return PIES_OK;
}

// The caller's stream must not be capturing; then the solver's stream waits for what the caller has queued so far.
int io_begin(pies_solver* s, const char* call, hipStream_t caller) {
  hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
  const hipError_t e = hipStreamIsCapturing(caller, &status);
  if (e != hipSuccess) (void)hipGetLastError();
  if (e != hipSuccess || status != hipStreamCaptureStatusNone)
    return fail(s, PIES_ERR_STATE, std::string(call) + ": the caller's stream is capturing");
  if (!s->evIoIn) HIP_TRY(s, ledger::event_create(&s->evIoIn, hipEventDisableTiming));
  if (!s->evIoOut) HIP_TRY(s, ledger::event_create(&s->evIoOut, hipEventDisableTiming));
  HIP_TRY(s, hipEventRecord(s->evIoIn, caller));
  HIP_TRY(s, hipStreamWaitEvent(s->stream, s->evIoIn, 0));
  return PIES_OK;
}

// ... and the caller's stream waits for the call's launches
int io_end(pies_solver* s, hipStream_t caller, uint32_t flags) {
  HIP_TRY(s, hipGetLastError());
  HIP_TRY(s, hipEventRecord(s->evIoOut, s->stream));
  HIP_TRY(s, hipStreamWaitEvent(caller, s->evIoOut, 0));
  if (flags & PIES_IO_HOST_SYNC) HIP_TRY(s, hipStreamSynchronize(s->stream));
  return PIES_OK;
}

}  // namespace pies

namespace {

// the argument checks that need no device; PIES_OK or the entry point's answer
int check_nodes(pies_solver* s, const char* call, const pies_device_nodes_t* a, bool write) {
  const auto who = [&] { return std::string(call) + ": "; };
  const void* p[5] = {a->position, a->prev_position, a->velocity, a->radius, a->inv_mass};
  if (!p[0] && !p[1] && !p[2] && !p[3] && !p[4]) return fail(s, PIES_ERR_INVALID, who() + "every array pointer is NULL");
  if (a->stride != 3 && a->stride != 4) return fail(s, PIES_ERR_INVALID, who() + "stride must be 3 or 4");
  for (const void* q : p)
    if (reinterpret_cast<uintptr_t>(q) & 3u) return fail(s, PIES_ERR_INVALID, who() + "an array pointer is not 4-byte aligned");
  if (write && (p[3] || p[4]))
    return fail(s, PIES_ERR_UNSUPPORTED, who() + "radius and inv_mass cannot be written on the device (pies_write_nodes is their path)");
  return PIES_OK;
}

int io_variant(pies_solver* s, const char* call, bool* staged) {
  const char* e = tuning_env("PIES_NODE_IO_VARIANT");
  *staged = false;  // the default: DESIGN.md section 8j
  if (!e || std::strcmp(e, "plain") == 0) return PIES_OK;
  if (std::strcmp(e, "staged") != 0) return fail(s, PIES_ERR_INVALID, std::string(call) + ": PIES_NODE_IO_VARIANT must be plain or staged");
  *staged = true;
  return PIES_OK;
}

NodeIoPass open_pass(pies_solver* s, const pies_device_nodes_t* a, bool staged) {
  NodeIoPass P;
  P.nd = s->dev.nd;
  P.inv = s->dev.d_nodeInv;
  P.user[0] = static_cast<float*>(a->position);
  P.user[1] = static_cast<float*>(a->prev_position);
  P.user[2] = static_cast<float*>(a->velocity);
  P.radius = static_cast<float*>(a->radius);
  P.invMass = static_cast<float*>(a->inv_mass);
  P.ids = nullptr;
  P.m = 0;
  P.stride = a->stride;
  P.staged = staged;
  return P;
}

}  // namespace

extern "C" {

int pies_read_nodes_device(pies_solver_t* s, const pies_device_nodes_t* dst, uint32_t n, void* stream, uint32_t flags) {
  static const char* const call = "pies_read_nodes_device";
  if (!s) return PIES_ERR_INVALID;
  if (!dst) return fail(s, PIES_ERR_INVALID, std::string(call) + ": dst is NULL");
  if (int rc = check_nodes(s, call, dst, false)) return rc;
  if (n != s->nodeCount()) return fail(s, PIES_ERR_INVALID, std::string(call) + ": n does not match the node count");
  bool staged = false;
  if (int rc = io_variant(s, call, &staged)) return rc;
  if (n == 0) return PIES_OK;
  if (s->device == PIES_DEVICE_NONE)
    return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): the node state is read where the device holds it");
  HIP_TRY(s, hipSetDevice(s->device));
  const size_t row = static_cast<size_t>(dst->stride) * sizeof(float) * n;
  const void* p[5] = {dst->position, dst->prev_position, dst->velocity, dst->radius, dst->inv_mass};
  for (int a = 0; a < 5; ++a)
    if (int rc = check_device_range(s, call, p[a], a < 3 ? row : sizeof(float) * n)) return rc;
  const hipStream_t caller = static_cast<hipStream_t>(stream);
  if (int rc = pies_internal_ensure_ready(s)) return rc;
  if (s->dev.nd.n != n) return fail(s, PIES_ERR_STATE, std::string(call) + ": the device holds another node count");
  if (int rc = io_begin(s, call, caller)) return rc;
  launch_node_io_read(s->stream, open_pass(s, dst, staged));
  return io_end(s, caller, flags);
}

int pies_write_nodes_device(pies_solver_t* s, const pies_device_nodes_t* src, const uint32_t* ids, uint32_t m, void* stream, uint32_t flags) {
  static const char* const call = "pies_write_nodes_device";
  if (!s) return PIES_ERR_INVALID;
  if (!src) return fail(s, PIES_ERR_INVALID, std::string(call) + ": src is NULL");
  if (int rc = check_nodes(s, call, src, true)) return rc;
  if (reinterpret_cast<uintptr_t>(ids) & 3u) return fail(s, PIES_ERR_INVALID, std::string(call) + ": ids is not 4-byte aligned");
  if (!ids && m != s->nodeCount()) return fail(s, PIES_ERR_INVALID, std::string(call) + ": m does not match the node count (ids is NULL)");
  bool staged = false;
  if (int rc = io_variant(s, call, &staged)) return rc;
  if (m == 0) return PIES_OK;
  if (s->device == PIES_DEVICE_NONE)
    return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): the node state is written where the device holds it");
  HIP_TRY(s, hipSetDevice(s->device));
  const size_t row = static_cast<size_t>(src->stride) * sizeof(float) * m;
  const void* p[3] = {src->position, src->prev_position, src->velocity};
  for (int a = 0; a < 3; ++a)
    if (int rc = check_device_range(s, call, p[a], row)) return rc;
  if (int rc = check_device_range(s, call, ids, sizeof(uint32_t) * m)) return rc;
  const hipStream_t caller = static_cast<hipStream_t>(stream);
  if (int rc = pies_internal_ensure_ready(s)) return rc;  // (a pending pies_write_nodes is uploaded here, before the scatter)
  if (s->dev.nd.n != s->nodeCount()) return fail(s, PIES_ERR_STATE, std::string(call) + ": the device holds another node count");
  if (s->dev.nd.n == 0) return PIES_OK;  // (only ids beyond the node count)
  if (int rc = io_begin(s, call, caller)) return rc;
  NodeIoPass P = open_pass(s, src, staged);
  P.ids = ids;
  P.m = m;
  launch_node_io_write(s->stream, P);
  // the host mirror is older than HBM for the arrays written (nothing is uploaded): bit 0 positions, 1 previous positions, 2 velocities
  s->stale |= (src->position ? 1u : 0u) | (src->prev_position ? 2u : 0u) | (src->velocity ? 4u : 0u);
  return io_end(s, caller, flags);
}

int pies_read_skin_device(pies_solver_t* s, uint32_t skin, void* positions, void* normals, uint32_t n, void* stream, uint32_t flags) {
  static const char* const call = "pies_read_skin_device";
  if (!s) return PIES_ERR_INVALID;
  if (skin >= s->h_skins.size()) return fail(s, PIES_ERR_INVALID, std::string(call) + ": no such skin");
  if (!positions) return fail(s, PIES_ERR_INVALID, std::string(call) + ": positions is NULL");
  if (n != s->h_skins[skin].vertexCount()) return fail(s, PIES_ERR_INVALID, std::string(call) + ": n does not match the skin's vertex count");
  if ((reinterpret_cast<uintptr_t>(positions) | reinterpret_cast<uintptr_t>(normals)) & 3u)
    return fail(s, PIES_ERR_INVALID, std::string(call) + ": an array pointer is not 4-byte aligned");
  if (n == 0) return PIES_OK;
  if (s->device == PIES_DEVICE_NONE) return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): skins are evaluated on the device");
  HIP_TRY(s, hipSetDevice(s->device));
  const size_t bytes = 3ull * n * sizeof(float);
  if (int rc = check_device_range(s, call, positions, bytes)) return rc;
  if (int rc = check_device_range(s, call, normals, bytes)) return rc;
  const hipStream_t caller = static_cast<hipStream_t>(stream);
  if (int rc = pies_internal_ensure_ready(s)) return rc;
  if (skin + 1 >= s->skinFirst.size() || s->skinFirst[skin + 1] - s->skinFirst[skin] != n)
    return fail(s, PIES_ERR_STATE, std::string(call) + ": the device holds other skins");
  if (int rc = io_begin(s, call, caller)) return rc;
  // the launches index a skin's vertices in the concatenation of all skins: vertex `first` is the caller's row 0
  const uint32_t first = s->skinFirst[skin];
  const uintptr_t shift = 3ull * first * sizeof(float);
  float* dPos = reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(positions) - shift);
  launch_skin_positions(s->stream, s->skin, s->dev.nd.pos, dPos, first, n);
  if (normals) launch_skin_normals(s->stream, s->skin, dPos, reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(normals) - shift), first, n);
  return io_end(s, caller, flags);
}

}  // extern "C"
