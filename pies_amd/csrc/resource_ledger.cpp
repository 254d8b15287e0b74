// The resource ledger: see resource_ledger.h.  The only file of the library that names the wrapped HIP calls.
#include "resource_ledger.h"

#include <atomic>
#include <mutex>
#include <unordered_map>

namespace pies {
namespace ledger {
namespace {

std::atomic<uint64_t> g_live[KINDS];
std::atomic<uint64_t> g_created[KINDS];

void add(Kind k, uint64_t n = 1) {
  g_live[k].fetch_add(n, std::memory_order_relaxed);
  g_created[k].fetch_add(n, std::memory_order_relaxed);
}
void sub(Kind k, uint64_t n = 1) { g_live[k].fetch_sub(n, std::memory_order_relaxed); }

// pointer -> bytes of the live device and pinned allocations (hipFree is not told the size)
struct Sizes {
  std::mutex m;
  std::unordered_map<void*, size_t> bytes;
  void put(void* p, size_t n) {
    std::lock_guard<std::mutex> lock(m);
    bytes[p] = n;
  }
  bool take(void* p, size_t* n) {
    std::lock_guard<std::mutex> lock(m);
    auto it = bytes.find(p);
    if (it == bytes.end()) return false;
    *n = it->second;
    bytes.erase(it);
    return true;
  }
};
// never destroyed: a handle may be closed from a static destructor of the host
Sizes& device_sizes() { static Sizes* v = new Sizes; return *v; }
Sizes& pinned_sizes() { static Sizes* v = new Sizes; return *v; }

}  // namespace

hipError_t dev_malloc(void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess && *p) {
    device_sizes().put(*p, bytes);
    add(DEVICE_BYTES, bytes);
    add(DEVICE_ALLOCATIONS);
  }
  return e;
}

hipError_t dev_free(void* p) {
  if (!p) return hipSuccess;
  // the entry leaves the map BEFORE the memory goes back: another thread's allocation may return the same address at once
  size_t bytes = 0;
  if (device_sizes().take(p, &bytes)) {
    sub(DEVICE_BYTES, bytes);
    sub(DEVICE_ALLOCATIONS);
  }
  return hipFree(p);
}

hipError_t host_malloc(void** p, size_t bytes, unsigned flags) {
  const hipError_t e = hipHostMalloc(p, bytes, flags);
  if (e == hipSuccess && *p) {
    pinned_sizes().put(*p, bytes);
    add(PINNED_BYTES, bytes);
    add(PINNED_ALLOCATIONS);
  }
  return e;
}

hipError_t host_free(void* p) {
  if (!p) return hipSuccess;
  size_t bytes = 0;
  if (pinned_sizes().take(p, &bytes)) {
    sub(PINNED_BYTES, bytes);
    sub(PINNED_ALLOCATIONS);
  }
  return hipHostFree(p);
}

hipError_t stream_create(hipStream_t* st, unsigned flags) {
  const hipError_t e = hipStreamCreateWithFlags(st, flags);
  if (e == hipSuccess) add(STREAMS);
  return e;
}

hipError_t stream_destroy(hipStream_t st) {
  if (!st) return hipSuccess;
  sub(STREAMS);
  return hipStreamDestroy(st);
}

hipError_t event_create(hipEvent_t* ev) {
  const hipError_t e = hipEventCreate(ev);
  if (e == hipSuccess) add(EVENTS);
  return e;
}

hipError_t event_create(hipEvent_t* ev, unsigned flags) {
  const hipError_t e = hipEventCreateWithFlags(ev, flags);
  if (e == hipSuccess) add(EVENTS);
  return e;
}

hipError_t event_destroy(hipEvent_t ev) {
  if (!ev) return hipSuccess;
  sub(EVENTS);
  return hipEventDestroy(ev);
}

hipError_t end_capture(hipStream_t st, hipGraph_t* g) {
  *g = nullptr;
  const hipError_t e = hipStreamEndCapture(st, g);
  if (*g) add(GRAPHS);
  return e;
}

hipError_t graph_destroy(hipGraph_t g) {
  if (!g) return hipSuccess;
  sub(GRAPHS);
  return hipGraphDestroy(g);
}

hipError_t graph_instantiate(hipGraphExec_t* ge, hipGraph_t g) {
  const hipError_t e = hipGraphInstantiate(ge, g, nullptr, nullptr, 0);
  if (e == hipSuccess) add(GRAPH_EXECS);
  return e;
}

hipError_t graph_exec_destroy(hipGraphExec_t ge) {
  if (!ge) return hipSuccess;
  sub(GRAPH_EXECS);
  return hipGraphExecDestroy(ge);
}

void counts(uint64_t out[2 * KINDS]) {
  for (int k = 0; k < KINDS; ++k) {
    out[k] = g_live[k].load(std::memory_order_relaxed);
    out[KINDS + k] = g_created[k].load(std::memory_order_relaxed);
  }
}

}  // namespace ledger
}  // namespace pies
