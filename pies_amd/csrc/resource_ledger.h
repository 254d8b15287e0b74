// Counted wrappers for every HIP resource the library creates or destroys (pies_resource_counts).  All other files of csrc/
// go through these - tests/test_resource_ledger.py fails on a raw call - so what a handle holds, and whether it gives it back,
// can be read from outside.  The counters are process-wide atomics; only device and pinned allocations take a mutex (the map
// from pointer to bytes).  Nothing here is called inside a captured substep or a tick.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace pies {
namespace ledger {

// index of a kind in either half of pies_resource_counts' sixteen words (live: 0..7, created since load: 8..15)
enum Kind { DEVICE_BYTES = 0, DEVICE_ALLOCATIONS, PINNED_BYTES, PINNED_ALLOCATIONS, STREAMS, EVENTS, GRAPHS, GRAPH_EXECS, KINDS };

hipError_t dev_malloc(void** p, size_t bytes);
template <class T> hipError_t dev_malloc(T** p, size_t bytes) { return dev_malloc(reinterpret_cast<void**>(p), bytes); }
hipError_t dev_free(void* p);  // nullptr: nothing is counted
hipError_t host_malloc(void** p, size_t bytes, unsigned flags);
template <class T> hipError_t host_malloc(T** p, size_t bytes, unsigned flags) { return host_malloc(reinterpret_cast<void**>(p), bytes, flags); }
hipError_t host_free(void* p);
hipError_t stream_create(hipStream_t* st, unsigned flags);
hipError_t stream_destroy(hipStream_t st);
hipError_t event_create(hipEvent_t* e);
hipError_t event_create(hipEvent_t* e, unsigned flags);
hipError_t event_destroy(hipEvent_t e);
// the end of a stream capture creates a graph (counted when *g comes back non-null, whatever the status)
hipError_t end_capture(hipStream_t st, hipGraph_t* g);
hipError_t graph_destroy(hipGraph_t g);
hipError_t graph_instantiate(hipGraphExec_t* ge, hipGraph_t g);
hipError_t graph_exec_destroy(hipGraphExec_t ge);

void counts(uint64_t out[2 * KINDS]);

}  // namespace ledger
}  // namespace pies
