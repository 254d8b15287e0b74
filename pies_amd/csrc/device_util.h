// Small HBM helpers shared by the host translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "solver_state.h"

namespace pies {

#define HIP_TRY(s, expr)                                                                    \
  do {                                                                                      \
    hipError_t e__ = (expr);                                                                \
    if (e__ != hipSuccess)                                                                  \
      return ::pies::fail((s), PIES_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
  } while (0)

template <class T> int dev_alloc(pies_solver* s, size_t count, T** d, bool zero = false) {
  *d = nullptr;
  if (count == 0) return PIES_OK;
  void* p = nullptr;
  HIP_TRY(s, ledger::dev_malloc(&p, count * sizeof(T)));
  s->dev.allocations.push_back(p);
  if (zero) HIP_TRY(s, hipMemsetAsync(p, 0, count * sizeof(T), s->stream));
  *d = static_cast<T*>(p);
  return PIES_OK;
}

// Allocates and copies; synchronises the stream so the caller's staging vector may die.
template <class T> int upload(pies_solver* s, const std::vector<T>& h, T** d) {
  if (int rc = dev_alloc(s, h.size(), d)) return rc;
  if (h.empty()) return PIES_OK;
  HIP_TRY(s, hipMemcpyAsync(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return PIES_OK;
}

// Frees the temporaries dev_alloc / upload have listed in s->dev.allocations since construction (trimesh.cpp, fields.cpp).
struct Temporaries {
  pies_solver* s;
  size_t mark;
  explicit Temporaries(pies_solver* solver) : s(solver), mark(solver->dev.allocations.size()) {}
  ~Temporaries() {
    if (s->dev.allocations.size() > mark) (void)hipStreamSynchronize(s->stream);
    while (s->dev.allocations.size() > mark) {
      (void)ledger::dev_free(s->dev.allocations.back());
      s->dev.allocations.pop_back();
    }
  }
};

// The PD system matrix as CSR (pd_setup.cpp), in the numbering the host containers hold
struct PdSystem {
  std::vector<uint32_t> rowptr, col;
  std::vector<float> val, kdiag;
};
void pd_assemble(const pies_solver* s, PdSystem& K);
bool pd_row_dictionary_applies(const PdSystem& K);  // pd_build would give K a row dictionary (PIES_ROW_STENCILS > 0)
uint32_t pd_window_chunk_rows();                    // rows per chunk of the windowed matrix (PIES_CG_CHUNK_ROWS, default 256)
int pd_build(pies_solver* s);         // pd_setup.cpp
int pd_upload_goals(pies_solver* s);  // pd_setup.cpp
bool pd_plan_tiles(const pies_solver* s, PdTilePlan& out);  // pd_tiles.cpp; false: the scene keeps per-(element, node) records

}  // namespace pies
