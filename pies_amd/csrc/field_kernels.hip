// Field props and the mesh build of a field (field_kernels.h; the rule is stated in pies_hip.h, lives in field_rule.h and is
// restated in numpy by tests/test_fields.py).
//  k_field_collide  a collide edit (node_edit_device.h: collide_pass).  The records (at most 64 x 160 bytes) are the prop, its
//                   field's dims, origin, cell and sample base.  The lattice test - three dot products, three divisions, six
//                   comparisons - is all a node outside a prop's lattice costs; inside it the lane gathers the cell's eight
//                   samples (four pairs of neighbouring words; scattered over the wave, but neighbouring nodes mostly share
//                   cells and cache lines) and only then knows whether it is touched.  The second pass reads the samples again:
//                   they are in cache.
//  k_field_points / k_field_combine  the mesh build: the lattice points for the distance and winding launches of
//                   near_kernels.h, and the two results combined into samples.
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written in field_rule.h.
#include "field_kernels.h"

#include "field_rule.h"
#include "node_edit_device.h"

namespace pies {
namespace {

constexpr uint32_t kFieldBlock = 256;

__global__ void __launch_bounds__(kPropTile) k_field_collide(FieldPass F) {
  __shared__ FieldPropRecord props[PIES_FIELD_PROP_MAX];
  __shared__ PropTileLds lds;  // second pass
  stage_records(props, F.records, F.base.nProps);
  __syncthreads();
  collide_pass(
      F.base, props, lds, [](const FieldPropRecord& r, V3 p, float rad, V3& n, V3& q) { return field_contact(r, p, rad, n, q); },
      [](const FieldPropRecord& r) -> const pies_prop_t& { return r.prop; });
}

struct FieldLattice {
  float origin[3];
  float cell;
  uint32_t dims[3];
  uint32_t n;
};

__global__ void __launch_bounds__(kFieldBlock) k_field_points(FieldLattice L, float* __restrict__ points) {
  const uint32_t s = blockIdx.x * kFieldBlock + threadIdx.x;
  if (s >= L.n) return;
  const uint32_t i = s % L.dims[0], jk = s / L.dims[0];
  const uint32_t j = jk % L.dims[1], k = jk / L.dims[1];
  points[3ull * s] = L.origin[0] + static_cast<float>(i) * L.cell;
  points[3ull * s + 1] = L.origin[1] + static_cast<float>(j) * L.cell;
  points[3ull * s + 2] = L.origin[2] + static_cast<float>(k) * L.cell;
}

__global__ void __launch_bounds__(kFieldBlock) k_field_combine(uint32_t n, const float* __restrict__ distance,
                                                               const float* __restrict__ winding, float* __restrict__ samples) {
  const uint32_t s = blockIdx.x * kFieldBlock + threadIdx.x;
  if (s >= n) return;
  const float d = distance[s];
  samples[s] = fabsf(winding[s]) > 0.5f ? -d : d;
}

}  // namespace

void launch_field_collide(hipStream_t st, const FieldPass& P) {
  if (!P.base.nd.n || !P.base.nProps || P.base.nProps > PIES_FIELD_PROP_MAX) return;
  hipLaunchKernelGGL(k_field_collide, dim3(prop_tiles(P.base.nd.n)), dim3(kPropTile), 0, st, P);
}

void launch_field_points(hipStream_t st, const float origin[3], float cell, const uint32_t dims[3], float* points) {
  const uint64_t n = static_cast<uint64_t>(dims[0]) * dims[1] * dims[2];
  if (!n || n > kFieldMaxSamples) return;
  const FieldLattice L{{origin[0], origin[1], origin[2]}, cell, {dims[0], dims[1], dims[2]}, static_cast<uint32_t>(n)};
  hipLaunchKernelGGL(k_field_points, dim3((L.n + kFieldBlock - 1) / kFieldBlock), dim3(kFieldBlock), 0, st, L, points);
}

void launch_field_combine(hipStream_t st, uint32_t n, const float* distance, const float* winding, float* samples) {
  if (!n) return;
  hipLaunchKernelGGL(k_field_combine, dim3((n + kFieldBlock - 1) / kFieldBlock), dim3(kFieldBlock), 0, st, n, distance, winding, samples);
}

}  // namespace pies
