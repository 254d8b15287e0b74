// Field props and the mesh build of a field (field_kernels.h; the rule is stated in pies_hip.h, lives in field_rule.h and is
// restated in numpy by tests/test_fields.py).
//  k_field_collide  k_prop_collide's shape: one lane per HOST node id, one workgroup per tile of 256 ids.  The records (at most
//                   64 x 160 bytes: the prop, its field's dims, origin, cell and sample base) are staged in LDS once and read as
//                   wave-wide broadcasts.  First pass: a lane walks the props in ascending index on its own node.  The lattice
//                   test - three dot products, three divisions, six comparisons - is all a node outside a prop's lattice costs;
//                   inside it the lane gathers the cell's eight samples (four pairs of neighbouring words; scattered over the
//                   wave, but neighbouring nodes mostly share cells and cache lines) and only then knows whether it is touched.
//                   The velocity is read at the first touch, and position, previous position and velocity are stored on a touch
//                   only.  Second pass: prop_tile_sums.h, shared with k_prop_collide - the touched lanes walk their touches again
//                   from the state they loaded, the same functions on the same operands (the samples are read again: they are in
//                   cache), and the tile's sums are taken in ascending node id.  No atomics.
//  k_field_points / k_field_combine  the mesh build: the lattice points for the distance and winding launches of
//                   near_kernels.h, and the two results combined into samples.
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written in field_rule.h.
#include "field_kernels.h"

#include "field_rule.h"
#include "prop_tile_sums.h"

namespace pies {
namespace {

constexpr uint32_t kFieldWords = sizeof(FieldPropRecord) / sizeof(uint32_t);
constexpr uint32_t kFieldBlock = 256;

__global__ void __launch_bounds__(kPropTile) k_field_collide(FieldPass F) {
  __shared__ FieldPropRecord props[PIES_FIELD_PROP_MAX];
  __shared__ PropTileLds lds;  // second pass
  const PropPass& P = F.base;
  const uint32_t tid = threadIdx.x, tile = blockIdx.x;
  const uint32_t h = tile * kPropTile + tid;  // host id
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(F.records);
    uint32_t* dst = reinterpret_cast<uint32_t*>(props);
    for (uint32_t k = tid; k < P.nProps * kFieldWords; k += kPropTile) dst[k] = src[k];
  }
  __syncthreads();
  const bool live = h < P.nd.n;  // (no early return: every lane meets the barriers)
  uint32_t i = 0;
  PropNode N0{};
  bool movable = false;
  if (live) {
    i = P.inv ? P.inv[h] : h;
    const float4 p4 = P.nd.pos[i];
    N0.p = V3{p4.x, p4.y, p4.z};
    N0.invMass = p4.w;
    N0.r = P.nd.radius[i];
    movable = !(p4.w == 0.0f);
  }

  // ---- first pass: the edit ----
  uint64_t touchedBy = 0;
  uint32_t last = PIES_PROP_NONE;
  float velW = 0.0f;
  if (movable) {
    PropNode N = N0;
    for (uint32_t k = 0; k < P.nProps; ++k) {
      V3 n, q;
      if (!field_contact(props[k], N.p, N.r, n, q)) continue;
      if (!touchedBy) {
        const float4 v4 = P.nd.vel[i];
        N0.v = N.v = V3{v4.x, v4.y, v4.z};
        velW = v4.w;
      }
      PropTouch T;
      prop_respond(props[k].prop, n, q, N, T);
      touchedBy |= 1ull << k;
      last = k;
    }
    if (touchedBy) {
      P.nd.pos[i] = make_float4(N.p.x, N.p.y, N.p.z, N0.invMass);
      P.nd.prev[i] = make_float4(N.p.x, N.p.y, N.p.z, 0.0f);  // (.w unused: 0 as the predict kernels and the upload write it)
      P.nd.vel[i] = make_float4(N.v.x, N.v.y, N.v.z, velW);
    }
  }
  if (P.nodeProp && live) P.nodeProp[h] = last;
  if (!P.tileMask) return;  // (uniform: a kernel argument)

  // ---- second pass: the tile's set of props and its sums (prop_tile_sums.h) ----
  PropNode N = N0;
  prop_tile_sums(lds, P.tileMask, P.tileSums, P.nProps, touchedBy, [&](uint32_t k, PropTouch& T) {
    V3 n, q;
    (void)field_contact(props[k], N.p, N.r, n, q);  // the touch of the first pass, once more
    prop_respond(props[k].prop, n, q, N, T);
  });
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
