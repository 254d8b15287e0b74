// Kinematic props (prop_kernels.h; the rule is stated in pies_hip.h, lives in prop_rule.h and is restated in numpy by
// tests/test_props.py).
//  k_prop_collide  one lane per HOST node id, one workgroup per tile of 256 ids.  The props (at most 64 x 120 bytes) are staged in
//                  LDS once and read as wave-wide broadcasts.  First pass: a lane walks the props in ascending index on its own
//                  node - position and radius are all an untouched node costs; the velocity is read at the first touch, and
//                  position, previous position and velocity are stored on a touch only - and remembers which props touched it.
//                  Second pass, only when the host asked for the reaction and only in a tile with a touch (one test, uniform over
//                  the workgroup): the touched lanes walk their touches again from the state they loaded - the same functions on
//                  the same operands, the same bits - and for every prop that touched the tile the impulses and torques go through
//                  LDS to six lanes, each of which adds one component in ascending node id (the touched lanes from the waves'
//                  ballots: an untouched node would add 0, which changes no bit of a sum that started at +0).  No atomics.  The
//                  second pass is prop_tile_sums.h's, shared with k_field_collide.
//  k_prop_fold     one workgroup per prop: the tile records, 256 tiles at a time through LDS, added in ascending tile index by six
//                  lanes (a tile outside a prop's set adds 0; 256 tiles without one are passed over); a seventh adds the hit counts.
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written in prop_rule.h.
#include "prop_kernels.h"

#include "prop_tile_sums.h"

namespace pies {
namespace {

constexpr uint32_t kPropWords = sizeof(pies_prop_t) / sizeof(uint32_t);
static_assert(sizeof(pies_prop_t) == 120 && sizeof(pies_prop_t) % sizeof(uint32_t) == 0, "pies_prop_t is 30 words without padding");

__global__ void __launch_bounds__(kPropTile) k_prop_collide(PropPass P) {
  __shared__ pies_prop_t props[PIES_PROP_MAX];
  __shared__ PropTileLds lds;  // second pass
  const uint32_t tid = threadIdx.x, tile = blockIdx.x;
  const uint32_t h = tile * kPropTile + tid;  // host id
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(P.props);
    uint32_t* dst = reinterpret_cast<uint32_t*>(props);
    for (uint32_t k = tid; k < P.nProps * kPropWords; k += kPropTile) dst[k] = src[k];
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
      if (!prop_contact(props[k], N.p, N.r, n, q)) continue;
      if (!touchedBy) {
        const float4 v4 = P.nd.vel[i];
        N0.v = N.v = V3{v4.x, v4.y, v4.z};
        velW = v4.w;
      }
      PropTouch T;
      prop_respond(props[k], n, q, N, T);
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
    (void)prop_contact(props[k], N.p, N.r, n, q);  // the touch of the first pass, once more
    prop_respond(props[k], n, q, N, T);
  });
}

__global__ void __launch_bounds__(kPropTile) k_prop_fold(const uint64_t* __restrict__ tileMask, const float* __restrict__ tileSums,
                                                         uint32_t nTiles, uint32_t nProps, float* __restrict__ out) {
  __shared__ uint32_t chunk[7][kPropTile];  // bits: six floats and the hit count of 256 tiles
  const uint32_t tid = threadIdx.x, k = blockIdx.x;
  float sum = 0.0f;
  uint32_t hits = 0;
  for (uint32_t base = 0; base < nTiles; base += kPropTile) {
    const uint32_t t = base + tid;
    const bool has = t < nTiles && ((tileMask[t] >> k) & 1ull);
    if (!__syncthreads_or(has)) continue;  // (uniform) 256 tiles the prop did not touch: they would add 0
    const uint32_t* record = reinterpret_cast<const uint32_t*>(tileSums) + (static_cast<size_t>(t) * nProps + k) * kPropSumWords;
#pragma unroll
    for (uint32_t c = 0; c < 7; ++c) chunk[c][tid] = has ? record[c] : 0u;  // (a tile outside the set: +0.0f and no hits)
    __syncthreads();
    const uint32_t count = min(kPropTile, nTiles - base);
    if (tid < 6)
#pragma unroll 8
      for (uint32_t j = 0; j < count; ++j) sum = sum + __uint_as_float(chunk[tid][j]);  // (the reads do not wait for the sum)
    else if (tid == 6)
      for (uint32_t j = 0; j < count; ++j) hits += chunk[6][j];
    __syncthreads();  // the chunk is free for the next 256 tiles
  }
  if (tid < 6) out[k * kPropSumWords + tid] = sum;
  else if (tid == 6) reinterpret_cast<uint32_t*>(out)[k * kPropSumWords + 6] = hits;
}

}  // namespace

void launch_prop_collide(hipStream_t st, const PropPass& P) {
  if (!P.nd.n || !P.nProps || P.nProps > PIES_PROP_MAX) return;
  hipLaunchKernelGGL(k_prop_collide, dim3(prop_tiles(P.nd.n)), dim3(kPropTile), 0, st, P);
}

void launch_prop_fold(hipStream_t st, const PropPass& P, float* out) {
  if (!P.nd.n || !P.nProps || P.nProps > PIES_PROP_MAX || !P.tileMask) return;
  hipLaunchKernelGGL(k_prop_fold, dim3(P.nProps), dim3(kPropTile), 0, st, P.tileMask, P.tileSums, prop_tiles(P.nd.n), P.nProps, out);
}

}  // namespace pies
