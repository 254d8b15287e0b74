// Kernels of pies_read_nodes_device / pies_write_nodes_device (node_io_kernels.h).  Plain bandwidth kernels: a workgroup owns a
// tile of 256 consecutive HOST ids, one lane per node, and moves every array the call names in ONE launch - the 16-byte records
// of the node arrays on the solver's side (gathered through d_nodeInv when the scene is renumbered: the reads of
// launch_pack_xyz / launch_gather_nodes), the caller's rows on the other.  No atomics, no arithmetic: the words are copied.
// The caller's packed form (stride 3) is 12 bytes per node.  Variant "plain" moves a row as the lane's three floats; variant
// "staged" passes a tile's 768 floats through LDS so that they cross as 192 16-byte accesses when the array's base is 16-byte
// aligned (a tile starts 3 072 bytes after the one before: the base decides for every tile), with a dword path - still through
// LDS, consecutive lanes on consecutive words - for a misaligned base and the words of the last tile that do not fill a quad.
#include "node_io_kernels.h"

namespace pies {
namespace {

constexpr uint32_t kTileFloats = 3 * kNodeIoTile;

__device__ inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// `floats` (<= 768) words of a tile between LDS and the caller's array at `base`; every lane of the workgroup calls it
__device__ inline void tile_store3(const float* lds, float* base, uint32_t floats, uint32_t t) {
  if (aligned16(base)) {
    const uint32_t quads = floats >> 2;
    if (t < quads) reinterpret_cast<float4*>(base)[t] = reinterpret_cast<const float4*>(lds)[t];
    if (t < (floats & 3u)) base[4 * quads + t] = lds[4 * quads + t];
  } else {
    for (uint32_t k = t; k < floats; k += kNodeIoTile) base[k] = lds[k];
  }
}
__device__ inline void tile_load3(float* lds, const float* base, uint32_t floats, uint32_t t) {
  if (aligned16(base)) {
    const uint32_t quads = floats >> 2;
    if (t < quads) reinterpret_cast<float4*>(lds)[t] = reinterpret_cast<const float4*>(base)[t];
    if (t < (floats & 3u)) lds[4 * quads + t] = base[4 * quads + t];
  } else {
    for (uint32_t k = t; k < floats; k += kNodeIoTile) lds[k] = base[k];
  }
}

template <bool Gather, bool Staged>
__global__ void __launch_bounds__(kNodeIoTile) k_node_io_read(const NodeIoPass P) {
  __shared__ __attribute__((aligned(16))) float lds[3][Staged ? kTileFloats : 4];
  const uint32_t t = threadIdx.x, tile0 = blockIdx.x * kNodeIoTile, i = tile0 + t, n = P.nd.n;
  const bool live = i < n;
  const uint32_t d = live ? (Gather ? P.inv[i] : i) : 0u;
  const float4* const src[3] = {P.nd.pos, P.nd.prev, P.nd.vel};
  float invMass = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float* const dst = P.user[a];
    if (!dst && !(a == 0 && P.invMass)) continue;  // (uniform: the arrays the call names)
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) v = src[a][d];
    if (a == 0) invMass = v.w;
    if (!dst) continue;
    if (Staged) {  // (stride 3, decided by the launch)
      if (live) {
        lds[a][3 * t] = v.x;
        lds[a][3 * t + 1] = v.y;
        lds[a][3 * t + 2] = v.z;
      }
    } else if (live) {
      if (P.stride == 4) {
        if (aligned16(dst)) {
          reinterpret_cast<float4*>(dst)[i] = make_float4(v.x, v.y, v.z, 0.0f);
        } else {
          float* o = dst + 4ull * i;
          o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = 0.0f;
        }
      } else {
        float* o = dst + 3ull * i;
        o[0] = v.x, o[1] = v.y, o[2] = v.z;
      }
    }
  }
  if (Staged) {
    __syncthreads();
    const uint32_t floats = 3u * (n - tile0 < kNodeIoTile ? n - tile0 : kNodeIoTile);
#pragma unroll
    for (int a = 0; a < 3; ++a)
      if (P.user[a]) tile_store3(lds[a], P.user[a] + 3ull * tile0, floats, t);
  }
  if (live && P.radius) P.radius[i] = P.nd.radius[d];
  if (live && P.invMass) P.invMass[i] = invMass;
}

// record of array a for device index d from the row (x, y, z): a position keeps its inverse mass
__device__ inline void put_row(const NodeIoPass& P, int a, uint32_t d, float x, float y, float z) {
  float4* const dst = a == 0 ? P.nd.pos : a == 1 ? P.nd.prev : P.nd.vel;
  dst[d] = make_float4(x, y, z, a == 0 ? dst[d].w : 0.0f);
}

template <bool Gather, bool Staged>
__global__ void __launch_bounds__(kNodeIoTile) k_node_io_write(const NodeIoPass P) {
  __shared__ __attribute__((aligned(16))) float lds[3][Staged ? kTileFloats : 4];
  const uint32_t t = threadIdx.x, tile0 = blockIdx.x * kNodeIoTile, i = tile0 + t, n = P.nd.n;
  const bool live = i < n;
  if (Staged) {
    const uint32_t floats = 3u * (n - tile0 < kNodeIoTile ? n - tile0 : kNodeIoTile);
#pragma unroll
    for (int a = 0; a < 3; ++a)
      if (P.user[a]) tile_load3(lds[a], P.user[a] + 3ull * tile0, floats, t);
    __syncthreads();
  }
  if (!live) return;
  const uint32_t d = Gather ? P.inv[i] : i;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float* const src = P.user[a];
    if (!src) continue;
    const float* r = Staged ? &lds[a][3 * t] : src + static_cast<uint64_t>(P.stride) * i;  // (a fourth float is not looked at)
    put_row(P, a, d, r[0], r[1], r[2]);
  }
}

// indexed: one lane per row
template <bool Gather>
__global__ void __launch_bounds__(kNodeIoTile) k_node_io_write_ids(const NodeIoPass P) {
  const uint32_t k = blockIdx.x * kNodeIoTile + threadIdx.x;
  if (k >= P.m) return;
  const uint32_t id = P.ids[k];
  if (id >= P.nd.n) return;
  const uint32_t d = Gather ? P.inv[id] : id;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float* const src = P.user[a];
    if (!src) continue;
    const float* r = src + static_cast<uint64_t>(P.stride) * k;
    put_row(P, a, d, r[0], r[1], r[2]);
  }
}

template <class K>
void launch_tiles(K kernel, hipStream_t st, uint32_t items, const NodeIoPass& P) {
  hipLaunchKernelGGL(kernel, dim3((items + kNodeIoTile - 1) / kNodeIoTile), dim3(kNodeIoTile), 0, st, P);
}

}  // namespace

void launch_node_io_read(hipStream_t st, const NodeIoPass& P) {
  if (!P.nd.n) return;
  const bool staged = P.staged && P.stride == 3 && (P.user[0] || P.user[1] || P.user[2]);
  if (P.inv) {
    if (staged) launch_tiles(k_node_io_read<true, true>, st, P.nd.n, P);
    else launch_tiles(k_node_io_read<true, false>, st, P.nd.n, P);
  } else {
    if (staged) launch_tiles(k_node_io_read<false, true>, st, P.nd.n, P);
    else launch_tiles(k_node_io_read<false, false>, st, P.nd.n, P);
  }
}

void launch_node_io_write(hipStream_t st, const NodeIoPass& P) {
  if (!P.nd.n) return;
  if (P.ids) {
    if (!P.m) return;
    if (P.inv) launch_tiles(k_node_io_write_ids<true>, st, P.m, P);
    else launch_tiles(k_node_io_write_ids<false>, st, P.m, P);
    return;
  }
  const bool staged = P.staged && P.stride == 3;
  if (P.inv) {
    if (staged) launch_tiles(k_node_io_write<true, true>, st, P.nd.n, P);
    else launch_tiles(k_node_io_write<true, false>, st, P.nd.n, P);
  } else {
    if (staged) launch_tiles(k_node_io_write<false, true>, st, P.nd.n, P);
    else launch_tiles(k_node_io_write<false, false>, st, P.nd.n, P);
  }
}

}  // namespace pies
