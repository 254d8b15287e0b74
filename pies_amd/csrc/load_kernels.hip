// Surface loads (load_kernels.h; the rule is stated in pies_hip.h, lives in load_rule.h and is restated in numpy by
// tests/test_loads.py).
//  k_load_measure   one workgroup per tile of kLoadTile container indices that some load's range meets (the host lists them), one
//                   lane per triangle.  The records (at most 64 x 64 bytes) and per load the corner o its volume is taken about
//                   are staged in LDS.  A lane reads its triangle once and forms six_t and area_t for each load whose range holds
//                   it; the loads go through LDS kLoadBatch at a time, and 2 x kLoadBatch lanes add one (load, quantity) column
//                   each in ascending index (a lane outside the range has written +0.0f, which changes no bit of a sum that
//                   started at +0.0f).
//  k_load_fold      one workgroup per load: the records of the tiles its range meets, 256 slots at a time through LDS, added in
//                   ascending tile index by two lanes; then V, A and the pressure (load_state) to HBM, where the evaluate launch
//                   reads them - the gas pressure never visits the host.
//  k_load_evaluate  k_force_evaluate's shape: one lane per HOST node id, one workgroup per tile of 256 ids, records and states
//                   staged in LDS and read as wave-wide broadcasts.  A lane walks its row of the node -> triangle incidence once
//                   per load whose range the row reaches, skips the entries outside the range and recomputes each incident
//                   triangle's F: the same F on the same operands in every lane that shares the triangle, no atomics and no
//                   per-triangle buffer.  Positions are never written, so a list without a fluid drag reads nothing another lane
//                   writes and stores in place; a drag reads the corners' velocities, and its list writes newVel[host id] and
//                   the wave's ballot, which k_force_commit (force_kernels.hip) commits.  Second pass, only when the host asked
//                   for the reaction: prop_tile_sums.h, shared with the props and the forces.
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written in load_rule.h.
#include "load_kernels.h"

#include "load_rule.h"
#include "prop_tile_sums.h"

namespace pies {
namespace {

constexpr uint32_t kLoadWords = sizeof(pies_surface_load_t) / sizeof(uint32_t);
constexpr uint32_t kLoadBatch = 8;  // loads per trip through LDS in k_load_measure
static_assert(sizeof(pies_surface_load_t) == 64, "pies_surface_load_t is 16 words without padding");
static_assert(sizeof(LoadState) == 16, "LoadState is 4 words");
static_assert(PIES_LOAD_MAX <= PIES_PROP_MAX, "the reaction's buffers and the 64-bit tile word are the props'");
static_assert(PIES_LOAD_MAX % kLoadBatch == 0 && 2 * kLoadBatch <= 64, "one wavefront adds a batch's columns");

PIES_DEV V3 xyz(const float4& a) { return V3{a.x, a.y, a.z}; }

PIES_DEV void stage_loads(pies_surface_load_t* dst, const pies_surface_load_t* src, uint32_t n) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);
  for (uint32_t k = threadIdx.x; k < n * kLoadWords; k += blockDim.x) d[k] = s[k];
}

// whether triangle t is of L's range / whether the tile is met by it (count is resolved: first + count <= the container's size)
PIES_DEV bool load_holds(const pies_surface_load_t& L, uint32_t t) { return t >= L.first && t - L.first < L.count; }
PIES_DEV bool load_meets(const pies_surface_load_t& L, uint32_t tile) {
  const uint64_t lo = static_cast<uint64_t>(tile) * kLoadTile;
  return L.count && L.first < lo + kLoadTile && static_cast<uint64_t>(L.first) + L.count > lo;
}

__global__ void __launch_bounds__(kLoadTile) k_load_measure(LoadPass P) {
  __shared__ pies_surface_load_t loads[PIES_LOAD_MAX];
  __shared__ float origin[PIES_LOAD_MAX][3];
  __shared__ float stage[kLoadTile][2 * kLoadBatch];  // (index major: the adding lanes read consecutive words)
  const uint32_t tid = threadIdx.x, slot = blockIdx.x, n = P.base.nProps;
  const uint32_t tile = P.tiles[slot];
  const uint32_t t = tile * kLoadTile + tid;
  stage_loads(loads, P.loads, n);
  __syncthreads();
  if (tid < n && loads[tid].count) {  // (an empty range names no triangle)
    const float4 o = P.base.nd.pos[P.tri[3ull * loads[tid].first]];
    origin[tid][0] = o.x, origin[tid][1] = o.y, origin[tid][2] = o.z;
  }
  const bool live = t < P.nTris;
  V3 a{}, b{}, c{};
  if (live) {
    const uint32_t* id = P.tri + 3ull * t;
    a = xyz(P.base.nd.pos[id[0]]);
    b = xyz(P.base.nd.pos[id[1]]);
    c = xyz(P.base.nd.pos[id[2]]);
  }
  __syncthreads();
  for (uint32_t base = 0; base < n; base += kLoadBatch) {
    bool any = false;
    for (uint32_t j = 0; j < kLoadBatch && base + j < n; ++j) any = any || load_meets(loads[base + j], tile);
    if (!any) continue;  // (uniform: every lane read the same words)
#pragma unroll
    for (uint32_t j = 0; j < kLoadBatch; ++j) {
      const uint32_t k = base + j;
      float six = 0.0f, area = 0.0f;
      if (k < n && live && load_holds(loads[k], t)) {
        const bool inward = loads[k].flags & PIES_LOAD_INWARD;
        load_measure(load3(origin[k]), a, inward ? c : b, inward ? b : c, six, area);
      }
      stage[tid][2 * j] = six;
      stage[tid][2 * j + 1] = area;
    }
    __syncthreads();
    const uint32_t k = base + (tid >> 1);
    if (tid < 2 * kLoadBatch && k < n && load_meets(loads[k], tile)) {
      float sum = 0.0f;
#pragma unroll 8
      for (uint32_t i = 0; i < kLoadTile; ++i) sum = sum + stage[i][tid];
      reinterpret_cast<float*>(P.tileSums)[(static_cast<size_t>(slot) * n + k) * 2 + (tid & 1u)] = sum;
    }
    __syncthreads();  // the stage is free for the next batch
  }
}

__global__ void __launch_bounds__(kLoadTile) k_load_fold(LoadPass P) {
  __shared__ float chunk[2][kLoadTile];
  __shared__ float total[2];
  const uint32_t tid = threadIdx.x, k = blockIdx.x, n = P.base.nProps;
  const pies_surface_load_t L = P.loads[k];
  float sum = 0.0f;
  for (uint32_t base = 0; base < P.nSlots; base += kLoadTile) {
    const uint32_t slot = base + tid;
    const bool has = slot < P.nSlots && load_meets(L, P.tiles[slot]);
    if (!__syncthreads_or(has)) continue;  // (uniform) 256 tiles outside the range
    const float2 record = has ? P.tileSums[static_cast<size_t>(slot) * n + k] : make_float2(0.0f, 0.0f);
    chunk[0][tid] = record.x;
    chunk[1][tid] = record.y;
    __syncthreads();
    const uint32_t count = min(kLoadTile, P.nSlots - base);
    if (tid < 2)
#pragma unroll 8
      for (uint32_t j = 0; j < count; ++j) sum = sum + chunk[tid][j];
    __syncthreads();  // the chunk is free for the next 256 slots
  }
  if (tid < 2) total[tid] = sum;
  __syncthreads();
  if (tid == 0) P.state[k] = load_state(L, total[0], total[1]);
}

template <bool kScratch>
__global__ void __launch_bounds__(kPropTile) k_load_evaluate(LoadPass F) {
  __shared__ pies_surface_load_t loads[PIES_LOAD_MAX];
  __shared__ LoadState states[PIES_LOAD_MAX];
  __shared__ PropTileLds lds;  // second pass
  const PropPass& P = F.base;
  const uint32_t tid = threadIdx.x, tile = blockIdx.x;
  const uint32_t h = tile * kPropTile + tid;  // host id
  stage_loads(loads, F.loads, P.nProps);
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(F.state);
    uint32_t* dst = reinterpret_cast<uint32_t*>(states);
    for (uint32_t k = tid; k < P.nProps * 4u; k += kPropTile) dst[k] = src[k];
  }
  __syncthreads();
  const bool live = h < P.nd.n;  // (no early return: every lane meets the barriers)
  uint32_t i = 0, rowBegin = 0, rowEnd = 0, rowFirst = 0, rowLast = 0;
  V3 p{}, v{};
  float w = 0.0f, velW = 0.0f;
  bool movable = false, haveVel = false;
  if (live) {
    i = P.inv ? P.inv[h] : h;
    const float4 p4 = P.nd.pos[i];
    p = xyz(p4);
    w = p4.w;
    rowBegin = F.incPtr[h], rowEnd = F.incPtr[h + 1];
    movable = !(w == 0.0f) && rowBegin < rowEnd;
    if (movable) rowFirst = F.inc[rowBegin], rowLast = F.inc[rowEnd - 1];  // (a row ascends)
  }
  auto need_velocity = [&]() {
    if (haveVel) return;
    const float4 v4 = P.nd.vel[i];
    v = xyz(v4);
    velW = v4.w;
    haveVel = true;
  };
  // dv of load k on this lane's (movable) node from the state the call found; false: not affected
  auto evaluate = [&](uint32_t k, V3& dv) -> bool {
    const pies_surface_load_t& L = loads[k];
    const LoadState& S = states[k];
    if (!S.acts || !L.count) return false;                                 // (uniform)
    if (rowLast < L.first || (rowFirst >= L.first && rowFirst - L.first >= L.count)) return false;  // the row does not reach the range
    const bool drag = kScratch && L.type == PIES_LOAD_FLUID && L.drag != 0.0f;  // (the host never launches the in-place variant with one)
    bool hit = false;
    dv = V3{0.0f, 0.0f, 0.0f};
    for (uint32_t e = rowBegin; e < rowEnd; ++e) {
      const uint32_t t = F.inc[e];
      if (!load_holds(L, t)) continue;
      uint32_t ia, ib, ic;
      load_corners(L, F.tri + 3ull * t, ia, ib, ic);
      V3 N;
      float nn, pressure;
      if (!load_face(L, S, xyz(P.nd.pos[ia]), xyz(P.nd.pos[ib]), xyz(P.nd.pos[ic]), N, nn, pressure)) continue;
      V3 force = load_force(N, pressure);
      if (drag) force = load_force_drag(L, force, nn, xyz(P.nd.vel[ia]), xyz(P.nd.vel[ib]), xyz(P.nd.vel[ic]));
      dv = add(dv, load_share(force, F.dt, w));
      hit = true;
    }
    if (hit) need_velocity();
    return hit;
  };

  // ---- first pass: the edit ----
  uint64_t affectedBy = 0;
  if (movable) {
    V3 sum{0.0f, 0.0f, 0.0f};
    for (uint32_t k = 0; k < P.nProps; ++k) {
      V3 dv;
      if (!evaluate(k, dv)) continue;
      sum = add(sum, dv);
      affectedBy |= 1ull << k;
    }
    if (affectedBy) {
      const V3 v1 = add(v, sum);
      if (kScratch) F.newVel[h] = make_float4(v1.x, v1.y, v1.z, velW);
      else P.nd.vel[i] = make_float4(v1.x, v1.y, v1.z, velW);
    }
  }
  if (kScratch) {
    const uint64_t ballot = __builtin_amdgcn_ballot_w64(affectedBy != 0);
    if ((tid & 63u) == 0) F.affected[tile * kForceWaves + (tid >> 6)] = ballot;
  }
  if (!P.tileMask) return;  // (uniform: a kernel argument)

  // ---- second pass: the tile's set of loads and its sums (prop_tile_sums.h) ----
  prop_tile_sums(lds, P.tileMask, P.tileSums, P.nProps, affectedBy, [&](uint32_t k, PropTouch& T) {
    V3 dv{};
    (void)evaluate(k, dv);  // the change of the first pass, once more
    T.impulse = scale(dv, 1.0f / w);
    T.torque = cross(sub(p, load3(loads[k].point)), T.impulse);
  });
}

bool launchable(const LoadPass& P) {
  return P.base.nd.n && P.nTris && P.base.nProps && P.base.nProps <= PIES_LOAD_MAX && P.loads && P.tri && P.incPtr && P.inc && P.state;
}

}  // namespace

void launch_load_measure(hipStream_t st, const LoadPass& P) {
  if (!launchable(P) || !P.nSlots || !P.tiles || !P.tileSums) return;
  hipLaunchKernelGGL(k_load_measure, dim3(P.nSlots), dim3(kLoadTile), 0, st, P);
}

void launch_load_fold(hipStream_t st, const LoadPass& P) {
  if (!launchable(P)) return;
  hipLaunchKernelGGL(k_load_fold, dim3(P.base.nProps), dim3(kLoadTile), 0, st, P);
}

void launch_load_evaluate(hipStream_t st, const LoadPass& P) {
  if (!launchable(P)) return;
  const dim3 grid(prop_tiles(P.base.nd.n)), block(kPropTile);
  if (P.newVel) hipLaunchKernelGGL(k_load_evaluate<true>, grid, block, 0, st, P);
  else hipLaunchKernelGGL(k_load_evaluate<false>, grid, block, 0, st, P);
}

void launch_load_commit(hipStream_t st, const LoadPass& P) {
  if (!launchable(P) || !P.newVel) return;
  launch_velocity_commit(st, P.base.nd, P.base.inv, P.newVel, P.affected);
}

}  // namespace pies
