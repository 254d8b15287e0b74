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
//  k_load_evaluate  a velocity edit (node_edit_device.h: velocity_edit_pass) with records and states staged in LDS; only a node
//                   with a row in the node -> triangle incidence is movable.  A lane walks its row once per load whose range
//                   the row reaches, skips the entries outside the range and recomputes each incident triangle's F: the same F
//                   on the same operands in every lane that shares the triangle, no atomics and no per-triangle buffer.
//                   Positions are never written, so a list without a fluid drag reads nothing another lane writes and stores
//                   in place; a drag reads the corners' velocities, and its list takes the scratch variant, which
//                   k_force_commit (force_kernels.hip) commits.
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written in load_rule.h.
#include "load_kernels.h"

#include "load_rule.h"
#include "node_edit_device.h"

namespace pies {
namespace {

constexpr uint32_t kLoadBatch = 8;  // loads per trip through LDS in k_load_measure
static_assert(sizeof(pies_surface_load_t) == 64, "pies_surface_load_t is 16 words without padding");
static_assert(sizeof(LoadState) == 16, "LoadState is 4 words");
static_assert(kLoadTile == kPropTile, "k_load_measure stages its records like the edit kernels");
static_assert(PIES_LOAD_MAX <= PIES_PROP_MAX, "the reaction's buffers and the 64-bit tile word are the props'");
static_assert(PIES_LOAD_MAX % kLoadBatch == 0 && 2 * kLoadBatch <= 64, "one wavefront adds a batch's columns");

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
  stage_records(loads, P.loads, n);
  __syncthreads();
  if (tid < n && loads[tid].count) {  // (an empty range names no triangle)
    const float4 o = P.base.nd.pos[P.surface.tri[3ull * loads[tid].first]];
    origin[tid][0] = o.x, origin[tid][1] = o.y, origin[tid][2] = o.z;
  }
  const bool live = t < P.surface.nTris;
  V3 a{}, b{}, c{};
  if (live) {
    const uint32_t* id = P.surface.tri + 3ull * t;
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
  const SurfaceIncidence& I = F.surface;
  stage_records(loads, F.loads, P.nProps);
  stage_records(states, F.state, P.nProps);
  __syncthreads();
  EditLane lane = edit_lane(P);
  uint32_t rowBegin = 0, rowEnd = 0, rowFirst = 0, rowLast = 0;
  if (lane.live) {
    rowBegin = I.incPtr[lane.h], rowEnd = I.incPtr[lane.h + 1];
    lane.movable = lane.movable && rowBegin < rowEnd;  // (a node of no triangle bears no load)
    if (lane.movable) rowFirst = I.inc[rowBegin], rowLast = I.inc[rowEnd - 1];  // (a row ascends)
  }
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
      const uint32_t t = I.inc[e];
      if (!load_holds(L, t)) continue;
      uint32_t ia, ib, ic;
      load_corners(L, I.tri + 3ull * t, ia, ib, ic);
      V3 N;
      float nn, pressure;
      if (!load_face(L, S, xyz(P.nd.pos[ia]), xyz(P.nd.pos[ib]), xyz(P.nd.pos[ic]), N, nn, pressure)) continue;
      V3 force = load_force(N, pressure);
      if (drag) force = load_force_drag(L, force, nn, xyz(P.nd.vel[ia]), xyz(P.nd.vel[ib]), xyz(P.nd.vel[ic]));
      dv = add(dv, load_share(force, F.dt, lane.w));
      hit = true;
    }
    if (hit) need_velocity(P, lane);
    return hit;
  };
  velocity_edit_pass<kScratch>(P, F.scratch, lds, lane, evaluate, [&](uint32_t k) { return load3(loads[k].point); });
}

bool launchable(const LoadPass& P) {
  const SurfaceIncidence& I = P.surface;
  return P.base.nd.n && I.nTris && P.base.nProps && P.base.nProps <= PIES_LOAD_MAX && P.loads && I.tri && I.incPtr && I.inc && P.state;
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
  if (P.scratch.newVel) hipLaunchKernelGGL(k_load_evaluate<true>, grid, block, 0, st, P);
  else hipLaunchKernelGGL(k_load_evaluate<false>, grid, block, 0, st, P);
}

}  // namespace pies
