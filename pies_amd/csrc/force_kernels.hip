// Force fields (force_kernels.h; the rule is stated in pies_hip.h, lives in force_rule.h and is restated in numpy by
// tests/test_forces.py).
//  k_force_evaluate  k_prop_collide's shape: one lane per HOST node id, one workgroup per tile of 256 ids.  The records (at most
//                    64 x 48 bytes) are staged in LDS once and read as wave-wide broadcasts.  First pass: a lane walks the forces
//                    in ascending index on its own node.  Every force reads the state the call found, so the walk keeps one sum of
//                    velocity changes; a node in no region pays its position only, the velocity is read at the first force whose
//                    region holds the node.  A wind walks the node's row of the incidence (by host id, ascending triangle
//                    index): per entry the triangle's three positions, and only for a triangle that contributes its three
//                    velocities - the same F on the same operands in every lane that shares the triangle, no atomics and no
//                    per-triangle buffer.  kScratch: the new velocity goes to newVel[host id] and the wave's ballot of affected
//                    lanes to `affected`; otherwise (no wind in the list: no lane reads another node's velocity) it is stored
//                    in place.  Second pass, only when the host asked for the reaction: prop_tile_sums.h, shared with
//                    k_prop_collide - the affected lanes evaluate their forces again from the state they loaded, the same
//                    functions on the same operands, and the tile's sums are taken in ascending node id.
//  k_force_commit    the scratch variant's second launch: one lane per host id reads its wave's word of `affected` (one broadcast)
//                    and, when its bit is set, moves newVel[host id] to the node's velocity.
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written in force_rule.h.
#include "force_kernels.h"

#include "force_rule.h"
#include "prop_tile_sums.h"

namespace pies {
namespace {

constexpr uint32_t kForceWords = sizeof(pies_force_t) / sizeof(uint32_t);
static_assert(sizeof(pies_force_t) == 48 && sizeof(pies_force_t) % sizeof(uint32_t) == 0, "pies_force_t is 12 words without padding");
static_assert(PIES_FORCE_MAX <= PIES_PROP_MAX, "the reaction's buffers and the 64-bit tile word are the props'");

PIES_DEV V3 xyz(const float4& a) { return V3{a.x, a.y, a.z}; }

template <bool kScratch>
__global__ void __launch_bounds__(kPropTile) k_force_evaluate(ForcePass F) {
  __shared__ pies_force_t forces[PIES_FORCE_MAX];
  __shared__ PropTileLds lds;  // second pass
  const PropPass& P = F.base;
  const uint32_t tid = threadIdx.x, tile = blockIdx.x;
  const uint32_t h = tile * kPropTile + tid;  // host id
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(F.forces);
    uint32_t* dst = reinterpret_cast<uint32_t*>(forces);
    for (uint32_t k = tid; k < P.nProps * kForceWords; k += kPropTile) dst[k] = src[k];
  }
  __syncthreads();
  const bool live = h < P.nd.n;  // (no early return: every lane meets the barriers)
  uint32_t i = 0;
  V3 p{}, v{};
  float w = 0.0f, velW = 0.0f;
  bool movable = false, haveVel = false;
  if (live) {
    i = P.inv ? P.inv[h] : h;
    const float4 p4 = P.nd.pos[i];
    p = xyz(p4);
    w = p4.w;
    movable = !(w == 0.0f);
  }
  auto need_velocity = [&]() {
    if (haveVel) return;
    const float4 v4 = P.nd.vel[i];
    v = xyz(v4);
    velW = v4.w;
    haveVel = true;
  };
  // dv of force k on this lane's (movable) node from the state the call found; false: not affected
  auto evaluate = [&](uint32_t k, V3& dv) -> bool {
    const pies_force_t& f = forces[k];
    if (f.type == PIES_FORCE_WIND) {
      if (!kScratch) return false;  // (the host never launches the in-place variant with a wind)
      bool hit = false;
      const float g = F.dt * w;
      dv = V3{0.0f, 0.0f, 0.0f};
      for (uint32_t e = F.incPtr[h], end = F.incPtr[h + 1]; e < end; ++e) {
        const uint32_t* id = F.tri + 3ull * F.inc[e];
        const uint32_t ia = id[0], ib = id[1], ic = id[2];
        V3 n;
        float weight;
        if (!force_wind_face(f, xyz(P.nd.pos[ia]), xyz(P.nd.pos[ib]), xyz(P.nd.pos[ic]), n, weight)) continue;
        dv = add(dv, scale(force_wind_third(f, n, weight, xyz(P.nd.vel[ia]), xyz(P.nd.vel[ib]), xyz(P.nd.vel[ic])), g));
        hit = true;
      }
      if (hit) need_velocity();
      return hit;
    }
    V3 d;
    float dd, fall;
    if (!force_region(f, p, d, dd, fall)) return false;
    need_velocity();
    return force_point(f, F.dt, d, dd, fall, v, w, dv);
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

  // ---- second pass: the tile's set of forces and its sums (prop_tile_sums.h) ----
  prop_tile_sums(lds, P.tileMask, P.tileSums, P.nProps, affectedBy, [&](uint32_t k, PropTouch& T) {
    V3 dv{};
    (void)evaluate(k, dv);  // the change of the first pass, once more
    T.impulse = scale(dv, 1.0f / w);
    T.torque = cross(sub(p, load3(forces[k].centre)), T.impulse);
  });
}

__global__ void __launch_bounds__(kPropTile) k_force_commit(NodeArrays nd, const uint32_t* __restrict__ inv,
                                                            const float4* __restrict__ newVel, const uint64_t* __restrict__ affected) {
  const uint32_t h = blockIdx.x * kPropTile + threadIdx.x;  // host id
  if (h >= nd.n) return;
  if (!((affected[h >> 6] >> (h & 63u)) & 1ull)) return;
  nd.vel[inv ? inv[h] : h] = newVel[h];
}

bool launchable(const ForcePass& P) {
  return P.base.nd.n && P.base.nProps && P.base.nProps <= PIES_FORCE_MAX && P.forces;
}

}  // namespace

void launch_force_evaluate(hipStream_t st, const ForcePass& P) {
  if (!launchable(P)) return;
  const dim3 grid(prop_tiles(P.base.nd.n)), block(kPropTile);
  if (P.newVel) hipLaunchKernelGGL(k_force_evaluate<true>, grid, block, 0, st, P);
  else hipLaunchKernelGGL(k_force_evaluate<false>, grid, block, 0, st, P);
}

void launch_force_commit(hipStream_t st, const ForcePass& P) {
  if (!launchable(P) || !P.newVel) return;
  launch_velocity_commit(st, P.base.nd, P.base.inv, P.newVel, P.affected);
}

void launch_velocity_commit(hipStream_t st, const NodeArrays& nd, const uint32_t* inv, const float4* newVel, const uint64_t* affected) {
  if (!nd.n) return;
  hipLaunchKernelGGL(k_force_commit, dim3(prop_tiles(nd.n)), dim3(kPropTile), 0, st, nd, inv, newVel, affected);
}

}  // namespace pies
