// Force fields (force_kernels.h; the rule is stated in pies_hip.h, lives in force_rule.h and is restated in numpy by
// tests/test_forces.py).
//  k_force_evaluate  a velocity edit (node_edit_device.h: velocity_edit_pass; the records are at most 64 x 48 bytes).  What is
//                    particular: a node in no region pays its position only, the velocity is read at the first force whose
//                    region holds the node.  A wind walks the node's row of the incidence (by host id, ascending triangle
//                    index): per entry the triangle's three positions, and only for a triangle that contributes its three
//                    velocities - the same F on the same operands in every lane that shares the triangle, no atomics and no
//                    per-triangle buffer.  A list with a wind takes the scratch variant; without one no lane reads another
//                    node's velocity and the new velocity is stored in place.
//  k_force_commit    the scratch variant's second launch: one lane per host id reads its wave's word of `affected` (one broadcast)
//                    and, when its bit is set, moves newVel[host id] to the node's velocity.
// Built with -ffp-contract=off like the rest of the library: the arithmetic is the IEEE sequence written in force_rule.h.
#include "force_kernels.h"

#include "force_rule.h"
#include "node_edit_device.h"

namespace pies {
namespace {

static_assert(sizeof(pies_force_t) == 48, "pies_force_t is 12 words without padding");
static_assert(PIES_FORCE_MAX <= PIES_PROP_MAX, "the reaction's buffers and the 64-bit tile word are the props'");

template <bool kScratch>
__global__ void __launch_bounds__(kPropTile) k_force_evaluate(ForcePass F) {
  __shared__ pies_force_t forces[PIES_FORCE_MAX];
  __shared__ PropTileLds lds;  // second pass
  const PropPass& P = F.base;
  stage_records(forces, F.forces, P.nProps);
  __syncthreads();
  EditLane lane = edit_lane(P);
  // dv of force k on this lane's (movable) node from the state the call found; false: not affected
  auto evaluate = [&](uint32_t k, V3& dv) -> bool {
    const pies_force_t& f = forces[k];
    if (f.type == PIES_FORCE_WIND) {
      if (!kScratch) return false;  // (the host never launches the in-place variant with a wind)
      bool hit = false;
      const float g = F.dt * lane.w;
      dv = V3{0.0f, 0.0f, 0.0f};
      for (uint32_t e = F.surface.incPtr[lane.h], end = F.surface.incPtr[lane.h + 1]; e < end; ++e) {
        const uint32_t* id = F.surface.tri + 3ull * F.surface.inc[e];
        const uint32_t ia = id[0], ib = id[1], ic = id[2];
        V3 n;
        float weight;
        if (!force_wind_face(f, xyz(P.nd.pos[ia]), xyz(P.nd.pos[ib]), xyz(P.nd.pos[ic]), n, weight)) continue;
        dv = add(dv, scale(force_wind_third(f, n, weight, xyz(P.nd.vel[ia]), xyz(P.nd.vel[ib]), xyz(P.nd.vel[ic])), g));
        hit = true;
      }
      if (hit) need_velocity(P, lane);
      return hit;
    }
    V3 d;
    float dd, fall;
    if (!force_region(f, lane.p, d, dd, fall)) return false;
    need_velocity(P, lane);
    return force_point(f, F.dt, d, dd, fall, lane.v, lane.w, dv);
  };
  velocity_edit_pass<kScratch>(P, F.scratch, lds, lane, evaluate, [&](uint32_t k) { return load3(forces[k].centre); });
}

__global__ void __launch_bounds__(kPropTile) k_force_commit(NodeArrays nd, const uint32_t* __restrict__ inv,
                                                            const float4* __restrict__ newVel, const uint64_t* __restrict__ affected) {
  const uint32_t h = blockIdx.x * kPropTile + threadIdx.x;  // host id
  if (h >= nd.n) return;
  if (!((affected[h >> 6] >> (h & 63u)) & 1ull)) return;
  nd.vel[inv ? inv[h] : h] = newVel[h];
}

}  // namespace

void launch_force_evaluate(hipStream_t st, const ForcePass& P) {
  if (!P.base.nd.n || !P.base.nProps || P.base.nProps > PIES_FORCE_MAX || !P.forces) return;
  const dim3 grid(prop_tiles(P.base.nd.n)), block(kPropTile);
  if (P.scratch.newVel) hipLaunchKernelGGL(k_force_evaluate<true>, grid, block, 0, st, P);
  else hipLaunchKernelGGL(k_force_evaluate<false>, grid, block, 0, st, P);
}

void launch_velocity_commit(hipStream_t st, const NodeArrays& nd, const uint32_t* inv, const VelocityScratch& scratch) {
  if (!nd.n || !scratch.newVel) return;
  hipLaunchKernelGGL(k_force_commit, dim3(prop_tiles(nd.n)), dim3(kPropTile), 0, st, nd, inv, scratch.newVel, scratch.affected);
}

}  // namespace pies
