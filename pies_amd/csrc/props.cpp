// pies_collide_props (an extension, pies_hip.h): kinematic spheres, capsules and rounded boxes push the nodes out where HBM holds
// them and hand back the reaction per prop.  Host side only: argument checks, the buffers (RayBuffers, solver_state.h) and the two
// launches (prop_kernels.h).  The edit goes to dev.nd.pos / prev / vel - the state every schedule and both solvers start a substep
// from - outside the captured substep: no graph, no schedule and no launch count changes.
// What every between-tick edit of node state shares on the host lives here too, for fields.cpp, forces.cpp
// and loads.cpp: edit_prelude - the argument checks, the empty list, the host-only handle and the empty scene -, prop_open_pass /
// prop_close_pass - the reaction's buffers, the fold, the stale marks and the copies out -, and edit_variant and
// edit_velocity_scratch of the two velocity edits.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "capi_internal.h"
#include "force_kernels.h"

using namespace pies;

namespace {

// nullptr, or what is wrong with the record
const char* prop_fault(const pies_prop_t& p) {
  if (p.shape != PIES_PROP_SPHERE && p.shape != PIES_PROP_CAPSULE && p.shape != PIES_PROP_BOX) return "unknown shape";
  if (!(p.radius >= 0.0f) || !std::isfinite(p.radius)) return "radius must be finite and >= 0";
  if (!(p.friction >= 0.0f && p.friction <= 1.0f)) return "friction must be in [0, 1]";
  if (!finite_all(p.centre, 3) || !finite_all(p.velocity, 3) || !finite_all(p.angular, 3) || !finite_all(p.pivot, 3))
    return "centre, velocity, angular and pivot must be finite";
  if (p.shape == PIES_PROP_CAPSULE && !finite_all(p.end, 3)) return "a capsule's end must be finite";
  if (p.shape == PIES_PROP_BOX) {
    if (!finite_all(p.axes, 9)) return "a box's axes must be finite";
    for (int j = 0; j < 3; ++j)
      if (!(p.half[j] >= 0.0f) || !std::isfinite(p.half[j])) return "a box's half extents must be finite and >= 0";
  }
  return nullptr;
}

}  // namespace

namespace pies {

int edit_prelude_checked(pies_solver* s, const EditNames& N, uint32_t count, const void* records, uint32_t bad, const char* what,
                         const float* dt, bool idle, const EditOutputs& out) {
  const auto who = [&] { return std::string(N.call) + ": "; };  // (messages are built on the failure paths only)
  if (count && !records) return fail(s, PIES_ERR_INVALID, who() + N.noun + "s is NULL");
  if (count > N.max)
    return fail(s, PIES_ERR_UNSUPPORTED, who() + "more than " + N.maxName + " (" + std::to_string(N.max) + ") " + N.noun + "s");
  if (what) return fail(s, PIES_ERR_INVALID, who() + N.noun + " " + std::to_string(bad) + ": " + what);
  if (dt && (!(*dt >= 0.0f) || !std::isfinite(*dt))) return fail(s, PIES_ERR_INVALID, who() + "dt must be finite and >= 0");
  if (count == 0) {
    if (out.nodeProp) std::fill(out.nodeProp, out.nodeProp + s->nodeCount(), PIES_PROP_NONE);
    return PIES_OK;
  }
  if (s->device == PIES_DEVICE_NONE)
    return fail(s, PIES_ERR_HIP, std::string("host-only handle (PIES_DEVICE_NONE): ") + N.subject + " meet the nodes on the device");
  if (int rc = pies_internal_ensure_ready(s)) return rc;
  if (s->dev.nd.n == 0 || idle) {  // nothing to edit: the call still waits for the queued work
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    if (out.impulse) std::fill(out.impulse, out.impulse + 3ull * count, 0.0f);
    if (out.torque) std::fill(out.torque, out.torque + 3ull * count, 0.0f);
    if (out.counts) std::fill(out.counts, out.counts + count, 0u);
    if (out.volume) std::fill(out.volume, out.volume + count, 0.0f);
    if (out.area) std::fill(out.area, out.area + count, 0.0f);
    return PIES_OK;
  }
  return kEditGo;
}

int edit_variant(pies_solver* s, const char* variable, const char* call, bool* scratch) {
  const char* e = tuning_env(variable);
  if (!e || std::strcmp(e, "inplace") == 0) return PIES_OK;
  if (std::strcmp(e, "scratch") != 0) return fail(s, PIES_ERR_INVALID, std::string(call) + ": " + variable + " must be inplace or scratch");
  *scratch = true;
  return PIES_OK;
}

int edit_velocity_scratch(pies_solver* s, VelocityScratch* out) {
  RayBuffers& B = s->ray;
  const uint32_t n = s->dev.nd.n;
  if (B.forceVelCap < n) {  // (two buffers under one capacity)
    B.forceVelCap = 0;
    if (int rc = ray_grow(s, n, &B.forceVel)) return rc;
    if (int rc = ray_grow(s, static_cast<size_t>(prop_tiles(n)) * kForceWaves, &B.forceAffected)) return rc;
    B.forceVelCap = n;
  }
  *out = VelocityScratch{B.forceVel, B.forceAffected};
  return PIES_OK;
}

// The part of a pass over the nodes that does not depend on what the props are: node arrays, numbering and the reaction's buffers.
int prop_open_pass(pies_solver* s, uint32_t nProps, bool reaction, bool nodeProp, PropPass* out) {
  RayBuffers& B = s->ray;
  const uint32_t n = s->dev.nd.n, tiles = prop_tiles(n);
  if (!B.propOut)
    if (int rc = ray_grow(s, static_cast<size_t>(PIES_PROP_MAX) * kPropSumWords, &B.propOut)) return rc;
  if (reaction) {
    if (int rc = ray_reserve(s, tiles, &B.propTileMask, &B.propTileCap)) return rc;
    if (int rc = ray_reserve(s, static_cast<size_t>(tiles) * nProps, &B.propTileSums, &B.propSumCap, kPropSumWords)) return rc;
  }
  if (nodeProp)
    if (int rc = ray_reserve(s, n, &B.propNodeProp, &B.propNodeCap)) return rc;
  PropPass P;
  P.nd = s->dev.nd;
  P.inv = s->dev.d_nodeInv;
  P.nProps = nProps;
  P.tileMask = reaction ? B.propTileMask : nullptr;
  P.tileSums = reaction ? B.propTileSums : nullptr;
  P.nodeProp = nodeProp ? B.propNodeProp : nullptr;
  *out = P;
  return PIES_OK;
}

// After the collide launch of pass P: the fold, the stale marks (staleBits: the node arrays the launch edited), the copies out and
// the synchronisation.
int prop_close_pass(pies_solver* s, const PropPass& P, float* out_impulse, float* out_torque, uint32_t* out_hits, uint32_t* out_node_prop,
                    uint32_t staleBits) {
  RayBuffers& B = s->ray;
  const bool reaction = P.tileMask != nullptr;
  const uint32_t n = P.nd.n, n_props = P.nProps;
  if (reaction) launch_prop_fold(s->stream, P, B.propOut);
  HIP_TRY(s, hipGetLastError());
  s->stale |= staleBits;  // the props' 7: positions, previous positions and velocities - the host mirror is older than HBM (nothing is uploaded)
  float folded[PIES_PROP_MAX * kPropSumWords];
  if (reaction) HIP_TRY(s, hipMemcpyAsync(folded, B.propOut, n_props * kPropSumWords * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  if (out_node_prop) HIP_TRY(s, hipMemcpyAsync(out_node_prop, B.propNodeProp, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  for (uint32_t k = 0; reaction && k < n_props; ++k) {
    const float* f = folded + k * kPropSumWords;
    if (out_impulse) std::memcpy(out_impulse + 3ull * k, f, 3 * sizeof(float));
    if (out_torque) std::memcpy(out_torque + 3ull * k, f + 3, 3 * sizeof(float));
    if (out_hits) std::memcpy(out_hits + k, f + 6, sizeof(uint32_t));
  }
  return PIES_OK;
}

}  // namespace pies

extern "C" {

int pies_collide_props(pies_solver_t* s, uint32_t n_props, const pies_prop_t* props, float* out_impulse, float* out_torque,
                       uint32_t* out_hits, uint32_t* out_node_prop) {
  if (!s) return PIES_ERR_INVALID;
  if (int rc = edit_prelude(s, {"pies_collide_props", "prop", "props", PIES_PROP_MAX, "PIES_PROP_MAX"}, n_props, props,
                            [&](uint32_t k) { return prop_fault(props[k]); }, nullptr, false,
                            {out_impulse, out_torque, out_hits, out_node_prop});
      rc != kEditGo)
    return rc;
  const bool reaction = out_impulse || out_torque || out_hits;

  PropPass P;
  if (int rc = prop_open_pass(s, n_props, reaction, out_node_prop != nullptr, &P)) return rc;
  RayBuffers& B = s->ray;
  if (!B.propRecords)
    if (int rc = ray_grow(s, PIES_PROP_MAX, &B.propRecords)) return rc;
  HIP_TRY(s, hipMemcpyAsync(B.propRecords, props, n_props * sizeof(pies_prop_t), hipMemcpyHostToDevice, s->stream));
  P.props = B.propRecords;
  launch_prop_collide(s->stream, P);
  return prop_close_pass(s, P, out_impulse, out_torque, out_hits, out_node_prop);
}

}  // extern "C"
