// pies_collide_props (an extension, pies_hip.h): kinematic spheres, capsules and rounded boxes push the nodes out where HBM holds
// them and hand back the reaction per prop.  Host side only: argument checks, the buffers (RayBuffers, solver_state.h) and the two
// launches (prop_kernels.h).  The edit goes to dev.nd.pos / prev / vel - the state every schedule and both solvers start a substep
// from - outside the captured substep: no graph, no schedule and no launch count changes.
// prop_open_pass / prop_close_pass - the reaction's buffers, the fold, the stale marks and the copies out - are shared with
// pies_collide_field_props (fields.cpp) and pies_apply_forces (forces.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "capi_internal.h"
#include "prop_kernels.h"

using namespace pies;

namespace {

bool finite_all(const float* v, int n) {
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

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

// The part of a pass over the nodes that does not depend on what the props are: node arrays, numbering and the reaction's buffers.
int prop_open_pass(pies_solver* s, uint32_t nProps, bool reaction, bool nodeProp, PropPass* out) {
  RayBuffers& B = s->ray;
  const uint32_t n = s->dev.nd.n, tiles = prop_tiles(n);
  if (!B.propOut)
    if (int rc = ray_grow(s, static_cast<size_t>(PIES_PROP_MAX) * kPropSumWords, &B.propOut)) return rc;
  if (reaction && B.propTileCap < tiles) {
    B.propTileCap = 0;
    if (int rc = ray_grow(s, tiles, &B.propTileMask)) return rc;
    B.propTileCap = tiles;
  }
  const size_t records = static_cast<size_t>(tiles) * nProps;
  if (reaction && B.propSumCap < records) {
    B.propSumCap = 0;
    if (int rc = ray_grow(s, records * kPropSumWords, &B.propTileSums)) return rc;
    B.propSumCap = records;
  }
  if (nodeProp && B.propNodeCap < n) {
    B.propNodeCap = 0;
    if (int rc = ray_grow(s, n, &B.propNodeProp)) return rc;
    B.propNodeCap = n;
  }
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
  if (n_props && !props) return fail(s, PIES_ERR_INVALID, "pies_collide_props: props is NULL");
  if (n_props > PIES_PROP_MAX) return fail(s, PIES_ERR_UNSUPPORTED, "pies_collide_props: more than PIES_PROP_MAX (64) props");
  for (uint32_t k = 0; k < n_props; ++k)
    if (const char* what = prop_fault(props[k]))
      return fail(s, PIES_ERR_INVALID, "pies_collide_props: prop " + std::to_string(k) + ": " + what);
  if (n_props == 0) {
    if (out_node_prop) std::fill(out_node_prop, out_node_prop + s->nodeCount(), PIES_PROP_NONE);
    return PIES_OK;
  }
  if (s->device == PIES_DEVICE_NONE)
    return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): props meet the nodes on the device");
  if (int rc = pies_internal_ensure_ready(s)) return rc;
  const uint32_t n = s->dev.nd.n;
  const bool reaction = out_impulse || out_torque || out_hits;
  if (n == 0) {  // no nodes: the call still waits for the queued work
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    if (out_impulse) std::fill(out_impulse, out_impulse + 3ull * n_props, 0.0f);
    if (out_torque) std::fill(out_torque, out_torque + 3ull * n_props, 0.0f);
    if (out_hits) std::fill(out_hits, out_hits + n_props, 0u);
    return PIES_OK;
  }

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
