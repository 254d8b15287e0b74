// pies_apply_forces (an extension, pies_hip.h): wind, blasts and attractors, vortices, drag and plain pushes change the velocities
// where HBM holds them and hand back the reaction per force.  Host side only: argument checks, the buffers (RayBuffers,
// solver_state.h), the choice of the variant and the launches (force_kernels.h) between the open and close steps of a prop pass
// (props.cpp).  The edit goes to dev.nd.vel outside the captured substep: no graph, no schedule and no launch count changes.
#include <cmath>

#include "capi_internal.h"
#include "force_kernels.h"

using namespace pies;

namespace {

// nullptr, or what is wrong with the record
const char* force_fault(const pies_force_t& f) {
  if (f.type < PIES_FORCE_DIRECTIONAL || f.type > PIES_FORCE_WIND) return "unknown type";
  if (f.falloff != PIES_FALLOFF_NONE && f.falloff != PIES_FALLOFF_LINEAR && f.falloff != PIES_FALLOFF_SMOOTH) return "unknown falloff";
  if (!(f.radius >= 0.0f)) return "radius must be >= 0 (+inf: everywhere)";
  if (!finite_all(f.centre, 3) || !finite_all(f.vector, 3) || !std::isfinite(f.strength) || !std::isfinite(f.shear))
    return "centre, vector, strength and shear must be finite";
  return nullptr;
}

}  // namespace

extern "C" {

int pies_apply_forces(pies_solver_t* s, uint32_t n_forces, const pies_force_t* forces, float dt, float* out_impulse,
                      float* out_torque, uint32_t* out_nodes) {
  if (!s) return PIES_ERR_INVALID;
  if (int rc = edit_prelude(s, {"pies_apply_forces", "force", "forces", PIES_FORCE_MAX, "PIES_FORCE_MAX"}, n_forces, forces,
                            [&](uint32_t k) { return force_fault(forces[k]); }, &dt, false, {out_impulse, out_torque, out_nodes});
      rc != kEditGo)
    return rc;
  const bool reaction = out_impulse || out_torque || out_nodes;

  // ---- the variant: a wind reads its neighbours' velocities, so its list goes through the scratch array ----
  bool wind = false;
  for (uint32_t k = 0; k < n_forces; ++k) wind = wind || forces[k].type == PIES_FORCE_WIND;
  bool scratch = wind;
  if (int rc = edit_variant(s, "PIES_FORCE_VARIANT", "pies_apply_forces", &scratch)) return rc;

  ForcePass P;
  if (int rc = prop_open_pass(s, n_forces, reaction, false, &P.base)) return rc;
  RayBuffers& B = s->ray;
  if (!B.forceRecords)
    if (int rc = ray_grow(s, PIES_FORCE_MAX, &B.forceRecords)) return rc;
  if (scratch)
    if (int rc = edit_velocity_scratch(s, &P.scratch)) return rc;
  if (wind) {
    RayTarget T;
    if (int rc = ray_open_target(s, PIES_RAY_SCENE_TRIANGLES, 0, &T)) return rc;
    if (int rc = ray_build_incidence(s)) return rc;
    P.surface = SurfaceIncidence{T.tri, T.nTris, B.incPtr, B.inc};
  }
  HIP_TRY(s, hipMemcpyAsync(B.forceRecords, forces, n_forces * sizeof(pies_force_t), hipMemcpyHostToDevice, s->stream));
  P.forces = B.forceRecords;
  P.dt = dt;
  launch_force_evaluate(s->stream, P);
  launch_velocity_commit(s->stream, P.base.nd, P.base.inv, P.scratch);
  return prop_close_pass(s, P.base, out_impulse, out_torque, out_nodes, nullptr, 4u);  // (the velocities alone are stale)
}

}  // extern "C"
