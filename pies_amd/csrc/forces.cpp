// pies_apply_forces (an extension, pies_hip.h): wind, blasts and attractors, vortices, drag and plain pushes change the velocities
// where HBM holds them and hand back the reaction per force.  Host side only: argument checks, the buffers (RayBuffers,
// solver_state.h), the choice of the variant and the launches (force_kernels.h) between the open and close steps of a prop pass
// (props.cpp).  The edit goes to dev.nd.vel outside the captured substep: no graph, no schedule and no launch count changes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "capi_internal.h"
#include "force_kernels.h"

using namespace pies;

namespace {

bool finite_all(const float* v, int n) {
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

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
  if (n_forces && !forces) return fail(s, PIES_ERR_INVALID, "pies_apply_forces: forces is NULL");
  if (n_forces > PIES_FORCE_MAX) return fail(s, PIES_ERR_UNSUPPORTED, "pies_apply_forces: more than PIES_FORCE_MAX (64) forces");
  for (uint32_t k = 0; k < n_forces; ++k)
    if (const char* what = force_fault(forces[k]))
      return fail(s, PIES_ERR_INVALID, "pies_apply_forces: force " + std::to_string(k) + ": " + what);
  if (!(dt >= 0.0f) || !std::isfinite(dt)) return fail(s, PIES_ERR_INVALID, "pies_apply_forces: dt must be finite and >= 0");
  if (n_forces == 0) return PIES_OK;
  if (s->device == PIES_DEVICE_NONE)
    return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): forces meet the nodes on the device");
  if (int rc = pies_internal_ensure_ready(s)) return rc;
  const uint32_t n = s->dev.nd.n;
  const bool reaction = out_impulse || out_torque || out_nodes;
  if (n == 0) {  // no nodes: the call still waits for the queued work
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    if (out_impulse) std::fill(out_impulse, out_impulse + 3ull * n_forces, 0.0f);
    if (out_torque) std::fill(out_torque, out_torque + 3ull * n_forces, 0.0f);
    if (out_nodes) std::fill(out_nodes, out_nodes + n_forces, 0u);
    return PIES_OK;
  }

  // ---- the variant: a wind reads its neighbours' velocities, so its list goes through the scratch array ----
  bool wind = false;
  for (uint32_t k = 0; k < n_forces; ++k) wind = wind || forces[k].type == PIES_FORCE_WIND;
  bool scratch = wind;
  if (const char* e = tuning_env("PIES_FORCE_VARIANT")) {
    if (std::strcmp(e, "scratch") == 0) scratch = true;
    else if (std::strcmp(e, "inplace") != 0) return fail(s, PIES_ERR_INVALID, "pies_apply_forces: PIES_FORCE_VARIANT must be inplace or scratch");
  }

  ForcePass P;
  if (int rc = prop_open_pass(s, n_forces, reaction, false, &P.base)) return rc;
  RayBuffers& B = s->ray;
  if (!B.forceRecords)
    if (int rc = ray_grow(s, PIES_FORCE_MAX, &B.forceRecords)) return rc;
  if (scratch && B.forceVelCap < n) {
    B.forceVelCap = 0;
    if (int rc = ray_grow(s, n, &B.forceVel)) return rc;
    if (int rc = ray_grow(s, static_cast<size_t>(prop_tiles(n)) * kForceWaves, &B.forceAffected)) return rc;
    B.forceVelCap = n;
  }
  if (wind) {
    RayTarget T;
    if (int rc = ray_open_target(s, PIES_RAY_SCENE_TRIANGLES, 0, &T)) return rc;
    if (int rc = ray_build_incidence(s)) return rc;
    P.tri = T.tri;
    P.incPtr = B.incPtr;
    P.inc = B.inc;
  }
  HIP_TRY(s, hipMemcpyAsync(B.forceRecords, forces, n_forces * sizeof(pies_force_t), hipMemcpyHostToDevice, s->stream));
  P.forces = B.forceRecords;
  P.dt = dt;
  if (scratch) {
    P.newVel = B.forceVel;
    P.affected = B.forceAffected;
  }
  launch_force_evaluate(s->stream, P);
  launch_force_commit(s->stream, P);
  return prop_close_pass(s, P.base, out_impulse, out_torque, out_nodes, nullptr, 4u);  // (the velocities alone are stale)
}

}  // extern "C"
