// Signed distance fields and field props (extensions, pies_hip.h): pies_add_field, pies_add_field_tri_mesh, pies_get_field and
// pies_collide_field_props.  Host side only: argument checks, the host copy of every field (pies_solver::h_fields), the device
// copies and records (RayBuffers, solver_state.h) and the launches.  The mesh build runs pies_closest_points' own distance and
// winding launches (near_launch, nearest.cpp) on lattice points generated on the device; the collision is k_field_collide
// (field_kernels.h) between the open and close steps of a prop pass (props.cpp).  Nothing here touches the captured substep.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "capi_internal.h"
#include "field_kernels.h"

using namespace pies;

namespace {

// nullptr, or what is wrong with the record
const char* field_prop_fault(const pies_solver* s, const pies_field_prop_t& p) {
  if (p.field >= s->h_fields.size()) return "unknown field id";
  if (!(p.radius >= 0.0f) || !std::isfinite(p.radius)) return "radius must be finite and >= 0";
  if (!(p.friction >= 0.0f && p.friction <= 1.0f)) return "friction must be in [0, 1]";
  if (!finite_all(p.centre, 3) || !finite_all(p.axes, 9) || !finite_all(p.velocity, 3) || !finite_all(p.angular, 3) ||
      !finite_all(p.pivot, 3))
    return "centre, axes, velocity, angular and pivot must be finite";
  return nullptr;
}

// PIES_OK and the sample count, or why a lattice cannot be a field
int check_lattice(pies_solver* s, const char* who, const uint32_t dims[3], uint32_t* samples) {
  if (dims[0] < 2 || dims[1] < 2 || dims[2] < 2) return fail(s, PIES_ERR_INVALID, std::string(who) + ": every lattice dimension must be at least 2");
  uint64_t n = static_cast<uint64_t>(dims[0]) * dims[1];  // (< 2^64)
  n = n > kFieldMaxSamples ? n : n * dims[2];
  if (n > kFieldMaxSamples) return fail(s, PIES_ERR_UNSUPPORTED, std::string(who) + ": more than 2^24 lattice samples");
  if (s->h_fields.size() >= PIES_FIELD_MAX) return fail(s, PIES_ERR_UNSUPPORTED, std::string(who) + ": more than PIES_FIELD_MAX (64) fields");
  *samples = static_cast<uint32_t>(n);
  return PIES_OK;
}

// The device copy of field `id`, staged from the host copy when the handle holds none (the first use, or after free_device).
int stage_field(pies_solver* s, uint32_t id, const float** out) {
  RayBuffers& B = s->ray;
  if (!B.fieldSamples[id]) {
    const std::vector<float>& h = s->h_fields[id].samples;
    float* d = nullptr;
    if (int rc = ray_grow(s, h.size(), &d)) return rc;
    HIP_TRY(s, hipMemcpyAsync(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, s->stream));  // (h outlives the call)
    B.fieldSamples[id] = d;
  }
  *out = B.fieldSamples[id];
  return PIES_OK;
}

}  // namespace

extern "C" {

int pies_add_field(pies_solver_t* s, const uint32_t dims[3], const float origin[3], float cell, const float* samples, uint32_t* field) {
  if (!s) return PIES_ERR_INVALID;
  if (!dims || !origin || !samples) return fail(s, PIES_ERR_INVALID, "pies_add_field: dims, origin or samples is NULL");
  if (!(cell > 0.0f) || !std::isfinite(cell) || !finite_all(origin, 3))
    return fail(s, PIES_ERR_INVALID, "pies_add_field: cell must be finite and > 0, origin finite");
  uint32_t n = 0;
  if (int rc = check_lattice(s, "pies_add_field", dims, &n)) return rc;
  HostField f{{dims[0], dims[1], dims[2]}, {origin[0], origin[1], origin[2]}, cell, std::vector<float>(samples, samples + n)};
  if (field) *field = static_cast<uint32_t>(s->h_fields.size());
  s->h_fields.push_back(std::move(f));
  return PIES_OK;
}

int pies_add_field_tri_mesh(pies_solver_t* s, uint32_t n_vertices, const float* positions, uint32_t n_triangles,
                            const uint32_t* tri_ids, float cell, float margin, uint32_t* field) {
  if (!s) return PIES_ERR_INVALID;
  const std::string who = "pies_add_field_tri_mesh: ";
  if (!positions || n_vertices == 0) return fail(s, PIES_ERR_INVALID, who + "no vertices");
  if (!tri_ids || n_triangles == 0) return fail(s, PIES_ERR_INVALID, who + "no triangles");
  if (n_triangles > kFieldMaxTriangles) return fail(s, PIES_ERR_UNSUPPORTED, who + "more than 2^24 triangles");
  for (size_t i = 0; i < 3ull * n_triangles; ++i)
    if (tri_ids[i] >= n_vertices) return fail(s, PIES_ERR_INVALID, who + "triangle index out of range");
  if (!finite_all(positions, 3ull * n_vertices)) return fail(s, PIES_ERR_INVALID, who + "non-finite vertex");
  if (!(cell > 0.0f) || !std::isfinite(cell)) return fail(s, PIES_ERR_INVALID, who + "cell must be finite and > 0");
  if (!(margin >= 0.0f) || !std::isfinite(margin)) return fail(s, PIES_ERR_INVALID, who + "margin must be finite and >= 0");

  // ---- the lattice, in fp32 ----
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t v = 0; v < n_vertices; ++v)
    for (int j = 0; j < 3; ++j) {
      lo[j] = std::min(lo[j], positions[3ull * v + j]);
      hi[j] = std::max(hi[j], positions[3ull * v + j]);
    }
  HostField f{};
  f.cell = cell;
  for (int j = 0; j < 3; ++j) {
    f.origin[j] = lo[j] - margin;
    const float top = hi[j] + margin;
    const float cells = std::ceil((top - f.origin[j]) / cell);
    if (!std::isfinite(f.origin[j]) || !(cells < static_cast<float>(kFieldMaxSamples)))  // (an overflow, or a lattice beyond the limit)
      return fail(s, PIES_ERR_UNSUPPORTED, who + "more than 2^24 lattice samples");
    f.dims[j] = std::max(2u, static_cast<uint32_t>(cells) + 1u);
  }
  uint32_t n = 0;
  if (int rc = check_lattice(s, "pies_add_field_tri_mesh", f.dims, &n)) return rc;
  if (s->device == PIES_DEVICE_NONE)
    return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): a field is built from a mesh on the device");

  // ---- the build: the mesh as a RayTarget over temporaries, lattice points, distance and winding, samples ----
  HIP_TRY(s, hipSetDevice(s->device));
  const uint32_t id = static_cast<uint32_t>(s->h_fields.size());
  float* dSamples = nullptr;
  if (int rc = ray_grow(s, n, &dSamples)) return rc;  // the field's device copy, if all goes well
  s->ray.fieldSamples[id] = dSamples;                  // (a failure below leaves it unused until ray_free_device frees it)
  {
    Temporaries scope(s);
    float *dPos = nullptr, *dPoints = nullptr, *dDistance = nullptr, *dWinding = nullptr;
    uint32_t* dTri = nullptr;
    int rc = upload(s, std::vector<float>(positions, positions + 3ull * n_vertices), &dPos);
    if (!rc) rc = upload(s, std::vector<uint32_t>(tri_ids, tri_ids + 3ull * n_triangles), &dTri);
    if (!rc) rc = dev_alloc(s, 3ull * n, &dPoints);
    if (!rc) rc = dev_alloc(s, n, &dDistance);
    if (!rc) rc = dev_alloc(s, n, &dWinding);
    if (!rc) {
      const RayTarget T{dPos, 3, dTri, n_triangles};
      launch_field_points(s->stream, f.origin, f.cell, f.dims, dPoints);
      rc = near_launch(s, T, dPoints, n, INFINITY, nullptr, dDistance, nullptr, nullptr, dWinding);
      if (!rc) launch_field_combine(s->stream, n, dDistance, dWinding, dSamples);
    }
    f.samples.resize(n);
    if (!rc && hipGetLastError() != hipSuccess) rc = fail(s, PIES_ERR_HIP, who + "a launch failed");
    if (!rc && hipMemcpyAsync(f.samples.data(), dSamples, n * sizeof(float), hipMemcpyDeviceToHost, s->stream) != hipSuccess)
      rc = fail(s, PIES_ERR_HIP, who + "the copy of the samples failed");
    if (!rc && hipStreamSynchronize(s->stream) != hipSuccess) rc = fail(s, PIES_ERR_HIP, who + "the build failed on the device");
    if (rc) {
      s->ray.fieldSamples[id] = nullptr;
      return rc;
    }
  }
  if (field) *field = id;
  s->h_fields.push_back(std::move(f));
  return PIES_OK;
}

int pies_get_field(pies_solver_t* s, uint32_t field, uint32_t dims[3], float origin[3], float* cell, float* samples, uint64_t capacity) {
  if (!s) return PIES_ERR_INVALID;
  if (field >= s->h_fields.size()) return fail(s, PIES_ERR_INVALID, "pies_get_field: unknown field id");
  const HostField& f = s->h_fields[field];
  if (samples && capacity < f.samples.size()) return fail(s, PIES_ERR_INVALID, "pies_get_field: capacity is below the field's sample count");
  if (dims) std::memcpy(dims, f.dims, sizeof(f.dims));
  if (origin) std::memcpy(origin, f.origin, sizeof(f.origin));
  if (cell) *cell = f.cell;
  if (samples) std::memcpy(samples, f.samples.data(), f.samples.size() * sizeof(float));
  return PIES_OK;
}

int pies_collide_field_props(pies_solver_t* s, uint32_t n_props, const pies_field_prop_t* props, float* out_impulse,
                             float* out_torque, uint32_t* out_hits, uint32_t* out_node_prop) {
  if (!s) return PIES_ERR_INVALID;
  if (int rc = edit_prelude(s, {"pies_collide_field_props", "prop", "field props", PIES_FIELD_PROP_MAX, "PIES_FIELD_PROP_MAX"},
                            n_props, props, [&](uint32_t k) { return field_prop_fault(s, props[k]); }, nullptr, false,
                            {out_impulse, out_torque, out_hits, out_node_prop});
      rc != kEditGo)
    return rc;
  const bool reaction = out_impulse || out_torque || out_hits;

  FieldPass P;
  if (int rc = prop_open_pass(s, n_props, reaction, out_node_prop != nullptr, &P.base)) return rc;
  RayBuffers& B = s->ray;
  if (!B.fieldRecords)
    if (int rc = ray_grow(s, PIES_FIELD_PROP_MAX, &B.fieldRecords)) return rc;
  FieldPropRecord records[PIES_FIELD_PROP_MAX];
  std::memset(records, 0, n_props * sizeof(FieldPropRecord));
  for (uint32_t k = 0; k < n_props; ++k) {
    const pies_field_prop_t& p = props[k];
    const HostField& f = s->h_fields[p.field];
    FieldPropRecord& r = records[k];
    r.prop.radius = p.radius;
    r.prop.friction = p.friction;
    std::memcpy(r.prop.centre, p.centre, sizeof(p.centre));
    std::memcpy(r.prop.axes, p.axes, sizeof(p.axes));
    std::memcpy(r.prop.velocity, p.velocity, sizeof(p.velocity));
    std::memcpy(r.prop.angular, p.angular, sizeof(p.angular));
    std::memcpy(r.prop.pivot, p.pivot, sizeof(p.pivot));
    std::memcpy(r.origin, f.origin, sizeof(f.origin));
    std::memcpy(r.dims, f.dims, sizeof(f.dims));
    r.cell = f.cell;
    if (int rc = stage_field(s, p.field, &r.samples)) return rc;
  }
  HIP_TRY(s, hipMemcpyAsync(B.fieldRecords, records, n_props * sizeof(FieldPropRecord), hipMemcpyHostToDevice, s->stream));
  P.records = B.fieldRecords;
  launch_field_collide(s->stream, P);
  return prop_close_pass(s, P.base, out_impulse, out_torque, out_hits, out_node_prop);  // (synchronises: `records` may die)
}

}  // extern "C"
