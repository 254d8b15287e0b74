// pies_closest_points (an extension, pies_hip.h): the closest surface point and the winding number of query points against the
// scene's triangles or a skin's, at the positions the device holds.  Host side only: argument checks, the buffers (RayBuffers,
// solver_state.h: the triangle list, the staged records and the partial keys are pies_raycast's), the choice of the kernel variant
// and the launches (near_kernels.h).  Nothing here touches the substep: no captured graph, no schedule, no node state.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "capi_internal.h"
#include "near_kernels.h"

using namespace pies;

namespace {

constexpr size_t kNearBatchBytes = 128ull << 20;  // partial keys, or tile sums, of one batch of points at most
// measured on BASELINE config 3's beam surface: narrow no slower at every point count of the sweep, which ends at 4 096
constexpr uint32_t kNearNarrowMaxDefault = 4096;
constexpr uint32_t kNearWorkgroupsWanted = 1024;  // wide variant: point blocks x chunks to aim for (4 workgroups per CU)

int no_candidates(uint32_t n, const float* points, uint32_t* outTriangle, float* outDistance, float* outUv, float* outPoint, float* outWinding) {
  for (uint32_t i = 0; i < n; ++i) {
    if (outTriangle) outTriangle[i] = PIES_NEAR_NONE;
    if (outDistance) outDistance[i] = INFINITY;
    if (outUv) outUv[2ull * i] = outUv[2ull * i + 1] = 0.0f;
    if (outWinding) outWinding[i] = 0.0f;
  }
  if (outPoint) std::memcpy(outPoint, points, 3ull * n * sizeof(float));
  return PIES_OK;
}

}  // namespace

namespace pies {

// The distance pass (any of dTri, dDistance, dUv, dPoint) and the winding pass (dWinding) of n points in HBM against target T: the
// choice of the kernel variant, the shared buffers of s->ray (staged records, partial keys / tile sums) and the launches, batch
// after batch on the handle's stream.  No synchronisation.  Shared with fields.cpp, whose lattice points never leave the device.
int near_launch(pies_solver* s, const RayTarget& T, const float* dPoints, uint32_t n_points, float max_distance, uint32_t* dTri,
                float* dDistance, float* dUv, float* dPoint, float* dWinding) {
  RayBuffers& B = s->ray;
  const bool distancePass = dTri || dDistance || dUv || dPoint;
  if (!n_points || !T.nTris || (!distancePass && !dWinding)) return PIES_OK;

  // ---- the variant of the distance pass ----
  bool narrow = n_points <= kNearNarrowMaxDefault;
  if (const char* e = tuning_env("PIES_NEAR_NARROW_MAX")) narrow = n_points <= static_cast<uint32_t>(std::max(0l, std::atol(e)));
  if (const char* e = tuning_env("PIES_NEAR_VARIANT")) {
    if (std::strcmp(e, "wide") == 0) narrow = false;
    else if (std::strcmp(e, "narrow") == 0) narrow = true;
    else return fail(s, PIES_ERR_INVALID, "pies_closest_points: PIES_NEAR_VARIANT must be wide or narrow");
  }
  const uint32_t nTiles = near_tiles(T.nTris);
  uint32_t parts;
  if (narrow) {
    parts = ray_narrow_parts(T.nTris);
  } else {
    const uint32_t pointBlocks = (n_points + kNearBlock - 1) / kNearBlock;
    parts = std::min(nTiles, std::max(1u, kNearWorkgroupsWanted / pointBlocks));
    if (const char* e = tuning_env("PIES_NEAR_CHUNKS")) {
      const long v = std::atol(e);
      if (v < 1 || v > static_cast<long>(kNearMaxChunks)) return fail(s, PIES_ERR_INVALID, "pies_closest_points: PIES_NEAR_CHUNKS must be 1 .. 1024");
      parts = static_cast<uint32_t>(v);  // (chunks beyond the last tile are empty: no candidate)
    }
  }
  // points per batch: a multiple of the workgroup, its partial keys (8 bytes per part) and its tile sums (4 bytes per tile) bounded
  const size_t perPoint = std::max<size_t>(distancePass ? sizeof(uint64_t) * parts : 0, dWinding ? sizeof(float) * nTiles : 0);
  const uint32_t batch = static_cast<uint32_t>(
      std::min<uint64_t>(n_points, std::max<uint64_t>(kNearBlock, kNearBatchBytes / perPoint / kNearBlock * kNearBlock)));

  // ---- buffers ----
  const size_t keys = (static_cast<size_t>(batch) * perPoint + sizeof(uint64_t) - 1) / sizeof(uint64_t);
  if (int rc = ray_reserve(s, keys, &B.partial, &B.partialCap)) return rc;
  if (distancePass && !narrow)
    if (int rc = ray_reserve(s, T.nTris, &B.records, &B.recordCap, 3)) return rc;

  // ---- the launches: per batch the distance pass, then the winding pass (the stream orders their use of `partial`) ----
  if (distancePass && !narrow) launch_ray_stage(s->stream, T, B.records);
  for (uint32_t first = 0; first < n_points; first += batch) {
    NearBatch P;
    P.points = dPoints + 3ull * first;
    P.n = std::min(batch, n_points - first);
    P.maxDistance2 = max_distance * max_distance;
    if (distancePass) {
      if (narrow) launch_near_narrow(s->stream, T, P, B.partial);
      else launch_near_wide(s->stream, B.records, T.nTris, P, parts, B.partial);
      launch_near_resolve(s->stream, T, P, B.partial, parts, dTri ? dTri + first : nullptr, dDistance ? dDistance + first : nullptr,
                          dUv ? dUv + 2ull * first : nullptr, dPoint ? dPoint + 3ull * first : nullptr);
    }
    if (dWinding) launch_near_winding(s->stream, T, P, reinterpret_cast<float*>(B.partial), dWinding + first);
  }
  return PIES_OK;
}

}  // namespace pies

extern "C" {

int pies_closest_points(pies_solver_t* s, int target, uint32_t skin, uint32_t n_points, const float* points, float max_distance,
                        uint32_t* out_triangle, float* out_distance, float* out_uv, float* out_point, float* out_winding) {
  if (!s) return PIES_ERR_INVALID;
  if (n_points && !points) return fail(s, PIES_ERR_INVALID, "pies_closest_points: points is NULL");
  if (target != PIES_RAY_SCENE_TRIANGLES && target != PIES_RAY_SKIN) return fail(s, PIES_ERR_INVALID, "pies_closest_points: unknown target");
  if (target == PIES_RAY_SKIN && skin >= s->h_skins.size()) return fail(s, PIES_ERR_INVALID, "pies_closest_points: no such skin");
  if (!(max_distance >= 0.0f)) return fail(s, PIES_ERR_INVALID, "pies_closest_points: max_distance must be >= 0 (+inf is allowed)");
  if (n_points > kNearMaxPoints) return fail(s, PIES_ERR_UNSUPPORTED, "pies_closest_points: more than 2^26 points");
  if (n_points == 0) return PIES_OK;
  if (s->device == PIES_DEVICE_NONE)
    return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): closest points are evaluated on the device");
  if (int rc = pies_internal_ensure_ready(s)) return rc;
  RayBuffers& B = s->ray;
  RayTarget T;
  if (int rc = ray_open_target(s, target, skin, &T)) return rc;
  if (T.nTris == 0) {
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    return no_candidates(n_points, points, out_triangle, out_distance, out_uv, out_point, out_winding);
  }
  const bool distancePass = out_triangle || out_distance || out_uv || out_point;
  if (!distancePass && !out_winding) {  // nothing asked for: the call still waits for the queued ticks
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    return PIES_OK;
  }
  if (B.nearCap < n_points) {
    B.nearCap = 0;
    if (int rc = ray_grow(s, 3ull * n_points, &B.nearPoints)) return rc;
    if (int rc = ray_grow(s, n_points, &B.nearTri)) return rc;
    if (int rc = ray_grow(s, n_points, &B.nearDistance)) return rc;
    if (int rc = ray_grow(s, 2ull * n_points, &B.nearUv)) return rc;
    if (int rc = ray_grow(s, 3ull * n_points, &B.nearPoint)) return rc;
    if (int rc = ray_grow(s, n_points, &B.nearWinding)) return rc;
    B.nearCap = n_points;
  }
  HIP_TRY(s, hipMemcpyAsync(B.nearPoints, points, 3ull * n_points * sizeof(float), hipMemcpyHostToDevice, s->stream));
  if (int rc = near_launch(s, T, B.nearPoints, n_points, max_distance, distancePass ? B.nearTri : nullptr,
                           distancePass ? B.nearDistance : nullptr, distancePass ? B.nearUv : nullptr,
                           distancePass ? B.nearPoint : nullptr, out_winding ? B.nearWinding : nullptr))
    return rc;
  HIP_TRY(s, hipGetLastError());
  if (out_triangle) HIP_TRY(s, hipMemcpyAsync(out_triangle, B.nearTri, n_points * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
  if (out_distance) HIP_TRY(s, hipMemcpyAsync(out_distance, B.nearDistance, n_points * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  if (out_uv) HIP_TRY(s, hipMemcpyAsync(out_uv, B.nearUv, 2ull * n_points * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  if (out_point) HIP_TRY(s, hipMemcpyAsync(out_point, B.nearPoint, 3ull * n_points * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  if (out_winding) HIP_TRY(s, hipMemcpyAsync(out_winding, B.nearWinding, n_points * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return PIES_OK;
}

}  // extern "C"
