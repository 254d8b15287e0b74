// pies_raycast (an extension, pies_hip.h): rays against the scene's triangles or a skin's, at the positions the device holds.
// Host side only: argument checks, the lazily built buffers (RayBuffers, solver_state.h), the choice of the kernel variant and
// the launches (ray_kernels.h).  Nothing here touches the substep: no captured graph, no schedule, no node state.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "capi_internal.h"

using namespace pies;

namespace pies {

void ray_free_device(pies_solver* s) {
  for (void* p : s->ray.allocations) (void)ledger::dev_free(p);
  s->ray = RayBuffers{};
}

namespace {

constexpr size_t kRayBatchKeys = 1ull << 24;  // partial keys of one batch of rays at most (128 MB)
constexpr uint32_t kRayNarrowMaxDefault = 512;  // measured crossover on BASELINE config 3's beam surface (narrow no slower up to 512 rays)
constexpr uint32_t kRayWorkgroupsWanted = 1024;  // wide variant: ray blocks x chunks to aim for (4 workgroups per CU)

}  // namespace

// Replaces *d by a buffer of `bytes` bytes (the stream is idle between calls: every call ends in a synchronisation).
int ray_grow_bytes(pies_solver* s, size_t bytes, void** d) {
  RayBuffers& B = s->ray;
  if (*d) {
    B.allocations.erase(std::remove(B.allocations.begin(), B.allocations.end(), *d), B.allocations.end());
    (void)ledger::dev_free(*d);
    *d = nullptr;
  }
  void* p = nullptr;
  HIP_TRY(s, ledger::dev_malloc(&p, std::max<size_t>(bytes, 1)));
  B.allocations.push_back(p);
  *d = p;
  return PIES_OK;
}

namespace {

// The scene's triangle list in the numbering the device holds; built once per pies_finalize (free_device forgets it).
int ray_build_scene_triangles(pies_solver* s) {
  RayBuffers& B = s->ray;
  if (B.triBuilt) return PIES_OK;
  const bool perm = s->nodeOrder.active() && s->nodeOrder.inv.size() == s->nodeCount();
  std::vector<uint32_t> ids(s->h_triangles);
  if (perm)
    for (uint32_t& id : ids) id = s->nodeOrder.inv[id];
  if (int rc = ray_grow(s, ids.size(), &B.tri)) return rc;
  if (!ids.empty()) HIP_TRY(s, hipMemcpyAsync(B.tri, ids.data(), ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));  // the staging vector dies with this scope
  B.nTris = static_cast<uint32_t>(ids.size() / 3);
  B.triBuilt = true;
  return PIES_OK;
}

}  // namespace

// The node -> triangle incidence of the scene's triangles for the wind of pies_apply_forces (forces.cpp): CSR by HOST node id, one
// entry (the triangle's index) per corner that names the node, ascending triangle index within a row.  Like the triangle list it
// is built once per pies_finalize.
int ray_build_incidence(pies_solver* s) {
  RayBuffers& B = s->ray;
  if (B.incBuilt) return PIES_OK;
  const uint32_t n = s->nodeCount();
  const std::vector<uint32_t>& tri = s->h_triangles;  // host ids (the call is outside an InternalNumbering scope)
  std::vector<uint32_t> ptr(static_cast<size_t>(n) + 1, 0u), inc(tri.size());
  for (uint32_t id : tri) ++ptr[id + 1];
  for (uint32_t h = 0; h < n; ++h) ptr[h + 1] += ptr[h];
  std::vector<uint32_t> next(ptr.begin(), ptr.end() - 1);
  for (size_t e = 0; e < tri.size(); ++e) inc[next[tri[e]]++] = static_cast<uint32_t>(e / 3);
  if (int rc = ray_grow(s, ptr.size(), &B.incPtr)) return rc;
  if (int rc = ray_grow(s, inc.size(), &B.inc)) return rc;
  HIP_TRY(s, hipMemcpyAsync(B.incPtr, ptr.data(), ptr.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  if (!inc.empty()) HIP_TRY(s, hipMemcpyAsync(B.inc, inc.data(), inc.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));  // the staging vectors die with this scope
  B.incBuilt = true;
  return PIES_OK;
}

namespace {

int all_misses(uint32_t n, uint32_t* hitTriangle, float* hitT, float* hitUv) {
  for (uint32_t r = 0; r < n; ++r) {
    if (hitTriangle) hitTriangle[r] = PIES_RAY_MISS;
    if (hitT) hitT[r] = INFINITY;
    if (hitUv) hitUv[2ull * r] = hitUv[2ull * r + 1] = 0.0f;
  }
  return PIES_OK;
}

}  // namespace

// The triangles of a checked (target, skin) at the positions the device holds; a skin's vertices are evaluated on the stream first.
int ray_open_target(pies_solver* s, int target, uint32_t skin, RayTarget* out) {
  RayBuffers& B = s->ray;
  RayTarget T;
  if (target == PIES_RAY_SKIN) {
    const HostSkin& k = s->h_skins[skin];
    uint64_t firstTri = 0;
    for (uint32_t i = 0; i < skin; ++i) firstTri += s->h_skins[i].tris.size() / 3;
    T.nTris = static_cast<uint32_t>(k.tris.size() / 3);
    T.stride = 3;
    T.pos = s->d_skinOut;  // (indices in the skins' triangle list are global to the concatenated vertices)
    T.tri = s->skin.tri + 3ull * firstTri;
    if (T.nTris) launch_skin_positions(s->stream, s->skin, s->dev.nd.pos, s->d_skinOut, s->skinFirst[skin], k.vertexCount());
  } else {
    if (int rc = ray_build_scene_triangles(s)) return rc;
    T.nTris = B.nTris;
    T.stride = 4;
    T.pos = reinterpret_cast<const float*>(s->dev.nd.pos);
    T.tri = B.tri;
  }
  *out = T;
  return PIES_OK;
}

}  // namespace pies

extern "C" {

int pies_raycast(pies_solver_t* s, int target, uint32_t skin, uint32_t n_rays, const float* origins, const float* directions,
                 float t_max, uint32_t flags, uint32_t* hit_triangle, float* hit_t, float* hit_uv) {
  if (!s) return PIES_ERR_INVALID;
  if (n_rays && (!origins || !directions)) return fail(s, PIES_ERR_INVALID, "pies_raycast: origins or directions is NULL");
  if (target != PIES_RAY_SCENE_TRIANGLES && target != PIES_RAY_SKIN) return fail(s, PIES_ERR_INVALID, "pies_raycast: unknown target");
  if (target == PIES_RAY_SKIN && skin >= s->h_skins.size()) return fail(s, PIES_ERR_INVALID, "pies_raycast: no such skin");
  if (!(t_max >= 0.0f)) return fail(s, PIES_ERR_INVALID, "pies_raycast: t_max must be >= 0 (+inf is allowed)");
  if (n_rays > kRayMaxRays) return fail(s, PIES_ERR_UNSUPPORTED, "pies_raycast: more than 2^26 rays");
  if (n_rays == 0) return PIES_OK;
  if (s->device == PIES_DEVICE_NONE) return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): rays are cast on the device");
  if (int rc = pies_internal_ensure_ready(s)) return rc;
  RayBuffers& B = s->ray;
  RayTarget T;
  if (int rc = ray_open_target(s, target, skin, &T)) return rc;
  if (T.nTris == 0) {
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    return all_misses(n_rays, hit_triangle, hit_t, hit_uv);
  }

  // ---- the variant ----
  bool narrow = n_rays <= kRayNarrowMaxDefault;
  if (const char* e = tuning_env("PIES_RAY_NARROW_MAX")) narrow = n_rays <= static_cast<uint32_t>(std::max(0l, std::atol(e)));
  if (const char* e = tuning_env("PIES_RAY_VARIANT")) {
    if (std::strcmp(e, "wide") == 0) narrow = false;
    else if (std::strcmp(e, "narrow") == 0) narrow = true;
    else return fail(s, PIES_ERR_INVALID, "pies_raycast: PIES_RAY_VARIANT must be wide or narrow");
  }
  uint32_t parts;
  if (narrow) {
    parts = ray_narrow_parts(T.nTris);
  } else {
    const uint32_t nTiles = (T.nTris + kRayTile - 1) / kRayTile, rayBlocks = (n_rays + kRayBlock - 1) / kRayBlock;
    parts = std::min(nTiles, std::max(1u, kRayWorkgroupsWanted / rayBlocks));
    if (const char* e = tuning_env("PIES_RAY_CHUNKS")) {
      const long v = std::atol(e);
      if (v < 1 || v > static_cast<long>(kRayMaxChunks)) return fail(s, PIES_ERR_INVALID, "pies_raycast: PIES_RAY_CHUNKS must be 1 .. 1024");
      parts = static_cast<uint32_t>(v);  // (chunks beyond the last tile are empty: all misses)
    }
  }
  // rays per batch: a multiple of the workgroup, its partial keys bounded
  const uint32_t batch = std::min<uint64_t>(n_rays, std::max<uint64_t>(kRayBlock, kRayBatchKeys / parts / kRayBlock * kRayBlock));

  // ---- buffers ----
  if (B.rayCap < n_rays) {
    B.rayCap = 0;
    if (int rc = ray_grow(s, 6ull * n_rays, &B.rays)) return rc;
    if (int rc = ray_grow(s, n_rays, &B.outTri)) return rc;
    if (int rc = ray_grow(s, n_rays, &B.outT)) return rc;
    if (int rc = ray_grow(s, 2ull * n_rays, &B.outUv)) return rc;
    B.rayCap = n_rays;
  }
  const size_t keys = static_cast<size_t>(batch) * parts;
  if (int rc = ray_reserve(s, keys, &B.partial, &B.partialCap)) return rc;
  if (!narrow)
    if (int rc = ray_reserve(s, T.nTris, &B.records, &B.recordCap, 3)) return rc;
  float *dOrigins = B.rays, *dDirections = B.rays + 3ull * n_rays;
  HIP_TRY(s, hipMemcpyAsync(dOrigins, origins, 3ull * n_rays * sizeof(float), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(s, hipMemcpyAsync(dDirections, directions, 3ull * n_rays * sizeof(float), hipMemcpyHostToDevice, s->stream));

  // ---- the launches ----
  if (!narrow) launch_ray_stage(s->stream, T, B.records);
  for (uint32_t first = 0; first < n_rays; first += batch) {
    RayBatch R;
    R.origins = dOrigins + 3ull * first;
    R.directions = dDirections + 3ull * first;
    R.n = std::min(batch, n_rays - first);
    R.tMax = t_max;
    R.flags = flags;
    if (narrow) launch_ray_cast_narrow(s->stream, T, R, B.partial);
    else launch_ray_cast_wide(s->stream, B.records, T.nTris, R, parts, B.partial);
    launch_ray_resolve(s->stream, T, R, B.partial, parts, B.outTri + first, B.outT + first, B.outUv + 2ull * first);
  }
  HIP_TRY(s, hipGetLastError());
  if (hit_triangle) HIP_TRY(s, hipMemcpyAsync(hit_triangle, B.outTri, n_rays * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
  if (hit_t) HIP_TRY(s, hipMemcpyAsync(hit_t, B.outT, n_rays * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  if (hit_uv) HIP_TRY(s, hipMemcpyAsync(hit_uv, B.outUv, 2ull * n_rays * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return PIES_OK;
}

}  // extern "C"
