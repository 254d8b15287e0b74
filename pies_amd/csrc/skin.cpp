// Embedded surface meshes (pies_add_skin, an extension): the binding of render vertices to tetrahedra on the host (setup
// time, like all scene construction), the device records built from it, and the two read paths.  The reference never got this
// far: Include/Pies/Tetrahedron.h exists, Solver.h declares _spatialHashTets / TetCompRange, Solver.cpp:78-79 holds the
// commented-out bulk insert of the tetrahedra - its hosts draw the simulation nodes themselves.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "capi_internal.h"

using namespace pies;

namespace pies {

namespace {

struct V3 {
  float x, y, z;
};
inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
// det [a, b, c] (columns), the expansion inverse_columns of scene.cpp uses
inline float det3(V3 a, V3 b, V3 c) {
  return a.x * (b.y * c.z - c.y * b.z) - b.x * (a.y * c.z - c.y * a.z) + c.x * (a.y * b.z - b.y * a.z);
}

// The binding rule of pies_hip.h for one (vertex, tetrahedron): false when the tetrahedron is no candidate on its own account
// (flat, or no finite inverse); the box test is the caller's.  w = (w0, w1, w2, w3).
bool barycentric(V3 v, V3 p0, V3 p1, V3 p2, V3 p3, float w[4]) {
  const V3 e1 = sub(p1, p0), e2 = sub(p2, p0), e3 = sub(p3, p0), d = sub(v, p0);
  const float det = det3(e1, e2, e3);
  if (!(std::fabs(det) >= FLT_MIN)) return false;  // (NaN too)
  const float inv = 1.0f / det;
  if (!std::isfinite(inv)) return false;
  w[1] = det3(d, e2, e3) * inv;
  w[2] = det3(e1, d, e3) * inv;
  w[3] = det3(e1, e2, d) * inv;
  w[0] = 1.0f - (w[1] + w[2] + w[3]);
  return std::isfinite(w[0]) && std::isfinite(w[1]) && std::isfinite(w[2]) && std::isfinite(w[3]);
}

// Uniform grid over the grown element boxes: every element is listed in every cell its box overlaps, so the cell of a vertex
// holds all of the vertex's candidates, in ascending element index.
struct ElementGrid {
  float lo[3] = {0, 0, 0}, invCell[3] = {0, 0, 0};
  uint32_t dim[3] = {1, 1, 1};
  std::vector<uint32_t> ptr, items;
  uint32_t cell_of(float v, int a) const {
    const float c = (v - lo[a]) * invCell[a];
    if (!(c > 0.0f)) return 0;
    return std::min(static_cast<uint32_t>(std::min(c, 4.0e6f)), dim[a] - 1);
  }
};

struct Box {
  float lo[3], hi[3];
  bool ok;  // finite
};

void build_grid(const std::vector<Box>& boxes, ElementGrid& G) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  double edge = 0.0;
  size_t live = 0;
  for (const Box& b : boxes) {
    if (!b.ok) continue;
    ++live;
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(lo[a], b.lo[a]);
      hi[a] = std::max(hi[a], b.hi[a]);
      edge += static_cast<double>(b.hi[a]) - b.lo[a];
    }
  }
  G = ElementGrid{};
  if (live) {
    // cells of the mean box edge (an element is listed in ~8 of them), at most 2^22 cells in all
    double h = edge / (3.0 * static_cast<double>(live));
    double ext[3];
    for (int a = 0; a < 3; ++a) ext[a] = static_cast<double>(hi[a]) - lo[a];
    const double longest = std::max(ext[0], std::max(ext[1], ext[2]));
    h = std::max(h, longest / 1024.0);
    for (;;) {
      double cells = 1.0;
      for (int a = 0; a < 3; ++a) cells *= std::max(1.0, std::ceil(h > 0.0 ? ext[a] / h : 1.0));
      if (!(h > 0.0) || cells <= 4194304.0) break;
      h *= 1.26;
    }
    for (int a = 0; a < 3; ++a) {
      G.lo[a] = lo[a];
      const double cnt = h > 0.0 ? std::max(1.0, std::ceil(ext[a] / h)) : 1.0;
      G.dim[a] = static_cast<uint32_t>(std::min(cnt, 1024.0));
      G.invCell[a] = ext[a] > 0.0 ? static_cast<float>(G.dim[a] / ext[a]) : 0.0f;
      if (!std::isfinite(G.invCell[a])) { G.invCell[a] = 0.0f; G.dim[a] = 1; }
    }
  }
  const size_t ncell = static_cast<size_t>(G.dim[0]) * G.dim[1] * G.dim[2];
  G.ptr.assign(ncell + 1, 0u);
  auto for_cells = [&](const Box& b, auto&& f) {
    uint32_t c0[3], c1[3];
    for (int a = 0; a < 3; ++a) { c0[a] = G.cell_of(b.lo[a], a); c1[a] = G.cell_of(b.hi[a], a); }
    for (uint32_t x = c0[0]; x <= c1[0]; ++x)
      for (uint32_t y = c0[1]; y <= c1[1]; ++y)
        for (uint32_t z = c0[2]; z <= c1[2]; ++z) f((static_cast<size_t>(x) * G.dim[1] + y) * G.dim[2] + z);
  };
  for (const Box& b : boxes)
    if (b.ok) for_cells(b, [&](size_t c) { ++G.ptr[c + 1]; });
  for (size_t c = 0; c < ncell; ++c) G.ptr[c + 1] += G.ptr[c];
  G.items.resize(G.ptr[ncell]);
  std::vector<uint32_t> fill(G.ptr.begin(), G.ptr.end() - 1);
  for (uint32_t t = 0; t < boxes.size(); ++t)
    if (boxes[t].ok) for_cells(boxes[t], [&](size_t c) { G.items[fill[c]++] = t; });
}

}  // namespace

void skin_free_device(pies_solver* s) {
  for (void* p : s->skinAllocations) (void)ledger::dev_free(p);
  s->skinAllocations.clear();
  s->skin = SkinArrays{};
  s->d_skinOut = nullptr;
  s->skinFirst.clear();
  s->skinDirty = !s->h_skins.empty();
}

namespace {
template <class T> int skin_upload_array(pies_solver* s, const std::vector<T>& h, const T** d) {
  *d = nullptr;
  void* p = nullptr;
  HIP_TRY(s, ledger::dev_malloc(&p, std::max<size_t>(h.size(), 1) * sizeof(T)));
  s->skinAllocations.push_back(p);
  if (!h.empty()) HIP_TRY(s, hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s->stream));
  *d = static_cast<const T*>(p);
  return PIES_OK;
}
}  // namespace

// Device records of every skin, skin after skin, node ids translated into the numbering the device holds.
int skin_upload(pies_solver* s) {
  if (s->device == PIES_DEVICE_NONE) return PIES_OK;
  if (s->h_skins.empty()) { s->skinDirty = false; return PIES_OK; }
  HIP_TRY(s, hipStreamSynchronize(s->stream));  // a queued evaluation may still read the old records
  skin_free_device(s);
  const bool perm = s->nodeOrder.active() && s->nodeOrder.inv.size() == s->nodeCount();
  uint64_t nv = 0, nt = 0;
  for (const HostSkin& k : s->h_skins) { nv += k.vertexCount(); nt += k.tris.size() / 3; }
  std::vector<uint4> ids;
  std::vector<float4> w;
  std::vector<uint32_t> tri, incPtr, inc;
  ids.reserve(nv); w.reserve(nv); tri.reserve(3 * nt); incPtr.reserve(nv + 1); inc.reserve(3 * nt);
  s->skinFirst.assign(1, 0u);
  incPtr.push_back(0u);
  for (const HostSkin& k : s->h_skins) {
    const uint32_t firstVert = static_cast<uint32_t>(ids.size()), firstTri = static_cast<uint32_t>(tri.size() / 3);
    for (uint32_t v = 0; v < k.vertexCount(); ++v) {
      uint32_t id[4];
      for (int c = 0; c < 4; ++c) id[c] = perm ? s->nodeOrder.inv[k.ids[4ull * v + c]] : k.ids[4ull * v + c];
      ids.push_back(make_uint4(id[0], id[1], id[2], id[3]));
      w.push_back(make_float4(k.w[4ull * v + 1], k.w[4ull * v + 2], k.w[4ull * v + 3], 0.0f));
      for (uint32_t e = k.incPtr[v]; e < k.incPtr[v + 1]; ++e) inc.push_back(firstTri + k.inc[e]);
      incPtr.push_back(static_cast<uint32_t>(inc.size()));
    }
    for (uint32_t x : k.tris) tri.push_back(firstVert + x);
    s->skinFirst.push_back(static_cast<uint32_t>(ids.size()));
  }
  SkinArrays& S = s->skin;
  if (int rc = skin_upload_array(s, ids, &S.ids)) return rc;
  if (int rc = skin_upload_array(s, w, &S.w)) return rc;
  if (int rc = skin_upload_array(s, tri, &S.tri)) return rc;
  if (int rc = skin_upload_array(s, incPtr, &S.incPtr)) return rc;
  if (int rc = skin_upload_array(s, inc, &S.inc)) return rc;
  S.nVerts = static_cast<uint32_t>(nv);
  S.nTris = static_cast<uint32_t>(nt);
  void* p = nullptr;
  HIP_TRY(s, ledger::dev_malloc(&p, 6ull * nv * sizeof(float)));
  s->skinAllocations.push_back(p);
  s->d_skinOut = static_cast<float*>(p);
  if (s->h_skinStage_n < nv) {
    if (s->h_skinStage) (void)ledger::host_free(s->h_skinStage);
    s->h_skinStage = nullptr;
    s->h_skinStage_n = 0;
    HIP_TRY(s, ledger::host_malloc(reinterpret_cast<void**>(&s->h_skinStage), 6ull * nv * sizeof(float), hipHostMallocDefault));
    s->h_skinStage_n = nv;
  }
  HIP_TRY(s, hipStreamSynchronize(s->stream));  // the staging vectors die with this scope
  s->skinDirty = false;
  return PIES_OK;
}

}  // namespace pies

extern "C" {

int pies_add_skin(pies_solver_t* s, uint32_t n_vertices, const float* positions, uint32_t n_triangles, const uint32_t* tri_ids,
                  uint32_t n_tets, const uint32_t* tet_node_ids, float max_distance, uint32_t* skin_id) {
  if (!s) return PIES_ERR_INVALID;
  if (n_vertices == 0 || !positions) return fail(s, PIES_ERR_INVALID, "pies_add_skin: no vertices");
  if (!(max_distance >= 0.0f) || !std::isfinite(max_distance)) return fail(s, PIES_ERR_INVALID, "pies_add_skin: max_distance must be finite and >= 0");
  if (n_tets == 0 || !tet_node_ids) return fail(s, PIES_ERR_INVALID, "pies_add_skin: no tetrahedra to bind to");
  if (n_triangles && !tri_ids) return fail(s, PIES_ERR_INVALID, "pies_add_skin: tri_ids is NULL");
  uint64_t total = n_vertices;
  for (const HostSkin& k : s->h_skins) total += k.vertexCount();
  if (total > 0x7FFFFFF0ull) return fail(s, PIES_ERR_INVALID, "pies_add_skin: too many skin vertices");
  const uint32_t nodes = s->nodeCount();
  for (size_t i = 0; i < 4ull * n_tets; ++i)
    if (tet_node_ids[i] >= nodes) return fail(s, PIES_ERR_INVALID, "pies_add_skin: node id out of range in tetrahedron " + std::to_string(i / 4));
  for (size_t i = 0; i < 3ull * n_triangles; ++i)
    if (tri_ids[i] >= n_vertices) return fail(s, PIES_ERR_INVALID, "pies_add_skin: vertex index out of range in triangle " + std::to_string(i / 3));
  if (int rc = scene_sync_host(s)) return rc;  // the rule works on the node positions as they are now

  auto node = [&](uint32_t id) { return V3{s->h_pos[3ull * id], s->h_pos[3ull * id + 1], s->h_pos[3ull * id + 2]}; };
  std::vector<Box> boxes(n_tets);
  for (uint32_t t = 0; t < n_tets; ++t) {
    Box& b = boxes[t];
    b.ok = true;
    for (int a = 0; a < 3; ++a) { b.lo[a] = INFINITY; b.hi[a] = -INFINITY; }
    for (int c = 0; c < 4; ++c) {
      const V3 p = node(tet_node_ids[4ull * t + c]);
      const float q[3] = {p.x, p.y, p.z};
      for (int a = 0; a < 3; ++a) { b.lo[a] = std::min(b.lo[a], q[a]); b.hi[a] = std::max(b.hi[a], q[a]); if (!std::isfinite(q[a])) b.ok = false; }
    }
    for (int a = 0; a < 3; ++a) {
      b.lo[a] -= max_distance;
      b.hi[a] += max_distance;
      if (!std::isfinite(b.lo[a]) || !std::isfinite(b.hi[a])) b.ok = false;
    }
  }
  ElementGrid G;
  build_grid(boxes, G);

  HostSkin k;
  k.tet.resize(n_vertices);
  k.ids.resize(4ull * n_vertices);
  k.w.resize(4ull * n_vertices);
  for (uint32_t v = 0; v < n_vertices; ++v) {
    const V3 x{positions[3ull * v], positions[3ull * v + 1], positions[3ull * v + 2]};
    const float q[3] = {x.x, x.y, x.z};
    bool found = false;
    float best = 0.0f, bw[4] = {0, 0, 0, 0};
    uint32_t bt = 0;
    if (std::isfinite(x.x) && std::isfinite(x.y) && std::isfinite(x.z)) {
      const size_t c = (static_cast<size_t>(G.cell_of(x.x, 0)) * G.dim[1] + G.cell_of(x.y, 1)) * G.dim[2] + G.cell_of(x.z, 2);
      for (uint32_t e = G.ptr[c]; e < G.ptr[c + 1]; ++e) {
        const uint32_t t = G.items[e];
        const Box& b = boxes[t];
        if (!(q[0] >= b.lo[0] && q[0] <= b.hi[0] && q[1] >= b.lo[1] && q[1] <= b.hi[1] && q[2] >= b.lo[2] && q[2] <= b.hi[2])) continue;
        const uint32_t* id = tet_node_ids + 4ull * t;
        float w[4];
        if (!barycentric(x, node(id[0]), node(id[1]), node(id[2]), node(id[3]), w)) continue;
        const float m = std::min(std::min(w[0], w[1]), std::min(w[2], w[3]));
        if (!found || m > best) {  // (ascending t: the lowest index keeps a tie)
          found = true;
          best = m;
          bt = t;
          std::memcpy(bw, w, sizeof(bw));
        }
      }
    }
    if (!found)
      return fail(s, PIES_ERR_INVALID, "pies_add_skin: vertex " + std::to_string(v) + " lies in no tetrahedron's box (grown by max_distance)");
    k.tet[v] = bt;
    std::memcpy(&k.ids[4ull * v], tet_node_ids + 4ull * bt, 4 * sizeof(uint32_t));
    std::memcpy(&k.w[4ull * v], bw, sizeof(bw));
  }
  // vertex -> triangle incidence (a triangle that names a vertex twice is listed once for it)
  k.tris.assign(tri_ids, tri_ids + 3ull * n_triangles);
  k.incPtr.assign(n_vertices + 1ull, 0u);
  auto corners = [&](uint32_t t, auto&& f) {
    const uint32_t* c = &k.tris[3ull * t];
    f(c[0]);
    if (c[1] != c[0]) f(c[1]);
    if (c[2] != c[0] && c[2] != c[1]) f(c[2]);
  };
  for (uint32_t t = 0; t < n_triangles; ++t) corners(t, [&](uint32_t v) { ++k.incPtr[v + 1]; });
  for (uint32_t v = 0; v < n_vertices; ++v) k.incPtr[v + 1] += k.incPtr[v];
  k.inc.resize(k.incPtr[n_vertices]);
  {
    std::vector<uint32_t> fill(k.incPtr.begin(), k.incPtr.end() - 1);
    for (uint32_t t = 0; t < n_triangles; ++t) corners(t, [&](uint32_t v) { k.inc[fill[v]++] = t; });
  }
  if (skin_id) *skin_id = static_cast<uint32_t>(s->h_skins.size());
  s->h_skins.push_back(std::move(k));
  s->skinDirty = true;  // the scene itself is untouched: no re-finalize, only the skin records are built again
  return PIES_OK;
}

int pies_get_skin_binding(const pies_solver_t* s, uint32_t skin, uint32_t* tet, uint32_t* node_ids, float* weights, uint32_t capacity,
                          uint32_t* n) {
  if (!s || skin >= s->h_skins.size()) return PIES_ERR_INVALID;
  const HostSkin& k = s->h_skins[skin];
  if (n) *n = k.vertexCount();
  if (!tet && !node_ids && !weights) return PIES_OK;
  if (k.vertexCount() > capacity) return PIES_ERR_INVALID;
  if (tet) std::memcpy(tet, k.tet.data(), k.tet.size() * sizeof(uint32_t));
  if (node_ids) std::memcpy(node_ids, k.ids.data(), k.ids.size() * sizeof(uint32_t));
  if (weights) std::memcpy(weights, k.w.data(), k.w.size() * sizeof(float));
  return PIES_OK;
}

int pies_read_skin(pies_solver_t* s, uint32_t skin, float* positions, float* normals, uint32_t n) {
  if (!s) return PIES_ERR_INVALID;
  if (skin >= s->h_skins.size()) return fail(s, PIES_ERR_INVALID, "pies_read_skin: no such skin");
  if (n != s->h_skins[skin].vertexCount() || !positions) return fail(s, PIES_ERR_INVALID, "pies_read_skin: n does not match the skin's vertex count");
  if (s->device == PIES_DEVICE_NONE) return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): skins are evaluated on the device");
  if (int rc = pies_internal_ensure_ready(s)) return rc;
  const uint32_t first = s->skinFirst[skin], total = s->skin.nVerts;
  float *dPos = s->d_skinOut, *dNrm = s->d_skinOut + 3ull * total;
  launch_skin_positions(s->stream, s->skin, s->dev.nd.pos, dPos, first, n);
  if (normals) launch_skin_normals(s->stream, s->skin, dPos, dNrm, first, n);
  HIP_TRY(s, hipGetLastError());
  float *hPos = s->h_skinStage, *hNrm = s->h_skinStage + 3ull * n;
  HIP_TRY(s, hipMemcpyAsync(hPos, dPos + 3ull * first, 3ull * n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  if (normals) HIP_TRY(s, hipMemcpyAsync(hNrm, dNrm + 3ull * first, 3ull * n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  std::memcpy(positions, hPos, 3ull * n * sizeof(float));
  if (normals) std::memcpy(normals, hNrm, 3ull * n * sizeof(float));
  return PIES_OK;
}

int pies_export_acquire_skin(pies_solver_t* s, uint64_t frame, uint32_t skin, const float** positions, const float** normals, uint32_t* n) {
  if (!s || !positions) return PIES_ERR_INVALID;
  *positions = nullptr;
  if (normals) *normals = nullptr;
  if (n) *n = 0;
  if (frame == 0 || frame > s->frameBegun || frame + 2 <= s->frameBegun)
    return fail(s, PIES_ERR_STATE, "pies_export_acquire_skin: only the last two frames begun are held");
  if (skin >= s->h_skins.size()) return fail(s, PIES_ERR_INVALID, "pies_export_acquire_skin: no such skin");
  const int b = static_cast<int>(frame & 1u);
  const uint32_t total = s->frameSkinVerts[b];
  if (s->skinDirty || skin + 1 >= s->skinFirst.size() || s->skinFirst[skin + 1] > total)
    return fail(s, PIES_ERR_STATE, "pies_export_acquire_skin: the skin was added after the frame was begun");
  HIP_TRY(s, hipSetDevice(s->device));
  HIP_TRY(s, hipEventSynchronize(s->evCopied[b]));
  s->frameAcquired = frame;
  const uint32_t first = s->skinFirst[skin];
  *positions = s->h_skinExport[b] + 3ull * first;
  if (normals) *normals = s->h_skinExport[b] + 3ull * total + 3ull * first;
  if (n) *n = s->skinFirst[skin + 1] - first;
  return PIES_OK;
}

}  // extern "C"
