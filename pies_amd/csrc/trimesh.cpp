// Solver::addTriMeshVolume (Src/PrimitiveUtilities.cpp:164-328) without tetgen: pies_voxelize_tri_mesh, the winding numbers of
// a lattice's cell centres on the device (voxel_kernels.hip), and pies_add_tri_mesh_volume, which turns the cells inside the
// surface into createTetBox's six tetrahedra each and binds the input mesh to them as a skin.  Everything but the winding
// numbers is host code that runs once per body, through the scene's own entry points (pies_add_nodes_ex, the constraint
// adders, pies_add_triangles, pies_add_skin); the rules are stated in pies_hip.h.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "capi_internal.h"
#include "voxel_kernels.h"

using namespace pies;

namespace {

const char* check_mesh(uint32_t nv, const float* positions, uint32_t nt, const uint32_t* tri) {
  if (!positions || nv == 0) return "no vertices";
  if (!tri || nt == 0) return "no triangles";
  for (size_t i = 0; i < 3ull * nt; ++i)
    if (tri[i] >= nv) return "triangle index out of range";
  for (size_t i = 0; i < 3ull * nv; ++i)
    if (!std::isfinite(positions[i])) return "non-finite vertex";
  return nullptr;
}

// The winding numbers of lattice L's cell centres; the mesh has passed check_mesh, the handle has a device.
int winding_on_device(pies_solver* s, uint32_t nv, const float* positions, uint32_t nt, const uint32_t* tri, const VoxelLattice& L,
                      float* winding, uint8_t* inside) {
  const size_t n = static_cast<size_t>(L.dims[0]) * L.dims[1] * L.dims[2];
  HIP_TRY(s, hipSetDevice(s->device));
  Temporaries scope(s);
  float *dPos = nullptr, *dW = nullptr;
  uint32_t* dTri = nullptr;
  uint8_t* dIn = nullptr;
  if (int rc = upload(s, std::vector<float>(positions, positions + 3ull * nv), &dPos)) return rc;
  if (int rc = upload(s, std::vector<uint32_t>(tri, tri + 3ull * nt), &dTri)) return rc;
  if (int rc = dev_alloc(s, n, &dW)) return rc;
  if (int rc = dev_alloc(s, n, &dIn)) return rc;
#ifdef PIES_EXPERIMENTS
  hipEvent_t ev[2] = {nullptr, nullptr};
  HIP_TRY(s, ledger::event_create(&ev[0]));
  HIP_TRY(s, ledger::event_create(&ev[1]));
  HIP_TRY(s, hipEventRecord(ev[0], s->stream));
#endif
  launch_winding(s->stream, dPos, dTri, nt, L, dW, dIn);
  HIP_TRY(s, hipGetLastError());
#ifdef PIES_EXPERIMENTS
  HIP_TRY(s, hipEventRecord(ev[1], s->stream));
  HIP_TRY(s, hipEventSynchronize(ev[1]));
  HIP_TRY(s, hipEventElapsedTime(&s->lastWindingMs, ev[0], ev[1]));
  (void)ledger::event_destroy(ev[0]);
  (void)ledger::event_destroy(ev[1]);
#endif
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  if (winding) HIP_TRY(s, hipMemcpy(winding, dW, n * sizeof(float), hipMemcpyDeviceToHost));
  if (inside) HIP_TRY(s, hipMemcpy(inside, dIn, n, hipMemcpyDeviceToHost));
  return PIES_OK;
}

int check_limits(pies_solver* s, const char* who, uint64_t samples, uint32_t nt) {
  if (samples > kVoxelMaxSamples) return fail(s, PIES_ERR_UNSUPPORTED, std::string(who) + ": more than 2^26 lattice samples");
  if (nt > kVoxelMaxTriangles) return fail(s, PIES_ERR_UNSUPPORTED, std::string(who) + ": more than 2^24 triangles");
  return PIES_OK;
}

// What a failed pies_add_tri_mesh_volume puts back: the sizes of every container the call appends to.
struct SceneMark {
  size_t nodes, position, distance, tet, volume, bend, triangles, lines, skins;
  uint32_t constraintId;
  bool skinDirty;
  explicit SceneMark(const pies_solver* s)
      : nodes(s->nodeCount()), position(s->h_position.size()), distance(s->h_distance.size()), tet(s->h_tet.size()),
        volume(s->h_volume.size()), bend(s->h_bend.size()), triangles(s->h_triangles.size()), lines(s->h_lines.size()),
        skins(s->h_skins.size()), constraintId(s->constraintId), skinDirty(s->skinDirty) {}
  template <class V> static void cut(V& v, size_t n) {
    if (v.size() > n) v.erase(v.begin() + static_cast<std::ptrdiff_t>(n), v.end());
  }
  void restore(pies_solver* s) const {
    cut(s->h_pos, 3 * nodes); cut(s->h_prev, 3 * nodes); cut(s->h_vel, 3 * nodes); cut(s->h_radius, nodes); cut(s->h_invMass, nodes);
    cut(s->h_position, position); cut(s->h_distance, distance); cut(s->h_tet, tet); cut(s->h_volume, volume); cut(s->h_bend, bend);
    cut(s->h_triangles, triangles); cut(s->h_lines, lines); cut(s->h_skins, skins);
    s->constraintId = constraintId;
    s->skinDirty = skinDirty;
  }
};

// The boundary rule of Solver::addTetMeshVolume's second overload (include/Pies/Solver.h): a face that belongs to exactly one
// element, elements in order, faces opposite vertex 0, 1, 2, 3, wound so that the normal points away from the fourth vertex.
// tets: local node indices into pos (n x 3).
std::vector<uint32_t> boundary_triangles(const std::vector<float>& pos, const std::vector<uint32_t>& tets) {
  struct Face { uint32_t key[3]; uint32_t index; };
  static const int kFace[4][3] = {{1, 2, 3}, {0, 3, 2}, {0, 1, 3}, {0, 2, 1}};
  const size_t nt = tets.size() / 4;
  std::vector<Face> faces(4 * nt);
  for (size_t t = 0; t < nt; ++t)
    for (uint32_t f = 0; f < 4; ++f) {
      Face& fc = faces[4 * t + f];
      for (int c = 0; c < 3; ++c) fc.key[c] = tets[4 * t + kFace[f][c]];
      std::sort(fc.key, fc.key + 3);
      fc.index = static_cast<uint32_t>(4 * t + f);
    }
  std::sort(faces.begin(), faces.end(), [](const Face& a, const Face& b) {
    for (int c = 0; c < 3; ++c)
      if (a.key[c] != b.key[c]) return a.key[c] < b.key[c];
    return a.index < b.index;
  });
  std::vector<char> boundary(4 * nt, 0);
  for (size_t i = 0; i < faces.size();) {
    size_t j = i + 1;
    while (j < faces.size() && std::memcmp(faces[i].key, faces[j].key, sizeof(faces[i].key)) == 0) ++j;
    if (j == i + 1) boundary[faces[i].index] = 1;
    i = j;
  }
  std::vector<uint32_t> out;
  for (size_t i = 0; i < boundary.size(); ++i) {
    if (!boundary[i]) continue;
    const size_t t = i / 4, f = i % 4;
    uint32_t a = tets[4 * t + kFace[f][0]], b = tets[4 * t + kFace[f][1]], c = tets[4 * t + kFace[f][2]];
    const float *pa = &pos[3ull * a], *pb = &pos[3ull * b], *pc = &pos[3ull * c], *pd = &pos[3ull * tets[4 * t + f]];
    const float ux = pb[0] - pa[0], uy = pb[1] - pa[1], uz = pb[2] - pa[2], vx = pc[0] - pa[0], vy = pc[1] - pa[1], vz = pc[2] - pa[2];
    const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    if (nx * (pd[0] - pa[0]) + ny * (pd[1] - pa[1]) + nz * (pd[2] - pa[2]) > 0.0f) std::swap(b, c);  // normal towards the inside: flip
    out.insert(out.end(), {a, b, c});
  }
  return out;
}

}  // namespace

extern "C" {

#ifdef PIES_EXPERIMENTS
int pies_exp_winding_ms(pies_solver_t* s, float* out) {
  if (!s || !out) return PIES_ERR_INVALID;
  *out = s->lastWindingMs;
  return PIES_OK;
}
#endif

int pies_voxelize_tri_mesh(pies_solver_t* s, uint32_t n_vertices, const float* positions, uint32_t n_triangles,
                           const uint32_t* tri_ids, const float origin[3], float cell, const uint32_t dims[3],
                           float* winding, uint8_t* inside) {
  if (!s) return PIES_ERR_INVALID;
  if (const char* why = check_mesh(n_vertices, positions, n_triangles, tri_ids)) return fail(s, PIES_ERR_INVALID, std::string("pies_voxelize_tri_mesh: ") + why);
  if (!origin || !dims) return fail(s, PIES_ERR_INVALID, "pies_voxelize_tri_mesh: origin or dims is NULL");
  if (!(cell > 0.0f) || !std::isfinite(cell) || !std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
    return fail(s, PIES_ERR_INVALID, "pies_voxelize_tri_mesh: cell must be finite and > 0, origin finite");
  if (dims[0] == 0 || dims[1] == 0 || dims[2] == 0) return fail(s, PIES_ERR_INVALID, "pies_voxelize_tri_mesh: a lattice dimension is 0");
  uint64_t samples = static_cast<uint64_t>(dims[0]) * dims[1];  // (< 2^64)
  samples = samples > kVoxelMaxSamples ? samples : samples * dims[2];
  if (int rc = check_limits(s, "pies_voxelize_tri_mesh", samples, n_triangles)) return rc;
  if (s->device == PIES_DEVICE_NONE) return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): winding numbers are evaluated on the device");
  const VoxelLattice L{{origin[0], origin[1], origin[2]}, cell, {dims[0], dims[1], dims[2]}};
  return winding_on_device(s, n_vertices, positions, n_triangles, tri_ids, L, winding, inside);
}

int pies_add_tri_mesh_volume(pies_solver_t* s, uint32_t n_vertices, const float* positions, uint32_t n_triangles,
                             const uint32_t* tri_ids, const float velocity[3], float density, float strain_stiffness,
                             float min_strain, float max_strain, float volume_stiffness, float compression, float stretching,
                             uint32_t resolution, uint32_t* first_node, uint32_t* n_nodes, uint32_t* n_tets, uint32_t* skin_id) {
  if (!s) return PIES_ERR_INVALID;
  const std::string who = "pies_add_tri_mesh_volume: ";
  if (const char* why = check_mesh(n_vertices, positions, n_triangles, tri_ids)) return fail(s, PIES_ERR_INVALID, who + why);
  if (!velocity) return fail(s, PIES_ERR_INVALID, who + "velocity is NULL");
  if (resolution == 0) return fail(s, PIES_ERR_INVALID, who + "resolution is 0");
  if (!(density > 0.0f)) return fail(s, PIES_ERR_INVALID, who + "density must be > 0");

  // ---- the lattice ----
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, extent[3];
  for (uint32_t v = 0; v < n_vertices; ++v)
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], positions[3ull * v + a]); hi[a] = std::max(hi[a], positions[3ull * v + a]); }
  for (int a = 0; a < 3; ++a) extent[a] = hi[a] - lo[a];
  const float longest = std::max(extent[0], std::max(extent[1], extent[2]));
  if (!(longest > 0.0f) || !std::isfinite(longest)) return fail(s, PIES_ERR_INVALID, who + "the mesh has no extent (or an extent that is not finite)");
  VoxelLattice L;
  L.cell = longest / static_cast<float>(resolution);
  if (!(L.cell > 0.0f)) return fail(s, PIES_ERR_INVALID, who + "the cell size underflows");
  uint64_t samples = 1;
  for (int a = 0; a < 3; ++a) {
    const float cells = std::max(1.0f, std::ceil(extent[a] / L.cell));
    if (!(cells <= static_cast<float>(kVoxelMaxSamples))) return check_limits(s, "pies_add_tri_mesh_volume", ~0ull, n_triangles);
    L.dims[a] = static_cast<uint32_t>(cells);
    L.origin[a] = lo[a] - 0.5f * (cells * L.cell - extent[a]);
    samples = samples > kVoxelMaxSamples ? samples : samples * L.dims[a];
  }
  if (int rc = check_limits(s, "pies_add_tri_mesh_volume", samples, n_triangles)) return rc;
  if (s->device == PIES_DEVICE_NONE) return fail(s, PIES_ERR_HIP, "host-only handle (PIES_DEVICE_NONE): the cells are classified on the device");
  const uint32_t nx = L.dims[0], ny = L.dims[1], nz = L.dims[2];

  // ---- kept cells: inside the surface, or holding an input vertex ----
  std::vector<uint8_t> keep(samples);
  if (int rc = winding_on_device(s, n_vertices, positions, n_triangles, tri_ids, L, nullptr, keep.data())) return rc;
  for (uint32_t v = 0; v < n_vertices; ++v) {
    uint32_t c[3];
    for (int a = 0; a < 3; ++a) {
      const float f = std::floor((positions[3ull * v + a] - L.origin[a]) / L.cell);
      c[a] = !(f > 0.0f) ? 0u : f >= static_cast<float>(L.dims[a]) ? L.dims[a] - 1 : static_cast<uint32_t>(f);
    }
    keep[(static_cast<size_t>(c[0]) * ny + c[1]) * nz + c[2]] = 1;
  }

  // ---- nodes: the lattice points that are a corner of a kept cell, ascending (i, j, k) ----
  const size_t points = static_cast<size_t>(nx + 1) * (ny + 1) * (nz + 1);
  constexpr uint32_t kUnused = 0xFFFFFFFFu;
  std::vector<uint32_t> nodeOf(points, kUnused);
  auto point = [&](uint32_t i, uint32_t j, uint32_t k) { return (static_cast<size_t>(i) * (ny + 1) + j) * (nz + 1) + k; };
  size_t cells = 0;
  for (uint32_t i = 0; i < nx; ++i)
    for (uint32_t j = 0; j < ny; ++j)
      for (uint32_t k = 0; k < nz; ++k) {
        if (!keep[(static_cast<size_t>(i) * ny + j) * nz + k]) continue;
        ++cells;
        for (uint32_t c = 0; c < 8; ++c) nodeOf[point(i + (c >> 2), j + ((c >> 1) & 1u), k + (c & 1u))] = 0;
      }
  if (cells == 0) return fail(s, PIES_ERR_INVALID, who + "no lattice cell lies inside the surface");
  std::vector<float> pos, vel;
  uint32_t count = 0;
  float reach = L.cell;  // largest |coordinate| of the lattice's corners (for the skin's max_distance)
  for (int a = 0; a < 3; ++a)
    reach = std::max(reach, std::max(std::fabs(L.origin[a]), std::fabs(L.origin[a] + static_cast<float>(L.dims[a]) * L.cell)));
  for (uint32_t i = 0; i <= nx; ++i)
    for (uint32_t j = 0; j <= ny; ++j)
      for (uint32_t k = 0; k <= nz; ++k) {
        uint32_t& id = nodeOf[point(i, j, k)];
        if (id == kUnused) continue;
        id = count++;
        pos.insert(pos.end(), {L.origin[0] + static_cast<float>(i) * L.cell, L.origin[1] + static_cast<float>(j) * L.cell,
                               L.origin[2] + static_cast<float>(k) * L.cell});
        vel.insert(vel.end(), {velocity[0], velocity[1], velocity[2]});
      }
  const std::vector<float> radius(count, std::min(0.5f, 0.95f * 0.5f * L.cell)), invMass(count, 1.0f / density);

  // ---- elements: the six tetrahedra of pies_create_tet_box per kept cell (local node indices first: the boundary rule) ----
  std::vector<uint32_t> tets;
  tets.reserve(24 * cells);
  for (uint32_t i = 0; i < nx; ++i)
    for (uint32_t j = 0; j < ny; ++j)
      for (uint32_t k = 0; k < nz; ++k) {
        if (!keep[(static_cast<size_t>(i) * ny + j) * nz + k]) continue;
        auto G = [&](uint32_t x, uint32_t y, uint32_t z) { return nodeOf[point(x, y, z)]; };
        const uint32_t n000 = G(i, j, k), n001 = G(i, j, k + 1), n010 = G(i, j + 1, k), n011 = G(i, j + 1, k + 1);
        const uint32_t n100 = G(i + 1, j, k), n101 = G(i + 1, j, k + 1), n110 = G(i + 1, j + 1, k), n111 = G(i + 1, j + 1, k + 1);
        const uint32_t q[6][4] = {{n000, n001, n011, n111}, {n000, n010, n011, n111}, {n000, n001, n101, n111},
                                  {n000, n100, n101, n111}, {n000, n010, n110, n111}, {n000, n100, n110, n111}};
        tets.insert(tets.end(), &q[0][0], &q[0][0] + 24);
      }
  std::vector<uint32_t> surface = boundary_triangles(pos, tets);

  // ---- into the scene, all or nothing ----
  const SceneMark mark(s);
  auto undo = [&](int rc) {
    const std::string why = s->error;
    mark.restore(s);
    s->error = why;
    return rc;
  };
  uint32_t first = 0, skin = 0;
  if (int rc = pies_add_nodes_ex(s, count, pos.data(), vel.data(), radius.data(), invMass.data(), &first)) return undo(rc);
  for (uint32_t& id : tets) id += first;
  for (uint32_t& id : surface) id += first;
  const uint32_t nt = static_cast<uint32_t>(tets.size() / 4);
  if (strain_stiffness != 0.0f)
    if (int rc = pies_add_tet_constraints(s, nt, tets.data(), strain_stiffness, min_strain, max_strain)) return undo(rc);
  if (volume_stiffness != 0.0f)
    if (int rc = pies_add_volume_constraints(s, nt, tets.data(), volume_stiffness, compression, stretching)) return undo(rc);
  if (int rc = pies_add_triangles(s, static_cast<uint32_t>(surface.size() / 3), surface.data())) return undo(rc);
  if (int rc = pies_add_skin(s, n_vertices, positions, n_triangles, tri_ids, nt, tets.data(), 8.0f * FLT_EPSILON * reach, &skin)) return undo(rc);
  if (first_node) *first_node = first;
  if (n_nodes) *n_nodes = count;
  if (n_tets) *n_tets = nt;
  if (skin_id) *skin_id = skin;
  return PIES_OK;
}

}  // extern "C"
