// Solver::addSkin through the drop-in class: a small tetrahedral brick (addTetMeshVolume), its boundary subdivided twice as
// finely as the elements bound to it as a skin, three PD ticks.  The skin's vertices are convex combinations of the nodes (they
// stay inside the nodes' bounding box), its normals have unit length, and the beginTick / endTick path delivers what tick() does
// on a twin solver.
// Exit code 0 on success.
#include <Pies/Solver.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <utility>
#include <vector>

namespace {
constexpr int W = 4, H = 3, D = 5;  // nodes per axis
constexpr float kOrigin[3] = {0.5f, 1.0f, 0.5f};

bool inside(const std::vector<glm::vec3>& pts, const float lo[3], const float hi[3], float grow) {
  for (const glm::vec3& p : pts)
    for (int k = 0; k < 3; ++k)
      if (!(p[k] >= lo[k] - grow && p[k] <= hi[k] + grow)) return false;
  return true;
}
}  // namespace

int main() {
  std::vector<glm::vec3> verts;
  auto lattice = [&](int x, int y, int z) { return static_cast<uint32_t>(z + D * (y + H * x)); };
  for (int x = 0; x < W; ++x)
    for (int y = 0; y < H; ++y)
      for (int z = 0; z < D; ++z) verts.push_back(glm::vec3(kOrigin[0] + x, kOrigin[1] + y, kOrigin[2] + z));
  std::vector<uint32_t> tets;
  static const int order[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (int x = 0; x + 1 < W; ++x)
    for (int y = 0; y + 1 < H; ++y)
      for (int z = 0; z + 1 < D; ++z)
        for (const auto& p : order) {  // Kuhn split of the cell
          int c[3] = {x, y, z};
          tets.push_back(lattice(c[0], c[1], c[2]));
          for (int k = 0; k < 3; ++k) { ++c[p[k]]; tets.push_back(lattice(c[0], c[1], c[2])); }
        }
  // the brick's boundary at half the element size: points (i, j, k) / 2 with a coordinate on the boundary
  const int n[3] = {2 * (W - 1), 2 * (H - 1), 2 * (D - 1)};
  std::map<std::array<int, 3>, uint32_t> index;
  std::vector<glm::vec3> skin;
  std::vector<uint32_t> tris;
  auto vid = [&](std::array<int, 3> p) {
    auto it = index.find(p);
    if (it != index.end()) return it->second;
    const uint32_t id = static_cast<uint32_t>(skin.size());
    skin.push_back(glm::vec3(kOrigin[0] + 0.5f * p[0], kOrigin[1] + 0.5f * p[1], kOrigin[2] + 0.5f * p[2]));
    index.emplace(p, id);
    return id;
  };
  for (int axis = 0; axis < 3; ++axis) {
    const int u = (axis + 1) % 3, v = (axis + 2) % 3;
    for (int side : {0, n[axis]})
      for (int i = 0; i < n[u]; ++i)
        for (int j = 0; j < n[v]; ++j) {
          auto corner = [&](int a, int b) {
            std::array<int, 3> p{};
            p[axis] = side; p[u] = a; p[v] = b;
            return vid(p);
          };
          uint32_t q[4] = {corner(i, j), corner(i + 1, j), corner(i + 1, j + 1), corner(i, j + 1)};
          if (side == 0) { std::swap(q[0], q[3]); std::swap(q[1], q[2]); }  // outward
          for (uint32_t t : {q[0], q[1], q[2], q[0], q[2], q[3]}) tris.push_back(t);
        }
  }
  Pies::SolverOptions options;
  options.solver = Pies::SolverName::PD;
  options.iterations = 6;
  Pies::Solver a(options), b(options);
  uint32_t ids[2] = {9, 9};
  for (int k = 0; k < 2; ++k) {
    Pies::Solver& s = k ? b : a;
    s.addTetMeshVolume(verts, tets, glm::vec3(0.0f, -1.0f, 0.0f), 1.0f, 1.0f, 0.8f, 1.0f, 1.0f, 1.0f, 1.0f);
    ids[k] = s.addSkin(skin, tris, tets);
  }
  if (ids[0] != 0 || ids[1] != 0) return 2;
  if (a.getSkinVertices(0).size() != skin.size() || a.getSkinNormals(0).size() != skin.size()) return 3;
  const float lo[3] = {kOrigin[0], kOrigin[1], kOrigin[2]}, hi[3] = {kOrigin[0] + W - 1, kOrigin[1] + H - 1, kOrigin[2] + D - 1};
  if (!inside(a.getSkinVertices(0), lo, hi, 1e-3f)) return 4;  // the bound rest state
  for (size_t i = 0; i < skin.size(); ++i)
    for (int k = 0; k < 3; ++k)
      if (std::fabs(a.getSkinVertices(0)[i][k] - skin[i][k]) > 1e-5f) return 5;
  auto unit_normals = [&](const Pies::Solver& s) {
    for (const glm::vec3& m : s.getSkinNormals(0))
      if (std::fabs(std::sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]) - 1.0f) > 1e-5f) return false;
    return true;
  };
  if (!unit_normals(a)) return 6;
  for (int t = 0; t < 3; ++t) {
    a.tick(0.0f);
    b.tick(0.0f);
    // convex combinations of the nodes: inside the nodes' bounding box as it is now
    float nlo[3] = {1e30f, 1e30f, 1e30f}, nhi[3] = {-1e30f, -1e30f, -1e30f};
    for (const auto& vtx : a.getVertices())
      for (int k = 0; k < 3; ++k) { nlo[k] = std::min(nlo[k], vtx.position[k]); nhi[k] = std::max(nhi[k], vtx.position[k]); }
    if (!inside(a.getSkinVertices(0), nlo, nhi, 1e-3f)) return 7;
    if (!unit_normals(a)) return 8;
  }
  float fall = 0.0f;
  for (size_t i = 0; i < skin.size(); ++i) fall = std::max(fall, skin[i][1] - a.getSkinVertices(0)[i][1]);
  // the fourth tick through beginTick / endTick on one solver, tick() on its twin
  a.beginTick();
  a.endTick();
  b.tick(0.0f);
  float dmax = 0.0f, nmax = 0.0f;
  for (size_t i = 0; i < skin.size(); ++i)
    for (int k = 0; k < 3; ++k) {
      if (!std::isfinite(a.getSkinVertices(0)[i][k])) return 9;
      dmax = std::max(dmax, std::fabs(a.getSkinVertices(0)[i][k] - b.getSkinVertices(0)[i][k]));
      nmax = std::max(nmax, std::fabs(a.getSkinNormals(0)[i][k] - b.getSkinNormals(0)[i][k]));
    }
  // the PD tolerance of tests/test_pd_parity_gpu.py (1e-5 x the bounding-box diagonal) for positions; a normal turns by at most
  // a few position errors over the shortest skin edge (0.5)
  const float tol = 1e-5f * std::sqrt(float((W - 1) * (W - 1) + (H - 1) * (H - 1) + (D - 1) * (D - 1))) + 2e-5f;
  if (!(dmax <= tol) || !(nmax <= 16.0f * tol) || !(fall > 0.01f) || !unit_normals(a)) {
    std::printf("skin FAILED: max |export - tick| = %g (normals %g), fall %g\n", dmax, nmax, fall);
    return 10;
  }
  // clear() empties the skins with everything else
  a.clear();
  bool threw = false;
  try { (void)a.getSkinVertices(0); } catch (const std::out_of_range&) { threw = true; }
  if (!threw) return 11;
  std::printf("skin ok: %zu skin vertices, %zu triangles on %zu elements, 4 PD ticks, max |export - tick| = %g\n", skin.size(), tris.size() / 3,
              tets.size() / 4, dmax);
  return 0;
}
