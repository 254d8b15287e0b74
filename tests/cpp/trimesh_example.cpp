// Solver::addTriMeshVolume through the drop-in class: an octahedron at triMeshResolution = 4 becomes a lattice body with the
// octahedron as its skin (lastTriMeshSkin); three PD ticks.  The call does not throw, getVertices() / getTriangles() /
// getSkinVertices() are sized and finite after tick(), and the skin's rest vertices are the input vertices.
// Exit code 0 on success.
#include <Pies/Solver.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <vector>

namespace {
bool finite(const glm::vec3& p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }
}  // namespace

int main() {
  const float cx = 0.5f, cy = 2.5f, cz = -0.25f, r = 1.0f;
  const std::vector<glm::vec3> verts = {glm::vec3(cx + r, cy, cz), glm::vec3(cx - r, cy, cz), glm::vec3(cx, cy + r, cz),
                                        glm::vec3(cx, cy - r, cz), glm::vec3(cx, cy, cz + r), glm::vec3(cx, cy, cz - r)};
  const std::vector<uint32_t> tris = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};  // outward
  Pies::SolverOptions options;
  options.solver = Pies::SolverName::PD;
  options.iterations = 6;
  Pies::Solver s(options);
  s.triMeshResolution = 4;
  try {
    s.addTriMeshVolume(verts, tris, glm::vec3(0.0f, -1.0f, 0.0f), 2.0f, 1.0f, 0.8f, 1.0f, 1.0f, 1.0f, 1.0f);
  } catch (const std::exception& e) {
    std::printf("trimesh FAILED: addTriMeshVolume threw: %s\n", e.what());
    return 2;
  }
  const uint32_t skin = s.lastTriMeshSkin;
  if (skin != 0) return 3;
  const size_t nodes = s.getVertices().size(), triangles = s.getTriangles().size();
  // 4 x 4 x 4 cells at most, at least the cells that hold the six vertices; every node belongs to the body
  if (nodes < 8 || nodes > 125 || triangles < 12 || s.getSkinVertices(skin).size() != verts.size() || s.getSkinNormals(skin).size() != verts.size())
    return 4;
  for (size_t i = 0; i < verts.size(); ++i)
    for (int k = 0; k < 3; ++k)
      if (!(std::fabs(s.getSkinVertices(skin)[i][k] - verts[i][k]) <= 1e-5f * 2.0f * r)) {  // the rest state: the input, to 1e-5 x extent
        std::printf("trimesh FAILED: rest vertex %zu is off by %g\n", i, s.getSkinVertices(skin)[i][k] - verts[i][k]);
        return 5;
      }
  for (const auto& t : s.getTriangles())
    for (int k = 0; k < 3; ++k)
      if (t.nodeIds[k] >= nodes) return 6;
  for (int t = 0; t < 3; ++t) s.tick(0.0f);
  if (s.getVertices().size() != nodes || s.getTriangles().size() != triangles || s.getSkinVertices(skin).size() != verts.size()) return 7;
  float fall = 0.0f;
  for (const auto& v : s.getVertices())
    if (!finite(v.position) || !std::isfinite(v.radius)) return 8;
  for (size_t i = 0; i < verts.size(); ++i) {
    if (!finite(s.getSkinVertices(skin)[i]) || !finite(s.getSkinNormals(skin)[i])) return 9;
    fall = std::fmax(fall, verts[i][1] - s.getSkinVertices(skin)[i][1]);
  }
  if (!(fall > 0.01f)) {
    std::printf("trimesh FAILED: the skin did not follow the body (fall %g)\n", fall);
    return 10;
  }
  // a second body gets the next skin id; moving the solver keeps the members
  s.addTriMeshVolume(verts, tris, glm::vec3(0.0f, 0.0f, 0.0f), 2.0f, 1.0f, 0.8f, 1.0f, 0.0f, 1.0f, 1.0f);
  if (s.lastTriMeshSkin != 1 || s.getVertices().size() != 2 * nodes) return 11;
  Pies::Solver moved(std::move(s));
  if (moved.lastTriMeshSkin != 1 || moved.triMeshResolution != 4) return 12;
  std::printf("trimesh ok: %zu nodes, %zu boundary triangles, %zu skin vertices, 3 PD ticks, fall %g\n", nodes, triangles, verts.size(), fall);
  return 0;
}
