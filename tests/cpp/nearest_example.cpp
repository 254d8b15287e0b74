// Solver::closestPoints / closestPointsSkin through the drop-in class: createTetBox's 3 x 3 x 3 lattice with its own surface
// triangles, and a small closed cube inside it bound as a skin.  A point above the top face reports the height above it and
// inside == false, the body's centre reports inside == true, a max distance that cuts reports nothing found, the skin answers the
// same questions with its own triangles, and after two PD ticks the body has fallen away from the point above it.
// Exit code 0 on success.
#include <Pies/Solver.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace {
constexpr int N = 3;  // nodes per axis of createTetBox's lattice, node id = z + N (y + N x)
constexpr float kOrigin[3] = {0.25f, 1.5f, 0.5f};
bool close_to(float a, float b, float tol = 1e-5f) { return std::fabs(a - b) <= tol; }
}  // namespace

int main() {
  Pies::SolverOptions options;
  options.solver = Pies::SolverName::PD;
  options.iterations = 6;
  Pies::Solver s(options);
  s.createTetBox(glm::vec3(kOrigin[0], kOrigin[1], kOrigin[2]), 1.0f, glm::vec3(0.0f, 0.0f, 0.0f), 1.0f, 1.0f, false);
  if (s.getVertices().size() != N * N * N || s.getTriangles().empty()) return 2;
  auto lattice = [&](int x, int y, int z) { return static_cast<uint32_t>(z + N * (y + N * x)); };
  for (int x = 0; x < N; ++x)
    for (int y = 0; y < N; ++y)
      for (int z = 0; z < N; ++z) {
        const glm::vec3& p = s.getVertices().at(lattice(x, y, z)).position;
        if (p[0] != kOrigin[0] + x || p[1] != kOrigin[1] + y || p[2] != kOrigin[2] + z) return 3;
      }
  const float top = kOrigin[1] + (N - 1);
  const glm::vec3 centre(kOrigin[0] + 1.0f, kOrigin[1] + 1.0f, kOrigin[2] + 1.0f);
  const glm::vec3 above(centre[0] + 0.3f, top + 0.75f, centre[2] + 0.2f);
  const glm::vec3 distant(centre[0], top + 50.0f, centre[2]);

  std::vector<Pies::Solver::SurfacePoint> r = s.closestPoints({above, centre, distant}, INFINITY, true);
  if (r.size() != 3) return 4;
  if (!r[0].found || r[0].triangle >= s.getTriangles().size() || !close_to(r[0].distance, 0.75f) || r[0].inside ||
      !close_to(r[0].position[0], above[0]) || !close_to(r[0].position[1], top) || !close_to(r[0].position[2], above[2])) {
    std::printf("nearest FAILED: above the top: triangle %u, distance %g, y %g, winding %g\n", r[0].triangle, r[0].distance, r[0].position[1],
                r[0].winding);
    return 5;
  }
  for (uint32_t id : s.getTriangles().at(r[0].triangle).nodeIds)
    if (s.getVertices().at(id).position[1] != top) return 6;  // a triangle of the top face
  if (!(r[0].u >= 0.0f && r[0].v >= 0.0f && r[0].u + r[0].v <= 1.0f + 1e-6f)) return 7;
  if (!r[1].found || !r[1].inside || !close_to(std::fabs(r[1].winding), 1.0f, 1e-3f) || !close_to(r[1].distance, 1.0f)) {
    std::printf("nearest FAILED: the centre: distance %g, winding %g\n", r[1].distance, r[1].winding);
    return 8;
  }
  if (!r[2].found || r[2].inside || !close_to(r[2].winding, 0.0f, 1e-3f) || !close_to(r[2].distance, 50.0f, 1e-4f)) return 9;
  // a max distance that cuts; without the winding pass `winding` and `inside` stay 0
  r = s.closestPoints({above, centre}, 0.5f);
  if (r[0].found || r[0].triangle != PIES_NEAR_NONE || !std::isinf(r[0].distance) || r[0].position[1] != above[1] || r[1].found) return 10;
  if (r[1].inside || r[1].winding != 0.0f) return 11;
  r = s.closestPoints({above}, 0.75f + 1e-3f);
  if (!r[0].found || !close_to(r[0].distance, 0.75f)) return 12;

  // the skin: the cube [0.5, 1.5]^3 about the body's centre, wound outward, bound to Kuhn's six tetrahedra per cell of the lattice
  std::vector<uint32_t> tets;
  static const int order[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (int x = 0; x + 1 < N; ++x)
    for (int y = 0; y + 1 < N; ++y)
      for (int z = 0; z + 1 < N; ++z)
        for (const auto& p : order) {
          int c[3] = {x, y, z};
          tets.push_back(lattice(c[0], c[1], c[2]));
          for (int k = 0; k < 3; ++k) { ++c[p[k]]; tets.push_back(lattice(c[0], c[1], c[2])); }
        }
  std::vector<glm::vec3> cube;
  for (int k = 0; k < 8; ++k)
    cube.push_back(glm::vec3(centre[0] - 0.5f + float(k & 1), centre[1] - 0.5f + float((k >> 1) & 1), centre[2] - 0.5f + float(k >> 2)));
  const std::vector<uint32_t> cubeTris = {0, 4, 6, 0, 6, 2, 1, 3, 7, 1, 7, 5, 0, 1, 5, 0, 5, 4, 2, 6, 7, 2, 7, 3, 0, 2, 3, 0, 3, 1, 4, 5, 7, 4, 7, 6};
  const uint32_t skin = s.addSkin(cube, cubeTris, tets);
  const float skinTop = centre[1] + 0.5f;
  const glm::vec3 overSkin(centre[0] + 0.1f, skinTop + 0.25f, centre[2] + 0.2f);  // inside the body, above the cube
  r = s.closestPointsSkin(skin, {overSkin, centre, above}, INFINITY, true);
  if (!r[0].found || r[0].triangle >= 12 || !close_to(r[0].distance, 0.25f) || r[0].inside || !close_to(r[0].position[1], skinTop)) {
    std::printf("nearest FAILED: skin: triangle %u, distance %g, winding %g\n", r[0].triangle, r[0].distance, r[0].winding);
    return 13;
  }
  if (!r[1].found || !r[1].inside || !close_to(r[1].winding, 1.0f, 1e-3f) || !close_to(r[1].distance, 0.5f)) return 14;
  if (r[2].inside || !close_to(r[2].distance, 1.25f)) return 15;  // the point above the body is over the cube's top face too
  if (!s.closestPoints({overSkin}, INFINITY, true)[0].inside) return 16;  // ... while the scene's triangles have it inside
  bool threw = false;
  try { (void)s.closestPointsSkin(skin + 1, {centre}); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) return 17;

  // two ticks: the body falls, the point above its top is further from it
  s.tick(0.0f);
  s.tick(0.0f);
  const Pies::Solver::SurfacePoint after = s.closestPoints({above}, INFINITY, true)[0];
  if (!after.found || !(after.distance > 0.75f) || after.inside) {
    std::printf("nearest FAILED after ticks: distance %g\n", after.distance);
    return 18;
  }
  std::printf("nearest ok: top at %g, 0.75 above it, centre inside (winding %g), after 2 PD ticks %g above\n", top, r[1].winding, after.distance);
  return 0;
}
