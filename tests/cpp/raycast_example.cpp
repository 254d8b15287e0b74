// Solver::raycast / raycastSkin through the drop-in class: a small tetrahedral brick (addTetMeshVolume, whose boundary becomes the
// scene's triangles) with a horizontal quad inside it bound as a skin.  A vertical ray from above hits a top triangle at the
// height of the brick's top, a miss reports no hit, the skin is hit at the quad's height, back-face culling turns the hit from
// below into a miss, and after two PD ticks the same ray meets the fallen top further away.  Last, the same vertical ray over createTetBox's lattice.
// Exit code 0 on success.
#include <Pies/Solver.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace {
constexpr int W = 3, H = 3, D = 4;  // nodes per axis
constexpr float kOrigin[3] = {0.5f, 2.0f, 0.5f};

// the hit triangle's node heights, from the render state
void triangle_heights(const Pies::Solver& s, uint32_t triangle, float& lo, float& hi) {
  lo = 1e30f;
  hi = -1e30f;
  for (uint32_t id : s.getTriangles().at(triangle).nodeIds) {
    lo = std::min(lo, s.getVertices().at(id).position[1]);
    hi = std::max(hi, s.getVertices().at(id).position[1]);
  }
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
  const float top = kOrigin[1] + H - 1, mid = kOrigin[1] + 0.75f;
  // the skin: one quad at height `mid`, wound so that its normal points up
  const std::vector<glm::vec3> quad = {glm::vec3(kOrigin[0] + 0.25f, mid, kOrigin[2] + 0.25f), glm::vec3(kOrigin[0] + 0.25f, mid, kOrigin[2] + 2.5f),
                                       glm::vec3(kOrigin[0] + 1.75f, mid, kOrigin[2] + 2.5f), glm::vec3(kOrigin[0] + 1.75f, mid, kOrigin[2] + 0.25f)};
  const std::vector<uint32_t> quadTris = {0, 1, 2, 0, 2, 3};

  Pies::SolverOptions options;
  options.solver = Pies::SolverName::PD;
  options.iterations = 6;
  Pies::Solver s(options);
  s.addTetMeshVolume(verts, tets, glm::vec3(0.0f, -1.0f, 0.0f), 1.0f, 1.0f, 0.8f, 1.0f, 1.0f, 1.0f, 1.0f);
  const uint32_t skin = s.addSkin(quad, quadTris, tets);
  if (s.getTriangles().empty()) return 2;

  // rays: 0 straight down over the brick, 1 down beside it, 2 up from below the quad (inside the brick)
  const float above = top + 3.0f;
  const std::vector<glm::vec3> origins = {glm::vec3(kOrigin[0] + 0.7f, above, kOrigin[2] + 1.3f), glm::vec3(kOrigin[0] - 2.0f, above, kOrigin[2]),
                                          glm::vec3(kOrigin[0] + 0.7f, mid - 0.5f, kOrigin[2] + 1.3f)};
  const std::vector<glm::vec3> directions = {glm::vec3(0.0f, -2.0f, 0.0f), glm::vec3(0.0f, -2.0f, 0.0f), glm::vec3(0.0f, 1.0f, 0.0f)};

  std::vector<Pies::Solver::RayHit> hits = s.raycast(origins, directions, 1e9f);
  if (hits.size() != 3) return 3;
  float lo, hi;
  if (!hits[0].hit || hits[0].triangle >= s.getTriangles().size()) return 4;
  triangle_heights(s, hits[0].triangle, lo, hi);
  // t counts in units of |d| = 2
  if (lo != top || hi != top || std::fabs(hits[0].t - 1.5f) > 1e-5f || std::fabs(hits[0].position[1] - top) > 1e-5f) {
    std::printf("raycast FAILED: top triangle %u at [%g, %g], t %g, y %g\n", hits[0].triangle, lo, hi, hits[0].t, hits[0].position[1]);
    return 5;
  }
  if (!(hits[0].u >= 0.0f && hits[0].v >= 0.0f && hits[0].u + hits[0].v <= 1.0f)) return 6;
  if (hits[1].hit || hits[1].triangle != PIES_RAY_MISS || !std::isinf(hits[1].t)) return 7;
  if (!hits[2].hit) return 8;  // the scene's triangles from inside: the top, seen from below
  if (s.raycast(origins, directions, 1.0f)[0].hit) return 9;  // tMax in front of the top

  std::vector<Pies::Solver::RayHit> skinHits = s.raycastSkin(skin, origins, directions, 1e9f);
  const float tSkin = (above - mid) / 2.0f;
  if (!skinHits[0].hit || skinHits[0].triangle > 1 || std::fabs(skinHits[0].t - tSkin) > 1e-5f || std::fabs(skinHits[0].position[1] - mid) > 1e-5f) {
    std::printf("raycast FAILED: skin t %g (expected %g)\n", skinHits[0].t, tSkin);
    return 10;
  }
  if (skinHits[1].hit || !skinHits[2].hit || std::fabs(skinHits[2].t - 0.5f) > 1e-5f) return 11;
  skinHits = s.raycastSkin(skin, origins, directions, 1e9f, true);
  if (!skinHits[0].hit || skinHits[2].hit) return 12;  // the quad's back is culled
  bool threw = false;
  try { (void)s.raycastSkin(skin + 1, origins, directions, 1.0f); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) return 13;

  // two ticks: the brick falls, the same ray meets its top further away, at the height the render state shows
  s.tick(0.0f);
  s.tick(0.0f);
  hits = s.raycast(origins, directions, 1e9f);
  if (!hits[0].hit) return 14;
  triangle_heights(s, hits[0].triangle, lo, hi);
  if (!(hits[0].t > 1.5f) || !(hits[0].position[1] >= lo - 1e-4f && hits[0].position[1] <= hi + 1e-4f) || !(hi < top)) {
    std::printf("raycast FAILED after ticks: t %g, y %g in [%g, %g]\n", hits[0].t, hits[0].position[1], lo, hi);
    return 15;
  }
  // createTetBox's 3 x 3 x 3 lattice with its own surface triangles: a vertical ray hits a top triangle at the top's height
  Pies::Solver box(options);
  box.createTetBox(glm::vec3(0.25f, 1.5f, 0.5f), 1.0f, glm::vec3(0.0f, 0.0f, 0.0f), 1.0f, 1.0f, false);
  float boxTop = -1e30f, cx = 0.0f, cz = 0.0f;
  for (const auto& vtx : box.getVertices()) {
    boxTop = std::max(boxTop, vtx.position[1]);
    cx += vtx.position[0] / float(box.getVertices().size());
    cz += vtx.position[2] / float(box.getVertices().size());
  }
  const Pies::Solver::RayHit down = box.raycast({glm::vec3(cx + 0.3f, boxTop + 2.0f, cz + 0.2f)}, {glm::vec3(0.0f, -1.0f, 0.0f)}, 1e9f)[0];
  if (!down.hit) return 16;
  triangle_heights(box, down.triangle, lo, hi);
  if (lo != boxTop || hi != boxTop || std::fabs(down.t - 2.0f) > 1e-5f || std::fabs(down.position[1] - boxTop) > 1e-5f) {
    std::printf("raycast FAILED: tet box top %g, triangle at [%g, %g], t %g\n", boxTop, lo, hi, down.t);
    return 17;
  }
  std::printf("raycast ok: top at %g hit at t %g, skin at t %g, after 2 PD ticks t %g\n", top, 1.5f, tSkin, hits[0].t);
  return 0;
}
