// Solver::applySurfaceLoads through the drop-in class: a small closed tetrahedral box (addTetMeshVolume, whose boundary becomes the
// scene's triangles, wound outward) holds a gas that is below its rest volume and stands half in a fluid with drag.  The gas
// pushes every boundary node outward and sums to nothing; the fluid lifts the box by about the weight of what it displaces.  The
// program prints reaction, volume and area with nine digits (tests/test_loads_cpp.py compares the bits with the numpy restatement
// of the rule on the same box) and ticks once from the edited velocities.
// Exit code 0 on success.
#include <Pies/Solver.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace {
constexpr int W = 3, H = 4, D = 3;  // nodes per axis
constexpr float kOrigin[3] = {0.5f, 2.0f, 0.25f};
}  // namespace

int main() {
  std::vector<glm::vec3> verts;
  auto lattice = [&](int x, int y, int z) { return static_cast<uint32_t>(z + D * (y + H * x)); };
  for (int x = 0; x < W; ++x)
    for (int y = 0; y < H; ++y)
      for (int z = 0; z < D; ++z) verts.push_back(glm::vec3(kOrigin[0] + 0.5f * x, kOrigin[1] + 0.5f * y, kOrigin[2] + 0.5f * z));
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
  Pies::SolverOptions options;
  options.solver = Pies::SolverName::PD;
  options.iterations = 6;
  Pies::Solver s(options);
  s.addTetMeshVolume(verts, tets, glm::vec3(0.0f, -1.0f, 0.0f), 2.0f, 1.0f, 0.8f, 1.0f, 1.0f, 1.0f, 1.0f);
  const uint32_t n = static_cast<uint32_t>(s.getVertices().size());
  const uint32_t boundary = n - (W - 2) * (H - 2) * (D - 2);
  if (n != W * H * D || s.getTriangles().size() != 4u * ((W - 1) * (H - 1) + (H - 1) * (D - 1) + (W - 1) * (D - 1))) return 2;
  std::vector<glm::vec3> before(n);
  for (uint32_t i = 0; i < n; ++i) before[i] = s.getVertices()[i].position;

  using Load = Pies::Solver::SurfaceLoad;
  const float dt = 1.0f / 64.0f, volume = 1.0f * 1.5f * 1.0f, area = 2.0f * (1.5f + 1.5f + 1.0f);
  const glm::vec3 centre(kOrigin[0] + 0.5f, kOrigin[1] + 0.75f, kOrigin[2] + 0.5f);
  const float level = kOrigin[1] + 0.75f + 0.0078125f;  // the fluid's surface: just above the box's middle
  const std::vector<Load> loads = {
      Load::gas(1.5f, 2.0f).about(centre),
      Load::fluid(9.8125f, glm::vec3(0.0f, level, 0.0f)).withDrag(0.5f, glm::vec3(0.25f, 0.0f, 0.0f)),
  };
  const std::vector<Pies::Solver::SurfaceReaction> reaction = s.applySurfaceLoads(loads, dt);
  if (reaction.size() != 2) return 3;
  for (size_t k = 0; k < reaction.size(); ++k)
    std::printf("reaction %zu %.9g %.9g %.9g %.9g %.9g %.9g %u %.9g %.9g\n", k, reaction[k].impulse[0], reaction[k].impulse[1],
                reaction[k].impulse[2], reaction[k].torque[0], reaction[k].torque[1], reaction[k].torque[2], reaction[k].nodes,
                reaction[k].volume, reaction[k].area);
  // the boundary is wound outward: the volume is the box's, positive; the gas reaches every boundary node, the fluid a part
  for (const auto& r : reaction)
    if (std::fabs(r.volume - volume) > 1e-5f || std::fabs(r.area - area) > 1e-5f) {
      std::printf("loads FAILED: volume %g (%g), area %g (%g)\n", r.volume, volume, r.area, area);
      return 4;
    }
  if (reaction[0].nodes != boundary || reaction[1].nodes == 0 || reaction[1].nodes >= boundary) {
    std::printf("loads FAILED: nodes %u %u of %u on the boundary\n", reaction[0].nodes, reaction[1].nodes, boundary);
    return 5;
  }
  // a pressure on a closed surface sums to nothing; the fluid lifts: about weight x the submerged volume x dt
  const float scale = 1.5f * (2.0f / volume - 1.0f) * area * dt;
  for (int c = 0; c < 3; ++c)
    if (std::fabs(reaction[0].impulse[c]) > 1e-5f * scale || std::fabs(reaction[0].torque[c]) > 1e-5f * scale) return 6;
  const float lift = 9.8125f * (1.0f * 0.75f * 1.0f) * dt;
  if (!(reaction[1].impulse[1] > 0.5f * lift && reaction[1].impulse[1] < 1.5f * lift)) {
    std::printf("loads FAILED: lift %g, expected about %g\n", reaction[1].impulse[1], lift);
    return 7;
  }
  // positions are where they were
  for (uint32_t i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c)
      if (s.getVertices()[i].position[c] != before[i][c]) return 8;
  // no load: nothing happens; an invalid one is refused
  if (!s.applySurfaceLoads({}, dt).empty()) return 9;
  bool threw = false;
  try { (void)s.applySurfaceLoads({Load::gas(1.5f, -1.0f)}, dt); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) return 10;

  // the tick starts from the edited velocities
  s.tick(0.0f);
  for (uint32_t i = 0; i < n; ++i) {
    const glm::vec3 p = s.getVertices()[i].position;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return 11;
  }
  std::printf("loads ok: gas on %u boundary nodes, fluid on %u; lift %g of about %g\n", reaction[0].nodes, reaction[1].nodes,
              reaction[1].impulse[1], lift);
  return 0;
}
