// Solver::addField / addFieldFromTriMesh / collideFieldProps through the drop-in class: createTetBox's 3 x 3 x 3 lattice and three
// field props the host moves.  A host-sampled plane phi = y, placed upside down above the body and descending, pushes the top
// face's centre node down to its level set and hands back an upward impulse; the field of a small cube, built on the device from
// its twelve triangles, pushes a side node out along -x; a copy of the plane far away touches nothing.  getVertices() shows the
// edit without a tick, and the tick that follows starts from it.
// Exit code 0 on success.
#include <Pies/Solver.h>

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
  if (s.getVertices().size() != N * N * N) return 2;
  auto lattice = [&](int x, int y, int z) { return static_cast<uint32_t>(z + N * (y + N * x)); };
  const uint32_t topCentre = lattice(1, 2, 1), sideCentre = lattice(2, 1, 1);
  const glm::vec3 top = s.getVertices().at(topCentre).position, side = s.getVertices().at(sideCentre).position;
  const float r = s.getVertices().at(topCentre).radius;
  std::vector<float> invMass(N * N * N);
  if (pies_read_nodes(s.handle(), PIES_NODE_INV_MASS, invMass.data(), N * N * N) != PIES_OK) return 2;
  const float mTop = 1.0f / invMass[topCentre];

  // field 0: the plane phi = y on a 5 x 5 x 5 lattice of cell 0.25 about the local origin (a height field from host samples)
  const uint32_t n = 5;
  const float cell = 0.25f;
  std::vector<float> plane(n * n * n);
  for (uint32_t k = 0; k < n; ++k)
    for (uint32_t j = 0; j < n; ++j)
      for (uint32_t i = 0; i < n; ++i) plane[(k * n + j) * n + i] = -0.5f + static_cast<float>(j) * cell;
  const uint32_t planeField = s.addField(n, n, n, glm::vec3(-0.5f, -0.5f, -0.5f), cell, plane);
  // field 1: a cube of half extent 0.25 about the local origin, from its triangles
  std::vector<glm::vec3> corners;
  for (int c = 0; c < 8; ++c) corners.push_back(glm::vec3((c & 1) ? 0.25f : -0.25f, (c & 2) ? 0.25f : -0.25f, (c & 4) ? 0.25f : -0.25f));
  const std::vector<uint32_t> cube = {0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5};
  const uint32_t cubeField = s.addFieldFromTriMesh(corners, cube, 0.125f, 0.5f);
  if (planeField != 0 || cubeField != 1) return 3;

  using FieldProp = Pies::Solver::FieldProp;
  // the plane upside down (local y = world -y): its solid side is above; the level set is 0.25 inside the top node's sphere
  const glm::vec3 above(top[0], top[1] + r - 0.25f, top[2]);
  // the cube's -x face is 0.125 inside the side node's sphere; it moves in -x at 1 per second
  const glm::vec3 beside(side[0] + r + 0.25f - 0.125f, side[1], side[2]);
  std::vector<FieldProp> props = {
      FieldProp(planeField, above).setAxes(glm::vec3(1.0f, 0.0f, 0.0f), glm::vec3(0.0f, -1.0f, 0.0f), glm::vec3(0.0f, 0.0f, -1.0f))
          .setVelocity(glm::vec3(0.0f, -2.0f, 0.0f)),
      FieldProp(cubeField, beside).setVelocity(glm::vec3(-1.0f, 0.0f, 0.0f)).setFriction(1.0f),
      FieldProp(planeField, glm::vec3(50.0f, 50.0f, 50.0f)),
  };
  const std::vector<Pies::Solver::PropReaction> reaction = s.collideFieldProps(props);
  if (reaction.size() != 3) return 4;
  if (reaction[0].hits != 1 || reaction[1].hits != 1 || reaction[2].hits != 0) {
    std::printf("fields FAILED: hits %u %u %u\n", reaction[0].hits, reaction[1].hits, reaction[2].hits);
    return 5;
  }
  // getVertices() shows the push without a tick: the top node 0.25 down (one step onto a plane is exact), the side node 0.125 in -x
  // (the cube's field is sampled: within a hundredth), the others where they were
  const glm::vec3 topNow = s.getVertices().at(topCentre).position, sideNow = s.getVertices().at(sideCentre).position;
  if (!close_to(topNow[1], top[1] - 0.25f) || topNow[0] != top[0] || topNow[2] != top[2]) return 6;
  if (!close_to(sideNow[0], side[0] - 0.125f, 0.01f) || !close_to(sideNow[1], side[1], 0.01f) || !close_to(sideNow[2], side[2], 0.01f)) {
    std::printf("fields FAILED: side node %g %g %g\n", sideNow[0], sideNow[1], sideNow[2]);
    return 7;
  }
  if (s.getVertices().at(lattice(0, 0, 0)).position[1] != kOrigin[1]) return 8;
  // the nodes were at rest: the plane gave the top node its own velocity, the reaction on the plane points up
  if (!close_to(reaction[0].impulse[1], 2.0f * mTop) || !close_to(reaction[0].impulse[0], 0.0f) || !close_to(reaction[0].impulse[2], 0.0f)) {
    std::printf("fields FAILED: impulse of the plane %g %g %g\n", reaction[0].impulse[0], reaction[0].impulse[1], reaction[0].impulse[2]);
    return 9;
  }
  if (!(reaction[1].impulse[0] > 0.0f)) return 10;
  if (reaction[2].impulse[0] != 0.0f || reaction[2].torque[1] != 0.0f) return 11;
  // no prop: nothing happens; an unknown field is refused
  if (!s.collideFieldProps({}).empty()) return 12;
  bool threw = false;
  try { (void)s.collideFieldProps({FieldProp(7, above)}); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) return 13;

  // the tick starts from the pushed state: the top node moves on downwards with the velocity the plane gave it
  s.tick(0.0f);
  const glm::vec3 after = s.getVertices().at(topCentre).position;
  if (!(after[1] < topNow[1]) || !std::isfinite(after[1])) {
    std::printf("fields FAILED after the tick: y %g -> %g\n", topNow[1], after[1]);
    return 14;
  }
  std::printf("fields ok: a sampled plane pushed the top node 0.25 down (impulse %g up), a mesh-built cube pushed a side node %g in, "
              "after a PD tick y = %g\n", reaction[0].impulse[1], side[0] - sideNow[0], after[1]);
  return 0;
}
