// Solver::applyForces through the drop-in class: createSheet's 20 x 20 cloth in a wind whose region cuts it and in a medium that
// brakes everything.  The wind's impulse has a positive component along the wind; the drag on a sheet at rest pulls every movable
// node towards the medium's velocity.  The program prints the reaction with nine digits (tests/test_forces_cpp.py compares the
// bits with the numpy restatement of the rule on the same sheet) and ticks once from the edited velocities.
// Exit code 0 on success.
#include <Pies/Solver.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

int main() {
  Pies::SolverOptions options;
  options.solver = Pies::SolverName::PBD;
  options.iterations = 4;
  Pies::Solver s(options);
  s.createSheet(glm::vec3(0.5f, 3.0f, 0.25f), 1.0f, 2.0f, 1.0f);
  const uint32_t n = static_cast<uint32_t>(s.getVertices().size());
  if (n != 400 || s.getTriangles().empty()) return 2;
  std::vector<glm::vec3> before(n);
  for (uint32_t i = 0; i < n; ++i) before[i] = s.getVertices()[i].position;
  std::vector<float> invMass(n), velocity(3 * size_t(n));
  if (pies_read_nodes(s.handle(), PIES_NODE_INV_MASS, invMass.data(), n) != PIES_OK) return 2;
  uint32_t movable = 0;
  for (float w : invMass) movable += w != 0.0f;

  using Force = Pies::Solver::Force;
  const float dt = 1.0f / 64.0f;
  const glm::vec3 middle = before[n / 2 + 10];
  const std::vector<Force> forces = {
      Force::wind(glm::vec3(1.0f, 2.0f, 6.0f), 1.5f, 0.25f).within(glm::vec3(middle[0] + 0.015625f, middle[1], middle[2]), 4.03125f, PIES_FALLOFF_LINEAR),
      Force::drag(8.0f, glm::vec3(0.0f, -1.0f, 0.0f)),
  };
  const std::vector<Pies::Solver::ForceReaction> reaction = s.applyForces(forces, dt);
  if (reaction.size() != 2) return 3;
  for (size_t k = 0; k < reaction.size(); ++k)
    std::printf("reaction %zu %.9g %.9g %.9g %.9g %.9g %.9g %u\n", k, reaction[k].impulse[0], reaction[k].impulse[1], reaction[k].impulse[2],
                reaction[k].torque[0], reaction[k].torque[1], reaction[k].torque[2], reaction[k].nodes);
  // the wind reaches a part of the sheet, the drag every movable node
  if (reaction[0].nodes == 0 || reaction[0].nodes >= movable || reaction[1].nodes != movable) {
    std::printf("forces FAILED: nodes %u %u of %u movable\n", reaction[0].nodes, reaction[1].nodes, movable);
    return 4;
  }
  // the air pushes along its own direction, the medium pulls the resting sheet down: k = 8 / 64 of (0, -1, 0) per unit of mass
  const glm::vec3 push = reaction[0].impulse;
  if (!(push[0] * 1.0f + push[1] * 2.0f + push[2] * 6.0f > 0.0f)) return 5;
  float mass = 0.0f;
  for (float w : invMass) mass += w != 0.0f ? 1.0f / w : 0.0f;
  if (std::fabs(reaction[1].impulse[1] + 0.125f * mass) > 1e-4f * mass || reaction[1].impulse[0] != 0.0f) {
    std::printf("forces FAILED: drag impulse %g, expected %g\n", reaction[1].impulse[1], -0.125f * mass);
    return 6;
  }
  // positions are where they were; the velocities carry the edit
  for (uint32_t i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c)
      if (s.getVertices()[i].position[c] != before[i][c]) return 7;
  if (pies_read_nodes(s.handle(), PIES_NODE_VELOCITY, velocity.data(), n) != PIES_OK) return 2;
  uint32_t moving = 0;
  for (uint32_t i = 0; i < n; ++i) moving += velocity[3 * i] != 0.0f || velocity[3 * i + 1] != 0.0f || velocity[3 * i + 2] != 0.0f;
  if (moving != movable) return 8;
  // no force: nothing happens; an invalid one is refused
  if (!s.applyForces({}, dt).empty()) return 9;
  bool threw = false;
  try { (void)s.applyForces({Force::radial(middle, 1.0f).within(middle, -1.0f)}, dt); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) return 10;

  // the tick starts from the edited velocities
  s.tick(0.0f);
  float moved = 0.0f;
  for (uint32_t i = 0; i < n; ++i) {
    const glm::vec3 p = s.getVertices()[i].position;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return 11;
    moved = std::fmax(moved, std::fabs(p[2] - before[i][2]));
  }
  if (!(moved > 0.0f)) return 12;
  std::printf("forces ok: wind on %u of %u movable nodes, drag on all; after a tick the sheet has moved %g along z\n", reaction[0].nodes,
              movable, moved);
  return 0;
}
