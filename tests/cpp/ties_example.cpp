// Solver::addTies and applyTies through the drop-in class: a second 20 x 20 sheet lies an eighth above the first; its first row is
// sewn to triangles of the first sheet's first rows (group 0), and five nodes of its second row are tied node to node by a seam
// that rips at a tenth (group 1).  The program prints the reaction with nine digits (tests/test_ties_cpp.py compares the bits with
// the numpy restatement of the rule on the same sheets), checks the ripped seam and ticks once from the edited state.
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
  s.createSheet(glm::vec3(0.5f, 3.125f, 0.25f), 1.0f, 2.0f, 1.0f);
  const uint32_t n = static_cast<uint32_t>(s.getVertices().size());
  if (n != 800) return 2;
  std::vector<glm::vec3> before(n);
  for (uint32_t i = 0; i < n; ++i) before[i] = s.getVertices()[i].position;

  using Tie = Pies::Solver::Tie;
  using Group = Pies::Solver::TieGroup;
  const float dt = 1.0f / 64.0f;
  std::vector<Tie> ties;
  for (uint32_t i = 0; i < 20; ++i) ties.push_back(Tie::onTriangle(400 + i, i, i + 1, i + 20, 0.25f, 0.25f, 600.0f, 2.0f, 0));
  for (uint32_t i = 0; i < 5; ++i) ties.push_back(Tie::toNode(420 + i, 20 + i, 300.0f, 1.0f, 1));
  const uint32_t seam = s.addTies(ties, 2);
  if (seam != 0) return 3;

  const std::vector<Group> groups = {Group(before[0]), Group(before[20], 1.0f, 0.1f)};
  std::vector<glm::vec4> perTie;
  const std::vector<Pies::Solver::TieReaction> reaction = s.applyTies(seam, groups, dt, 4, &perTie);
  if (reaction.size() != 2 || perTie.size() != 25) return 4;
  for (int g = 0; g < 2; ++g)
    std::printf("reaction %d %.9g %.9g %.9g %.9g %.9g %.9g %u\n", g, reaction[g].impulse[0], reaction[g].impulse[1], reaction[g].impulse[2],
                reaction[g].torque[0], reaction[g].torque[1], reaction[g].torque[2], reaction[g].live);
  // the seam pulls the upper row down; the node-to-node ties were an eighth long and ripped
  if (reaction[0].live != 20 || !(reaction[0].impulse[1] < 0.0f)) return 5;
  if (reaction[1].live != 0 || reaction[1].impulse[1] != 0.0f) return 6;
  const std::vector<uint8_t> broken = s.tieState(seam);
  uint32_t ripped = 0;
  for (uint32_t i = 0; i < broken.size(); ++i) {
    if (broken[i] != (i >= 20 ? 1 : 0)) return 7;
    ripped += broken[i];
  }
  for (uint32_t i = 20; i < 25; ++i)
    if (!(std::fabs(perTie[i][3] - 0.125f) < 1e-5f) || perTie[i][1] != 0.0f) return 8;
  // ties do not move a node: positions are where they were
  for (uint32_t i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c)
      if (s.getVertices()[i].position[c] != before[i][c]) return 9;

  // a ripped tie stays ripped with the limit gone, and holds again after resetTies; a wrong group count is refused
  const std::vector<Group> slack = {Group(before[0]), Group(before[20])};
  if (s.applyTies(seam, slack, dt)[1].live != 0) return 10;
  s.resetTies(seam);
  if (s.applyTies(seam, slack, dt)[1].live != 5) return 11;
  bool threw = false;
  try { (void)s.applyTies(seam, {Group()}, dt); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) return 12;

  // the tick starts from the edited state
  s.tick(0.0f);
  for (uint32_t i = 0; i < n; ++i) {
    const glm::vec3 p = s.getVertices()[i].position;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return 13;
  }
  std::printf("ties ok: %u live ties pull the upper row with %g along y, %u ties ripped\n", reaction[0].live, reaction[0].impulse[1], ripped);
  return 0;
}
