// Solver::addAnchorsHere and applyAnchors through the drop-in class: the first row of createSheet's 20 x 20 cloth is tied by
// springs to a bar where it hangs, the bar is then lifted, pushed and turned, and the sheet's far corner is pinned to a second
// frame.  The program prints the reaction with nine digits (tests/test_anchors_cpp.py compares the bits with the numpy restatement
// of the rule on the same sheet) and ticks once from the edited state.
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
  if (n != 400) return 2;
  std::vector<glm::vec3> before(n);
  for (uint32_t i = 0; i < n; ++i) before[i] = s.getVertices()[i].position;

  using Frame = Pies::Solver::AnchorFrame;
  const float dt = 1.0f / 64.0f;
  std::vector<uint32_t> row(20);
  for (uint32_t i = 0; i < 20; ++i) row[i] = i;
  const glm::vec3 bar = before[0];
  const uint32_t held = s.addAnchorsHere(row, 0, Frame(bar), 600.0f, 2.0f);
  const uint32_t corner = s.addAnchors({Pies::Solver::Anchor::pin(n - 1, 0, glm::vec3(0.25f, 0.0f, -0.5f))}, 1);
  if (held != 0 || corner != 1) return 3;

  // the bar a little higher than where the row hangs, moving up and turning about its own origin
  Frame lifted(glm::vec3(bar[0], bar[1] + 0.125f, bar[2]));
  lifted.setMotion(glm::vec3(0.0f, 2.0f, 0.5f), glm::vec3(0.0f, 1.5f, 0.0f), glm::vec3(bar[0], bar[1] + 0.125f, bar[2]));
  std::vector<glm::vec4> perAnchor;
  const std::vector<Pies::Solver::AnchorReaction> reaction = s.applyAnchors(held, {lifted}, dt, &perAnchor);
  if (reaction.size() != 1 || perAnchor.size() != 20) return 4;
  std::printf("reaction 0 %.9g %.9g %.9g %.9g %.9g %.9g %u\n", reaction[0].impulse[0], reaction[0].impulse[1], reaction[0].impulse[2],
              reaction[0].torque[0], reaction[0].torque[1], reaction[0].torque[2], reaction[0].live);
  // the bar pulls the row up; every spring is stretched by the lift
  if (reaction[0].live == 0 || !(reaction[0].impulse[1] > 0.0f)) return 5;
  for (const glm::vec4& a : perAnchor)
    if (!(std::fabs(a[3] - 0.125f) < 1e-5f)) return 6;
  // springs do not move a node: positions are where they were
  for (uint32_t i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c)
      if (s.getVertices()[i].position[c] != before[i][c]) return 7;

  // the pin puts the corner on its point of the second frame
  Frame post(glm::vec3(before[n - 1][0], before[n - 1][1] + 0.5f, before[n - 1][2]));
  post.setMotion(glm::vec3(0.0f, 1.0f, 0.0f), glm::vec3(0.0f, 0.0f, 0.0f), glm::vec3(0.0f, 0.0f, 0.0f));
  const std::vector<Pies::Solver::AnchorReaction> pinned = s.applyAnchors(corner, {post}, dt);
  std::printf("reaction 1 %.9g %.9g %.9g %.9g %.9g %.9g %u\n", pinned[0].impulse[0], pinned[0].impulse[1], pinned[0].impulse[2],
              pinned[0].torque[0], pinned[0].torque[1], pinned[0].torque[2], pinned[0].live);
  const glm::vec3 at = s.getVertices()[n - 1].position;
  if (pinned[0].live != 1 || at[0] != before[n - 1][0] + 0.25f || at[1] != before[n - 1][1] + 0.5f || at[2] != before[n - 1][2] - 0.5f) return 8;

  // a released frame does nothing; a frame count that is not the set's is refused
  const std::vector<Pies::Solver::AnchorReaction> off = s.applyAnchors(held, {Frame(bar).setStrength(0.0f)}, dt);
  if (off[0].live != 0 || off[0].impulse[1] != 0.0f) return 9;
  bool threw = false;
  try { (void)s.applyAnchors(held, {lifted, lifted}, dt); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) return 10;

  // the tick starts from the edited state
  s.tick(0.0f);
  float moved = 0.0f;
  for (uint32_t i = 0; i < n; ++i) {
    const glm::vec3 p = s.getVertices()[i].position;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return 11;
    moved = std::fmax(moved, std::fabs(p[1] - before[i][1]));
  }
  if (!(moved > 0.0f)) return 12;
  std::printf("anchors ok: %u live springs pull the row with %g upward, the corner is pinned; after a tick the sheet has moved %g along y\n",
              reaction[0].live, reaction[0].impulse[1], moved);
  return 0;
}
