// Solver::collideProps through the drop-in class: createTetBox's 3 x 3 x 3 lattice and three props the host moves.  A sphere
// that descends onto the top face's centre pushes that node down to its surface and hands back an upward impulse, a box beside the
// body that moves into it pushes a side face along its axis, a capsule far away touches nothing; getVertices() shows the edit
// without a tick, and the tick that follows starts from it.
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
  const float mTop = 1.0f / invMass[topCentre], mSide = 1.0f / invMass[sideCentre];

  using Prop = Pies::Solver::Prop;
  // the sphere's lowest point is 0.25 below the top node's own sphere; it descends at 2 per second
  const float ballRadius = 0.5f;
  const glm::vec3 ballCentre(top[0], top[1] + ballRadius + r - 0.25f, top[2]);
  // the box's face is 0.125 inside the side node's sphere; it moves in -x at 1 per second
  const glm::vec3 half(0.5f, 0.25f, 0.25f);
  const glm::vec3 boxCentre(side[0] + r + half[0] - 0.125f, side[1], side[2]);
  std::vector<Prop> props = {
      Prop::sphere(ballCentre, ballRadius).setVelocity(glm::vec3(0.0f, -2.0f, 0.0f)),
      Prop::box(boxCentre, half).setVelocity(glm::vec3(-1.0f, 0.0f, 0.0f)).setFriction(1.0f),
      Prop::capsule(glm::vec3(50.0f, 50.0f, 50.0f), glm::vec3(51.0f, 50.0f, 50.0f), 0.5f),
  };
  const std::vector<Pies::Solver::PropReaction> reaction = s.collideProps(props);
  if (reaction.size() != 3) return 3;
  if (reaction[0].hits != 1 || reaction[1].hits != 1 || reaction[2].hits != 0) {
    std::printf("props FAILED: hits %u %u %u\n", reaction[0].hits, reaction[1].hits, reaction[2].hits);
    return 4;
  }
  // getVertices() shows the push without a tick: the top node 0.25 down, the side node 0.125 in -x, the others where they were
  const glm::vec3 topNow = s.getVertices().at(topCentre).position, sideNow = s.getVertices().at(sideCentre).position;
  if (!close_to(topNow[1], top[1] - 0.25f) || topNow[0] != top[0] || topNow[2] != top[2]) return 5;
  if (!close_to(sideNow[0], side[0] - 0.125f) || sideNow[1] != side[1] || sideNow[2] != side[2]) return 6;
  if (s.getVertices().at(lattice(0, 0, 0)).position[1] != kOrigin[1]) return 7;
  // the nodes were at rest: the sphere gave the top node its own velocity, the reaction on the sphere points up
  if (!close_to(reaction[0].impulse[1], 2.0f * mTop) || !close_to(reaction[0].impulse[0], 0.0f) || !close_to(reaction[0].impulse[2], 0.0f)) {
    std::printf("props FAILED: impulse of the sphere %g %g %g\n", reaction[0].impulse[0], reaction[0].impulse[1], reaction[0].impulse[2]);
    return 8;
  }
  if (!close_to(reaction[1].impulse[0], 1.0f * mSide) || !close_to(reaction[1].impulse[1], 0.0f)) return 9;
  // about the sphere's centre the contact force has no arm sideways: no torque
  if (!close_to(reaction[0].torque[0], 0.0f) || !close_to(reaction[0].torque[2], 0.0f)) return 10;
  if (reaction[2].impulse[0] != 0.0f || reaction[2].torque[1] != 0.0f) return 11;
  // no prop: nothing happens
  if (!s.collideProps({}).empty()) return 12;
  // an invalid prop is refused
  bool threw = false;
  try { (void)s.collideProps({Prop::sphere(ballCentre, -1.0f)}); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) return 13;

  // the tick starts from the pushed state: the top node moves on downwards with the velocity the sphere gave it
  s.tick(0.0f);
  const glm::vec3 after = s.getVertices().at(topCentre).position;
  if (!(after[1] < topNow[1]) || !std::isfinite(after[1])) {
    std::printf("props FAILED after the tick: y %g -> %g\n", topNow[1], after[1]);
    return 14;
  }
  std::printf("props ok: sphere pushed the top node 0.25 down (impulse %g up), box pushed a side node 0.125 in, after a PD tick y = %g\n",
              reaction[0].impulse[1], after[1]);
  return 0;
}
