// Solver::addActuators, actuators and driveActuators through the drop-in class: forty distance constraints of createBox's 5 x 5 x 5
// lattice contract as a muscle band on channel 0, twenty more lengthen by an offset on channel 1.  The program prints the channel
// sums with nine digits (tests/test_actuators_cpp.py compares the bits with the numpy restatement of the rule on the same
// lattice), reads the driven rest lengths back and ticks once: the band pulls its nodes together.
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
  s.createBox(glm::vec3(0.5f, 3.0f, 0.25f), 1.0f, 0.5f);
  const uint32_t n = static_cast<uint32_t>(s.getVertices().size());
  if (n != 125) return 2;
  uint32_t constraints = 0;
  if (pies_count(s.handle(), PIES_DISTANCE, &constraints) != PIES_OK || constraints < 60) return 3;
  std::vector<float> rest0(constraints);
  if (pies_get_rest(s.handle(), PIES_DISTANCE, rest0.data(), constraints) != PIES_OK) return 3;

  using Actuator = Pies::Solver::Actuator;
  std::vector<Actuator> band;
  for (uint32_t i = 0; i < 40; ++i) band.push_back(Actuator::scaled(PIES_DISTANCE, i, 0, -0.5f, 0.25f, 4.0f));
  for (uint32_t i = 40; i < 60; ++i) band.push_back(Actuator::offset(PIES_DISTANCE, i, 1, 0.25f, 0.25f, 4.0f));
  const uint32_t set = s.addActuators(band, 2);
  uint32_t channels = 0;
  const std::vector<pies_actuator_t> stored = s.actuators(set, &channels);
  if (set != 0 || channels != 2 || stored.size() != 60) return 4;
  for (uint32_t i = 0; i < 60; ++i)
    if (stored[i].base != rest0[i] || stored[i].index != i) return 5;

  std::vector<Pies::Solver::ActuatorEntry> entries;
  const std::vector<Pies::Solver::ActuatorChannel> out = s.driveActuators(set, {0.5f, 1.0f}, &entries);
  if (out.size() != 2 || entries.size() != 60) return 6;
  for (uint32_t c = 0; c < 2; ++c) std::printf("channel %u %.9g %.9g %u\n", c, out[c].value, out[c].rest, out[c].live);
  if (out[0].live != 40 || out[1].live != 20) return 7;
  // the host mirror is truthful: pies_get_rest returns the driven values, and only those changed
  std::vector<float> rest1(constraints);
  if (pies_get_rest(s.handle(), PIES_DISTANCE, rest1.data(), constraints) != PIES_OK) return 8;
  for (uint32_t i = 0; i < constraints; ++i) {
    const float want = i < 40 ? rest0[i] * (1.0f + -0.5f * 0.5f) : i < 60 ? rest0[i] + 0.25f * 1.0f : rest0[i];
    if (rest1[i] != want) return 9;
    if (i < 60 && (entries[i].rest != want || !(std::fabs(entries[i].value - rest0[i]) < 1e-5f))) return 10;
  }
  // a channel count that is not the set's, and a non-finite activation, are refused
  for (const std::vector<float>& bad : {std::vector<float>{0.5f}, std::vector<float>{0.5f, NAN}}) {
    bool threw = false;
    try { (void)s.driveActuators(set, bad); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) return 11;
  }
  std::vector<glm::vec3> before(n);
  for (uint32_t i = 0; i < n; ++i) before[i] = s.getVertices()[i].position;
  s.tick(0.0f);
  float moved = 0.0f;
  for (uint32_t i = 0; i < n; ++i) {
    const glm::vec3 p = s.getVertices()[i].position;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return 12;
    for (int c = 0; c < 3; c += 2) moved = std::fmax(moved, std::fabs(p[c] - before[i][c]));
  }
  if (!(moved > 1e-3f)) return 13;  // (gravity acts along y only: a sideways move is the band's)
  std::printf("actuators ok: %u constraints contract to %g of their length, %u lengthen by 0.25; after a tick a node has moved %g sideways\n",
              out[0].live, 0.75, out[1].live, moved);
  return 0;
}
