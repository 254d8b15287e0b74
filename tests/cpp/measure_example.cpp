// Solver::measureElements / measureNodes through the drop-in class: createTetBox's 3 x 3 x 3 body is stretched along x by writing
// its nodes, given a rigid velocity, and measured where the device holds it.  The program prints the summary and the node sums
// with nine digits (tests/test_measure_cpp.py compares the bits with the numpy restatement of the two rules on the same body) and
// checks what must hold whatever the bits are.  Exit code 0 on success.
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
  s.createTetBox(glm::vec3(0.25f, 1.5f, 0.5f), 1.0f, glm::vec3(0.0f, 0.0f, 0.0f), 1.0f, 1.0f, false);
  const uint32_t n = static_cast<uint32_t>(s.getVertices().size());
  uint32_t tets = 0;
  if (pies_count(s.handle(), PIES_TET, &tets) != PIES_OK || tets == 0 || n == 0) return 2;

  // at rest: every stretch is 1 to rounding, nothing is over, under or inverted
  std::vector<pies_element_measure_t> records;
  const pies_element_summary_t rest = s.measureElements(PIES_TET, 0, UINT32_MAX, &records);
  if (records.size() != tets || rest.inverted || rest.over || rest.under || rest.nonfinite) return 3;
  if (std::fabs(rest.max_stretch - 1.0f) > 1e-5f || std::fabs(rest.min_stretch - 1.0f) > 1e-5f) return 4;
  // an element's volume is signed by its node order and the factory's elements are not all wound alike: the body's volume is the
  // sum of the magnitudes, 2 x 2 x 2 cells of side 1
  double restVolume = 0.0;
  for (const pies_element_measure_t& r : records) restVolume += std::fabs(r.volume);
  if (std::fabs(restVolume - 8.0) > 1e-4) return 4;

  // stretched by 5/4 along x about x = 0, moving rigidly
  std::vector<float> pos(3 * size_t(n)), vel(3 * size_t(n));
  if (pies_read_nodes(s.handle(), PIES_NODE_POSITION, pos.data(), n) != PIES_OK) return 2;
  for (uint32_t i = 0; i < n; ++i) {
    pos[3 * i] *= 1.25f;
    vel[3 * i] = 0.5f, vel[3 * i + 1] = -0.25f, vel[3 * i + 2] = 2.0f;
  }
  if (pies_write_nodes(s.handle(), PIES_NODE_POSITION, pos.data(), n) != PIES_OK) return 2;
  if (pies_write_nodes(s.handle(), PIES_NODE_VELOCITY, vel.data(), n) != PIES_OK) return 2;

  const pies_element_summary_t m = s.measureElements(PIES_TET, 0, UINT32_MAX, &records);
  std::printf("summary %.9g %.9g %.9g %.9g %.9g %.9g %u %u %u %u\n", m.max_stretch, m.min_stretch, m.min_j, m.max_j, m.max_green, m.volume,
              m.inverted, m.over, m.under, m.nonfinite);
  if (m.over != tets || m.under || m.inverted || m.nonfinite) {
    std::printf("measure FAILED: %u of %u elements over their limit\n", m.over, tets);
    return 5;
  }
  if (std::fabs(m.max_stretch - 1.25f) > 1e-5f || std::fabs(m.volume - 1.25f * rest.volume) > 1e-4f) return 6;
  double volume = 0.0;
  for (const pies_element_measure_t& r : records) volume += std::fabs(r.volume);
  if (std::fabs(volume - 10.0) > 1e-4) return 6;
  for (const pies_element_measure_t& r : records)
    if (!(r.flags & PIES_ELEMENT_OVER) || std::fabs(r.j - 1.25f) > 1e-5f) return 7;

  const glm::vec3 about(1.0f, 2.0f, 0.5f);
  const std::vector<pies_node_sums_t> sums = s.measureNodes({{0, n, about}, {n / 2, 7, glm::vec3(0.0f, 0.0f, 0.0f)}, {n, 0, about}});
  if (sums.size() != 3) return 8;
  for (size_t k = 0; k < sums.size(); ++k)
    std::printf("sums %zu %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %u %u\n", k, sums[k].mass, sums[k].momentum[0],
                sums[k].momentum[1], sums[k].momentum[2], sums[k].angular[0], sums[k].angular[1], sums[k].angular[2], sums[k].moment[0],
                sums[k].moment[1], sums[k].moment[2], sums[k].kinetic, sums[k].dynamic, sums[k].fixed);
  // a rigidly translating body: momentum = mass x velocity, kinetic = mass |v|^2 / 2
  const pies_node_sums_t& all = sums[0];
  if (all.dynamic + all.fixed != n || !(all.mass > 0.0f)) return 9;
  if (std::fabs(all.momentum[2] - 2.0f * all.mass) > 1e-4f * all.mass || std::fabs(all.kinetic - 0.5f * 4.3125f * all.mass) > 1e-4f * all.mass) return 10;
  if (sums[1].dynamic + sums[1].fixed != 7 || sums[2].dynamic || sums[2].fixed || sums[2].mass != 0.0f) return 11;
  // a range that leaves the nodes is refused
  bool threw = false;
  try { (void)s.measureNodes({{n - 1, 2, about}}); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) return 12;

  // read-only: the positions are the ones written, and the tick goes on from them
  s.tick(0.0f);
  for (uint32_t i = 0; i < n; ++i) {
    const glm::vec3 p = s.getVertices()[i].position;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return 13;
  }
  std::printf("measure ok: %u elements over their limit at a stretch of %g, %u nodes of mass %g\n", m.over, m.max_stretch, n, all.mass);
  return 0;
}
