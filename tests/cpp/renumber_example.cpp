// Solver::renumberNodes through the drop-in class: a tetrahedral mesh whose node ids are shuffled (what a tetrahedraliser hands
// over), ticked under PD once with the extension flag set and once without.  getVertices() is in the host's numbering either way:
// both solvers must end at the same positions (same solve, other summation order).  (tests/test_node_renumber.py checks through the
// C ABI that a shuffled unstructured mesh like this one is renumbered.)
// Exit code 0 on success.
#include <Pies/Solver.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <utility>
#include <vector>

int main() {
  const int W = 8, H = 6, D = 30;
  const uint32_t n = W * H * D;
  // a seeded shuffle of the lattice ids (xorshift + Fisher-Yates): host id perm[k] holds lattice node k
  std::vector<uint32_t> perm(n);
  for (uint32_t i = 0; i < n; ++i) perm[i] = i;
  uint64_t state = 0x9E3779B97F4A7C15ull;
  for (uint32_t i = n - 1; i > 0; --i) {
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    std::swap(perm[i], perm[state % (i + 1)]);
  }
  std::vector<glm::vec3> verts(n);
  auto lattice = [&](int x, int y, int z) { return static_cast<uint32_t>(z + D * (y + H * x)); };
  for (int x = 0; x < W; ++x)
    for (int y = 0; y < H; ++y)
      for (int z = 0; z < D; ++z) verts[perm[lattice(x, y, z)]] = glm::vec3(0.5f + x, 1.0f + y, 0.5f + z);
  std::vector<uint32_t> tets;
  static const int order[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (int x = 0; x + 1 < W; ++x)
    for (int y = 0; y + 1 < H; ++y)
      for (int z = 0; z + 1 < D; ++z)
        for (const auto& p : order) {  // Kuhn split of the cell, positively oriented
          int c[3] = {x, y, z};
          uint32_t v[4];
          v[0] = perm[lattice(c[0], c[1], c[2])];
          for (int k = 0; k < 3; ++k) { ++c[p[k]]; v[k + 1] = perm[lattice(c[0], c[1], c[2])]; }
          const glm::vec3 &a = verts[v[0]], &b = verts[v[1]], &cc = verts[v[2]], &d = verts[v[3]];
          const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], vx = cc[0] - a[0], vy = cc[1] - a[1], vz = cc[2] - a[2];
          const float wx = d[0] - a[0], wy = d[1] - a[1], wz = d[2] - a[2];
          if (ux * (vy * wz - vz * wy) - uy * (vx * wz - vz * wx) + uz * (vx * wy - vy * wx) < 0) std::swap(v[2], v[3]);
          for (uint32_t q : v) tets.push_back(q);
        }
  Pies::SolverOptions options;
  options.solver = Pies::SolverName::PD;
  options.iterations = 6;
  Pies::Solver a(options), b(options);
  a.renumberNodes = true;
  for (Pies::Solver* s : {&a, &b})
    s->addTetMeshVolume(verts, tets, glm::vec3(0.0f, -1.0f, 0.0f), 1.0f, 1.0f, 0.8f, 1.0f, 1.0f, 1.0f, 1.0f);
  if (a.getVertices().size() != n) return 2;
  for (uint32_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k)
      if (a.getVertices()[i].position[k] != verts[i][k]) return 3;
  for (int t = 0; t < 3; ++t) {
    a.tick(0.0f);
    b.tick(0.0f);
  }
  // the export path (beginTick / endTick) in host numbering as well
  a.beginTick();
  a.endTick();
  b.tick(0.0f);
  float dmax = 0.0f, fall = 0.0f;
  for (uint32_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      const float pa = a.getVertices()[i].position[k], pb = b.getVertices()[i].position[k];
      if (!std::isfinite(pa)) return 6;
      dmax = std::max(dmax, std::fabs(pa - pb));
      if (k == 1) fall = std::max(fall, verts[i][1] - pa);
    }
  // the PD tolerance of tests/test_pd_parity_gpu.py: 1e-5 x the body's bounding-box diagonal
  const float tol = 1e-5f * std::sqrt(float((W - 1) * (W - 1) + (H - 1) * (H - 1) + (D - 1) * (D - 1))) + 2e-5f;
  if (!(dmax <= tol) || !(fall > 0.01f)) {
    std::printf("renumber FAILED: max |renumbered - plain| = %g, fall %g\n", dmax, fall);
    return 7;
  }
  std::printf("renumber ok: %u nodes, %zu elements, 4 PD ticks, max |renumbered - plain| = %g\n", n, tets.size() / 4, dmax);
  return 0;
}
