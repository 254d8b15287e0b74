// tet_rows.h (the tetrahedral projection of k_layer on row pairs) against the oracle's statement of the same projection -
// ora::svd3 + ora::svd3_recompose (oracle/ora_math.h) and the clamp, flip and blend of oracle/pies_oracle.cpp (TetCon::project,
// pos += w * (projected - pos)) - bit for bit, on a host: a ballot is the lane's own predicate, a pair a struct of two floats.
// Counts how many inputs took each path of the decomposition and fails if one is empty.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "ora_math.h"
#include "tet_rows.h"

namespace {

struct V4 {
  float x, y, z, w;
};
struct Case {
  V4 x[4];
  float q[3][3];  // Qinv[col][row]
  float lo, hi, w;
};

// the oracle's TetCon::project + the PBD blend
void reference(const Case& c, V4 out[4], ora::Svd3& d) {
  using namespace ora;
  const vec3 p1(c.x[0].x, c.x[0].y, c.x[0].z), p2(c.x[1].x, c.x[1].y, c.x[1].z), p3(c.x[2].x, c.x[2].y, c.x[2].z), p4(c.x[3].x, c.x[3].y, c.x[3].z);
  const mat3 Qinv(vec3(c.q[0][0], c.q[0][1], c.q[0][2]), vec3(c.q[1][0], c.q[1][1], c.q[1][2]), vec3(c.q[2][0], c.q[2][1], c.q[2][2]));
  const mat3 P(p2 - p1, p3 - p1, p4 - p1);
  const mat3 F = P * Qinv;
  float F_[3][3];
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) F_[r][k] = F[r][k];
  d = svd3(F_);
  float s[3];
  for (int i = 0; i < 3; ++i) s[i] = clampf(d.s[i], c.lo, c.hi);
  if (determinant(F) < 0.0f) {
    int k = 0;
    if (d.s[1] <= d.s[k]) k = 1;
    if (d.s[2] <= d.s[k]) k = 2;
    s[k] *= -1.0f;
  }
  float Fhat[3][3];
  svd3_recompose(d, s, Fhat);
  vec3 proj[4] = {vec3(0.0f), vec3(Fhat[0][0], Fhat[0][1], Fhat[0][2]), vec3(Fhat[1][0], Fhat[1][1], Fhat[1][2]), vec3(Fhat[2][0], Fhat[2][1], Fhat[2][2])};
  const vec3 pos[4] = {p1, p2, p3, p4};
  for (int i = 0; i < 4; ++i) {
    vec3 p = pos[i];
    p += c.w * (proj[i] - p);
    out[i] = V4{p.x, p.y, p.z, c.x[i].w};
  }
}

void rows_form(const Case& c, V4 out[4], pies::rows::Paths& paths) {
  for (int i = 0; i < 4; ++i) out[i] = c.x[i];
  // the record layout of pbd_project.h: a0 = Qinv col0 + Qinv[1][0], a1 = Qinv[1][1..2] + Qinv[2][0..1], a2 = Qinv[2][2], min, max, w
  const V4 a0{c.q[0][0], c.q[0][1], c.q[0][2], c.q[1][0]}, a1{c.q[1][1], c.q[1][2], c.q[2][0], c.q[2][1]}, a2{c.q[2][2], c.lo, c.hi, c.w};
  pies::rows::tet_rows(out[0], out[1], out[2], out[3], pies::rows::rest_of(a0, a1, a2), &paths);
}

bool same(float a, float b) {
  uint32_t x, y;
  std::memcpy(&x, &a, 4);
  std::memcpy(&y, &b, 4);
  return x == y || (a != a && b != b);
}

std::mt19937 rng(20240607u);
float uni(float lo, float hi) { return std::uniform_real_distribution<float>(lo, hi)(rng); }

// the element whose matrix handed to the SVD is exactly a (row-major): Qinv = I, node 1 at the origin, edge j = row j of a
Case exact(const float a[3][3], float lo = 0.8f, float hi = 1.0f, float w = 0.35f) {
  Case c{};
  for (int j = 0; j < 3; ++j) c.x[j + 1] = V4{a[j][0], a[j][1], a[j][2], 1.0f};
  c.x[0] = V4{0.0f, 0.0f, 0.0f, 1.0f};
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) c.q[i][k] = i == k ? 1.0f : 0.0f;
  c.lo = lo; c.hi = hi; c.w = w;
  return c;
}
void rotation(float r[3][3]) {  // a random rotation (from a unit quaternion), float
  float q[4], n = 0.0f;
  for (float& v : q) { v = uni(-1.0f, 1.0f); n += v * v; }
  n = 1.0f / std::sqrt(n > 0.0f ? n : 1.0f);
  const float w = q[0] * n, x = q[1] * n, y = q[2] * n, z = q[3] * n;
  const float m[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)},
                         {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)},
                         {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}};
  std::memcpy(r, m, sizeof(m));
}
void usv(const float s[3], float a[3][3]) {  // R1 diag(s) R2
  float r1[3][3], r2[3][3];
  rotation(r1);
  rotation(r2);
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) a[i][k] = r1[i][0] * s[0] * r2[0][k] + r1[i][1] * s[1] * r2[1][k] + r1[i][2] * s[2] * r2[2][k];
}
Case perturbed_rest() {  // a random rest element (edges of a distorted unit cell), its Qinv, and its nodes moved by up to 5 %
  using namespace ora;
  Case c{};
  mat3 Q;
  do {
    for (int j = 0; j < 3; ++j) Q[j] = vec3(uni(-0.3f, 0.3f) + (j == 0), uni(-0.3f, 0.3f) + (j == 1), uni(-0.3f, 0.3f) + (j == 2));
  } while (std::fabs(determinant(Q)) < 0.2f);
  const mat3 Qi = inverse(Q);
  const vec3 o(uni(-5.0f, 5.0f), uni(0.0f, 5.0f), uni(-5.0f, 5.0f));
  c.x[0] = V4{o.x + uni(-0.05f, 0.05f), o.y + uni(-0.05f, 0.05f), o.z + uni(-0.05f, 0.05f), 1.0f};
  for (int j = 0; j < 3; ++j) c.x[j + 1] = V4{o.x + Q[j].x + uni(-0.05f, 0.05f), o.y + Q[j].y + uni(-0.05f, 0.05f), o.z + Q[j].z + uni(-0.05f, 0.05f), 1.0f};
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) c.q[i][k] = Qi[i][k];
  c.lo = uni(0.5f, 0.95f); c.hi = uni(1.0f, 1.3f); c.w = uni(0.02f, 1.0f);
  return c;
}

}  // namespace

int main() {
  std::vector<Case> cases;
  const int N = 10000;
  for (int n = 0; n < 3 * N; ++n) cases.push_back(perturbed_rest());
  for (int n = 0; n < N; ++n) {  // inverted: a perturbed rest state mirrored in a coordinate plane
    Case c = perturbed_rest();
    const int ax = n % 3;
    for (V4& p : c.x) (ax == 0 ? p.x : ax == 1 ? p.y : p.z) *= -1.0f;
    cases.push_back(c);
  }
  for (int n = 0; n < N / 2; ++n) {  // the identity and other diagonal matrices: no pair out of tolerance
    const float s = n == 0 ? 1.0f : uni(0.2f, 3.0f);
    const float a[3][3] = {{s, 0, 0}, {0, n % 2 ? s : uni(0.2f, 3.0f), 0}, {0, 0, n % 3 ? s : uni(0.2f, 3.0f)}};
    cases.push_back(exact(a));
  }
  for (int n = 0; n < N; ++n) {  // exactly one pair out of tolerance: a diagonal matrix and one more entry
    float a[3][3] = {{uni(0.3f, 2.0f), 0, 0}, {0, uni(0.3f, 2.0f), 0}, {0, 0, uni(0.3f, 2.0f)}};
    const int p = n % 3, i = p == 2 ? 1 : 0, k = p == 0 ? 1 : 2;  // the pairs (0,1), (0,2), (1,2)
    a[i][k] = uni(-1.0f, 1.0f);
    if (n % 5 == 0) a[i][i] = -a[i][i];  // (and inverted ones)
    cases.push_back(exact(a));
  }
  for (int n = 0; n < N; ++n) {  // flattened along an axis: one column of the matrix exactly zero, at most one pair out of tolerance
    float a[3][3] = {{uni(0.3f, 2.0f), 0, 0}, {0, uni(0.3f, 2.0f), 0}, {0, 0, uni(0.3f, 2.0f)}};
    const int z = n % 3, i = (z + 1) % 3, k = (z + 2) % 3;
    a[z][z] = 0.0f;
    if (n % 2) a[i][k] = uni(-1.0f, 1.0f);
    cases.push_back(exact(a, 0.8f, 1.0f, uni(0.05f, 1.0f)));
  }
  for (int n = 0; n < N; ++n) {  // flattened obliquely: R1 diag(s0, s1, 0) R2, and the same with all nodes in an oblique plane
    const float s[3] = {uni(0.3f, 2.0f), uni(0.3f, 2.0f), 0.0f};
    float a[3][3];
    usv(s, a);
    cases.push_back(exact(a));
  }
  for (int n = 0; n < N / 2; ++n) {  // two collapsed directions: one column alone, and all edges along one line
    float a[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if (n % 2) a[n % 3][(n / 3) % 3] = uni(0.3f, 2.0f);
    else for (int j = 0; j < 3; ++j) a[j][n % 3] = uni(-2.0f, 2.0f);
    cases.push_back(exact(a));
  }
  for (int n = 0; n < 2 * N; ++n) {  // condition numbers 1e3 .. 1e6: the rotating sweeps must run
    const float s[3] = {uni(0.5f, 2.0f), std::pow(10.0f, -uni(0.0f, 6.0f)), std::pow(10.0f, -uni(3.0f, 6.0f))};
    float a[3][3];
    usv(s, a);
    if (n % 4 == 0) a[0][0] = -a[0][0];
    cases.push_back(exact(a, 0.8f, 1.0f, 1.0f));
  }
  for (int n = 0; n < N; ++n) {  // equal column norms: circulant matrices, and signed permutations of one column's entries
    const float p = uni(0.5f, 2.0f), q = uni(-0.5f, 0.5f), r = n % 2 ? q : uni(-0.5f, 0.5f);
    const float a[3][3] = {{p, q, r}, {r, p, q}, {q, r, p}};
    const float b[3][3] = {{p, -q, r}, {q, r, p}, {-r, p, q}};
    cases.push_back(exact(n % 4 < 2 ? a : b));
  }
  for (int n = 0; n < N; ++n) {  // scaled out of the closed form's range (and out of single precision's for the squares)
    const float scales[4] = {1.0e-20f, 1.0e-8f, 1.0e+6f, 1.0e+10f};
    Case c = perturbed_rest();
    const float f = scales[n % 4];
    for (V4& p : c.x) { p.x *= f; p.y *= f; p.z *= f; }
    cases.push_back(c);
  }

  struct Count { const char* name; long n; } count[] = {{"closed form", 0}, {"no pair out of tolerance", 0}, {"one pair out of tolerance", 0},
      {"p2 out of range", 0}, {"rotating sweeps", 0}, {"sweeps exhausted or >= 2 rotating sweeps", 0}, {"one collapsed direction completed", 0},
      {"two collapsed directions", 0}, {"inverted (smallest singular value flipped)", 0}, {"polish guard met equal norms (inf or NaN)", 0}};
  long bad = 0;
  for (size_t n = 0; n < cases.size(); ++n) {
    V4 ref[4], got[4];
    ora::Svd3 d;
    pies::rows::Paths p;
    reference(cases[n], ref, d);
    rows_form(cases[n], got, p);
    bool ok = true;
    for (int i = 0; i < 4; ++i) ok = ok && same(ref[i].x, got[i].x) && same(ref[i].y, got[i].y) && same(ref[i].z, got[i].z) && same(ref[i].w, got[i].w);
    // the two statements agree on the path as well
    ok = ok && p.closedForm == d.closed_form && (!p.fallback ? 0 : p.exhausted ? pies::rows::kMaxSweeps : p.sweeps) == d.sweeps;
    if (!ok && bad++ < 5)
      std::printf("MISMATCH case %zu: ref (%a %a %a) got (%a %a %a) sweeps %d/%d closed %d/%d\n", n, ref[1].x, ref[1].y, ref[1].z, got[1].x, got[1].y,
                  got[1].z, p.sweeps, d.sweeps, int(p.closedForm), int(d.closed_form));
    const bool flags[] = {p.closedForm, p.identity, p.onePair, p.rangeOut, p.fallback, p.exhausted || p.sweeps >= 2, p.completed, p.twoCollapsed,
                          p.flipped, p.polishGuard};
    for (size_t k = 0; k < sizeof(flags) / sizeof(flags[0]); ++k) count[k].n += flags[k] ? 1 : 0;
  }
  std::printf("%zu inputs, %ld mismatches\n", cases.size(), bad);
  bool empty = false;
  for (const Count& c : count) {
    std::printf("  %-48s %ld\n", c.name, c.n);
    empty = empty || c.n == 0;
  }
  if (bad || empty || cases.size() < 100000) {
    std::printf("tet rows FAILED%s\n", empty ? " (a path was never taken)" : "");
    return 1;
  }
  std::printf("tet rows ok\n");
  return 0;
}
