// The tetrahedral strain projection of k_layer on ROW PAIRS (gfx950).
//
// The operations and operands are those of tet_core<0> + svd3 + svd3_recompose (pbd_project.h, dev_math.h), one for one: an fmaf is
// an fmaf, a separate multiply and add stay separate, every per-element decision is taken from the element's own data - the
// results are bit for bit the same.  What differs is what stands around the arithmetic:
//
//  * the matrices of the decomposition (A, B = A V, V, the recomposition's t) are held BY ROWS for columns 0 and 1 (struct Mat:
//    r[k] = (M[k][0], M[k][1]), a pair) with column 2 beside them.  Everything the common path does to columns 0 and 1 together is
//    then one pair operation whose operands are pairs as they stand, one half splatted or the halves swapped - all operand
//    selections of a packed instruction (op_sel), no moves: the Gram entries (s00, s11) and (s02, s12), the pair tests against
//    column 2, (d0, d1) and (m00, m11) against a splat, the cofactors (c11, c00) and (c02, c12), B = A V0 row by row, the norms and
//    the rotation <0, 1> (two pair operations per row), the polish with (t02, t12) one recip_rough chain on pairs, the certifying
//    snapshot, the singular values of columns 0, 1 as one rsqrt chain on pairs, and t = B diag(g).  The matrix handed to the SVD
//    arrives in that form for nothing: row c of it is the edges' (x, y) pairs against Qinv[c][j] splatted.  What is left scalar is
//    meant to be: c0.c1, column 2's own entries, the closed form's per-element chain, the rotation's coefficients.  The
//    recomposition's out[r] and the blend are pairs over (x, y) as the node records are, which needs V's columns 0, 1 as (rows 0,
//    1): the one transposition of the common path.
//  * the rare paths carry nothing through the common path: the first certifying snapshot is straight-line code and the sweeps of
//    the plain iteration run only for lanes whose snapshot is not clean; the start of an element with fewer than two pairs out of
//    tolerance and the completion of a collapsed direction likewise.  They run on columns (Col: rows 0, 1 as a pair, row 2; to_cols
//    / from_cols), as rotations <0, 2> and <1, 2> want.  Each stands behind a plain per-lane test: the compiler's branch around a
//    region no lane enters (s_cbranch_execz) skips it, and asks for no ballot in front.
//
// PIES_ROWS_SCALAR (or a host compiler) turns a pair into a struct of two floats: the same code in scalar instructions.  The
// arithmetic compiles for the host (tests/cpp/tet_rows_example.cpp compares it with the oracle's bit for bit).  Used by k_layer
// only: k_tet, k_wave and the experiment variants keep tet_core.
#pragma once
#if defined(__HIP__)
#include "dev_math.h"
#define PIES_ROWS_FN __device__ __forceinline__
#define PIES_ROWS_UNROLL _Pragma("unroll")
#else
#include <cmath>
#include <cstdint>
#include <cstring>
#define PIES_ROWS_FN inline
#define PIES_ROWS_UNROLL
#define PIES_RARE_PATH()
#endif

namespace pies {
namespace rows {

// ---- the shim: what differs between the device and a host ---------------------------------------------------------------------
#if defined(__HIP__)
PIES_ROWS_FN float rf_fma(float a, float b, float c) { return fmaf(a, b, c); }
PIES_ROWS_FN float rf_abs(float a) { return fabsf(a); }
PIES_ROWS_FN float rf_min(float a, float b) { return fminf(a, b); }
PIES_ROWS_FN float rf_max(float a, float b) { return fmaxf(a, b); }
PIES_ROWS_FN float rf_copysign(float a, float b) { return __builtin_copysignf(a, b); }
PIES_ROWS_FN int rf_bits(float a) { return __float_as_int(a); }
PIES_ROWS_FN float rf_float(int a) { return __int_as_float(a); }
#else
inline float rf_fma(float a, float b, float c) { return std::fmaf(a, b, c); }
inline float rf_abs(float a) { return std::fabs(a); }
inline float rf_min(float a, float b) { return std::fmin(a, b); }
inline float rf_max(float a, float b) { return std::fmax(a, b); }
inline float rf_copysign(float a, float b) { return std::copysign(a, b); }
inline int rf_bits(float a) { int32_t i; std::memcpy(&i, &a, 4); return i; }
inline float rf_float(int a) { float f; std::memcpy(&f, &a, 4); return f; }
#endif

// ---- a pair of rows ---------------------------------------------------------------------------------------------------------------
#if defined(__HIP__) && !defined(PIES_ROWS_SCALAR)
typedef float rp __attribute__((ext_vector_type(2)));
PIES_ROWS_FN rp rp_make(float x, float y) { return rp{x, y}; }
PIES_ROWS_FN rp rp_add(rp a, rp b) { return a + b; }
PIES_ROWS_FN rp rp_sub(rp a, rp b) { return a - b; }
PIES_ROWS_FN rp rp_mul(rp a, rp b) { return a * b; }
PIES_ROWS_FN rp rp_neg(rp a) { return -a; }
PIES_ROWS_FN rp rp_fma(rp a, rp b, rp c) { return __builtin_elementwise_fma(a, b, c); }
#else
struct rp {
  float x, y;
};
PIES_ROWS_FN rp rp_make(float x, float y) { return rp{x, y}; }
PIES_ROWS_FN rp rp_add(rp a, rp b) { return rp{a.x + b.x, a.y + b.y}; }
PIES_ROWS_FN rp rp_sub(rp a, rp b) { return rp{a.x - b.x, a.y - b.y}; }
PIES_ROWS_FN rp rp_mul(rp a, rp b) { return rp{a.x * b.x, a.y * b.y}; }
PIES_ROWS_FN rp rp_neg(rp a) { return rp{-a.x, -a.y}; }
PIES_ROWS_FN rp rp_fma(rp a, rp b, rp c) { return rp{rf_fma(a.x, b.x, c.x), rf_fma(a.y, b.y, c.y)}; }
#endif
PIES_ROWS_FN rp rp_splat(float a) { return rp_make(a, a); }

// one column of a 3x3: rows 0, 1 as a pair, row 2
struct Col {
  rp p;
  float z;
};

// ---- the scalar chains of dev_math.h (same constants, same sequences) ----------------------------------------------------------
constexpr int kMaxSweeps = 8;
constexpr float kTol = 4.76837158203125e-07f;  // 4 * 2^-23
constexpr float kTol2 = kTol * kTol;
constexpr float kTiny = 1.0e-18f;
constexpr float kTiny2 = 1.0e-36f;
constexpr float kCos[8] = {8.660253882e-01f,  1.666651964e-01f, -4.807964712e-02f, 2.440584078e-02f,
                           -1.432729699e-02f, 7.718813606e-03f, -2.961986931e-03f, 5.536798271e-04f};
#if defined(__HIP__)
static_assert(kMaxSweeps == kSvdMaxSweeps && kTol == kSvdTol && kTiny == kSvdTiny && kTiny2 == kSvdTiny2 && kCos[0] == kCos3[0] &&
                  kCos[1] == kCos3[1] && kCos[2] == kCos3[2] && kCos[3] == kCos3[3] && kCos[4] == kCos3[4] && kCos[5] == kCos3[5] &&
                  kCos[6] == kCos3[6] && kCos[7] == kCos3[7],
              "tet_rows.h restates dev_math.h's constants");
#endif

PIES_ROWS_FN float rsqrt_nr(float x) {
  float y = rf_float(0x5f3759df - (rf_bits(x) >> 1));
  const float hx = 0.5f * x;
  y = y * rf_fma(-hx, y * y, 1.5f);
  y = y * rf_fma(-hx, y * y, 1.5f);
  y = y * rf_fma(-hx, y * y, 1.5f);
  return y;
}
PIES_ROWS_FN float recip12(float t) {
  float y = rf_fma(-0.47058824f, t, 1.4117647f);
  y = y * rf_fma(-t, y, 2.0f);
  y = y * rf_fma(-t, y, 2.0f);
  y = y * rf_fma(-t, y, 2.0f);
  return y;
}
PIES_ROWS_FN float recip_rough(float x) {
  float y = rf_float(0x7EF311C7 - (rf_bits(x) & 0x7fffffff));
  y = y * rf_fma(-rf_abs(x), y, 2.0f);
  y = y * rf_fma(-rf_abs(x), y, 2.0f);
  return rf_copysign(y, x);
}
PIES_ROWS_FN float cdot(const Col& a, const Col& b) { return rf_fma(a.z, b.z, rf_fma(a.p.y, b.p.y, a.p.x * b.p.x)); }
PIES_ROWS_FN bool pair_needs(float alpha, float beta, float gamma) { return gamma * gamma > rf_fma(kTol2, alpha * beta, kTiny2); }

// jacobi_rotate<P, Q>: the coefficients per element, the six row updates on pairs
template <int P, int Q> PIES_ROWS_FN void rotate(Col (&b)[3], Col (&v)[3], const float alpha, const float beta, const float gamma) {
  const float delta = beta - alpha;
  const float g2 = gamma + gamma;
  const float hw = rf_fma(delta, delta, g2 * g2);
  const float h = hw * rsqrt_nr(hw);
  const float c1 = h + rf_abs(delta);
  const float s1 = delta < 0.0f ? -g2 : g2;
  const float inv = rsqrt_nr(rf_fma(c1, c1, s1 * s1));
  const float cs = c1 * inv, sn = s1 * inv;
  const rp cs2 = rp_splat(cs), sn2 = rp_splat(sn);
  const Col x = b[P], y = b[Q], vx = v[P], vy = v[Q];
  b[P].p = rp_fma(cs2, x.p, rp_neg(rp_mul(sn2, y.p)));
  b[P].z = rf_fma(cs, x.z, -(sn * y.z));
  b[Q].p = rp_fma(sn2, x.p, rp_mul(cs2, y.p));
  b[Q].z = rf_fma(sn, x.z, cs * y.z);
  v[P].p = rp_fma(cs2, vx.p, rp_neg(rp_mul(sn2, vy.p)));
  v[P].z = rf_fma(cs, vx.z, -(sn * vy.z));
  v[Q].p = rp_fma(sn2, vx.p, rp_mul(cs2, vy.p));
  v[Q].z = rf_fma(sn, vx.z, cs * vy.z);
}
// jacobi_pair<P, Q>: the test, and the rotation for the lanes that need it
template <int P, int Q> PIES_ROWS_FN void test_pair(Col (&b)[3], Col (&v)[3]) {
  const float alpha = cdot(b[P], b[P]);
  const float beta = cdot(b[Q], b[Q]);
  const float gamma = cdot(b[P], b[Q]);
  const bool need = pair_needs(alpha, beta, gamma);
  if (need) rotate<P, Q>(b, v, alpha, beta, gamma);
}

// ---- the common path on a 3x3 held BY ROWS for columns 0, 1 ----------------------------------------------------------------------
// r[k] = (M[k][0], M[k][1]): columns 0 and 1 side by side, row by row; column 2 as a Col.  What the common path does to columns 0
// and 1 together - their norms, their products with column 2, the one rotation <0, 1>, the polish, B = A V0 - is then a pair
// operation whose operands are whole pairs, a half splatted or the two halves swapped: all of them operand selections of a packed
// instruction.  The rare paths (rotations <0, 2>, <1, 2>, the completion) run on columns (to_cols / from_cols).
struct Mat {
  rp r[3];
  Col c;
};
PIES_ROWS_FN rp rp_swap(rp a) { return rp_make(a.y, a.x); }
PIES_ROWS_FN void to_cols(const Mat& m, Col (&c)[3]) {
  c[0].p = rp_make(m.r[0].x, m.r[1].x); c[0].z = m.r[2].x;
  c[1].p = rp_make(m.r[0].y, m.r[1].y); c[1].z = m.r[2].y;
  c[2] = m.c;
}
PIES_ROWS_FN void from_cols(const Col (&c)[3], Mat& m) {
  m.r[0] = rp_make(c[0].p.x, c[1].p.x);
  m.r[1] = rp_make(c[0].p.y, c[1].p.y);
  m.r[2] = rp_make(c[0].z, c[1].z);
  m.c = c[2];
}
// cdot of columns: (c0.c0, c1.c1), c0.c1, (c0.c2, c1.c2); c2.c2 is cdot(m.c, m.c)
PIES_ROWS_FN rp dot_self(const Mat& m) { return rp_fma(m.r[2], m.r[2], rp_fma(m.r[1], m.r[1], rp_mul(m.r[0], m.r[0]))); }
PIES_ROWS_FN float dot_01(const Mat& m) { return rf_fma(m.r[2].x, m.r[2].y, rf_fma(m.r[1].x, m.r[1].y, m.r[0].x * m.r[0].y)); }
PIES_ROWS_FN rp dot_with2(const Mat& m) {
  return rp_fma(m.r[2], rp_splat(m.c.z), rp_fma(m.r[1], rp_splat(m.c.p.y), rp_mul(m.r[0], rp_splat(m.c.p.x))));
}
// pair_needs of (column 0, column 2) and (column 1, column 2): both sides as pairs, the comparisons per half
PIES_ROWS_FN void pair_needs2(rp alpha, float beta, rp gamma, bool& n0, bool& n1) {
  const rp lhs = rp_mul(gamma, gamma);
  const rp rhs = rp_fma(rp_splat(kTol2), rp_mul(alpha, rp_splat(beta)), rp_splat(kTiny2));
  n0 = lhs.x > rhs.x;
  n1 = lhs.y > rhs.y;
}
// rsqrt_nr and recip_rough on both halves
PIES_ROWS_FN rp rsqrt_nr2(rp x) {
  rp y = rp_make(rf_float(0x5f3759df - (rf_bits(x.x) >> 1)), rf_float(0x5f3759df - (rf_bits(x.y) >> 1)));
  const rp mhx = rp_neg(rp_mul(rp_splat(0.5f), x));
  y = rp_mul(y, rp_fma(mhx, rp_mul(y, y), rp_splat(1.5f)));
  y = rp_mul(y, rp_fma(mhx, rp_mul(y, y), rp_splat(1.5f)));
  y = rp_mul(y, rp_fma(mhx, rp_mul(y, y), rp_splat(1.5f)));
  return y;
}
PIES_ROWS_FN rp recip_rough2(rp x) {
  const rp max_ = rp_neg(rp_make(rf_abs(x.x), rf_abs(x.y)));
  rp y = rp_make(rf_float(0x7EF311C7 - (rf_bits(x.x) & 0x7fffffff)), rf_float(0x7EF311C7 - (rf_bits(x.y) & 0x7fffffff)));
  y = rp_mul(y, rp_fma(max_, y, rp_splat(2.0f)));
  y = rp_mul(y, rp_fma(max_, y, rp_splat(2.0f)));
  return rp_make(rf_copysign(y.x, x.x), rf_copysign(y.y, x.y));
}

// jacobi_pair<0, 1> on rows: (alpha, beta) one pair chain, the rotation two pair operations per row of B and of V
PIES_ROWS_FN void rotate01(Mat& b, Mat& v, const float alpha, const float beta, const float gamma) {
  const float delta = beta - alpha;
  const float g2 = gamma + gamma;
  const float hw = rf_fma(delta, delta, g2 * g2);
  const float h = hw * rsqrt_nr(hw);
  const float c1 = h + rf_abs(delta);
  const float s1 = delta < 0.0f ? -g2 : g2;
  const float inv = rsqrt_nr(rf_fma(c1, c1, s1 * s1));
  const rp cs = rp_mul(rp_make(c1, s1), rp_splat(inv));  // (cs, sn)
  const rp sc = rp_make(-cs.y, cs.x);  // (-sn, cs): -(sn y) is (-sn) y, the sign of a product being the signs' product
PIES_ROWS_UNROLL
  for (int k = 0; k < 3; ++k) {  // column 0: cs x - sn y, column 1: sn x + cs y
    b.r[k] = rp_fma(cs, rp_splat(b.r[k].x), rp_mul(sc, rp_splat(b.r[k].y)));
    v.r[k] = rp_fma(cs, rp_splat(v.r[k].x), rp_mul(sc, rp_splat(v.r[k].y)));
  }
}
PIES_ROWS_FN void test_pair01(Mat& b, Mat& v) {
  const rp ab = dot_self(b);
  const float gamma = dot_01(b);
  const bool need = pair_needs(ab.x, ab.y, gamma);
  if (need) rotate01(b, v, ab.x, ab.y, gamma);
}
// jacobi_polish on rows
PIES_ROWS_FN void polish(Mat& b, Mat& v, bool* guarded = nullptr) {
  const rp n01 = dot_self(b);
  const float n2 = cdot(b.c, b.c);
  const float g01 = dot_01(b);
  const rp g2 = dot_with2(b);
  float t01 = g01 * recip_rough(n01.y - n01.x);
  const rp t2 = rp_mul(g2, recip_rough2(rp_sub(rp_splat(n2), n01)));  // (t02, t12)
  float t02 = t2.x, t12 = t2.y;
  if (guarded) *guarded = !(rf_abs(t01) <= 3.0e38f) || !(rf_abs(t02) <= 3.0e38f) || !(rf_abs(t12) <= 3.0e38f);  // (the host test's statistics: equal norms, inf or NaN)
  if (!(rf_abs(t01) < 2.5e-4f)) t01 = 0.0f;  // (also NaN: equal norms)
  if (!(rf_abs(t02) < 2.5e-4f)) t02 = 0.0f;
  if (!(rf_abs(t12) < 2.5e-4f)) t12 = 0.0f;
  const rp pm01 = rp_make(-t01, t01), m2 = rp_make(-t02, -t12);
PIES_ROWS_UNROLL
  for (int k = 0; k < 3; ++k) {  // x - t01 y - t02 z | y + t01 x - t12 z | z + t02 x + t12 y
    const float bz = k == 0 ? b.c.p.x : k == 1 ? b.c.p.y : b.c.z, vz = k == 0 ? v.c.p.x : k == 1 ? v.c.p.y : v.c.z;
    const rp bx = b.r[k], vx = v.r[k];
    b.r[k] = rp_fma(m2, rp_splat(bz), rp_fma(pm01, rp_swap(bx), bx));
    v.r[k] = rp_fma(m2, rp_splat(vz), rp_fma(pm01, rp_swap(vx), vx));
    const float bn = rf_fma(t12, bx.y, rf_fma(t02, bx.x, bz)), vn = rf_fma(t12, vx.y, rf_fma(t02, vx.x, vz));
    if (k == 0) { b.c.p.x = bn; v.c.p.x = vn; }
    else if (k == 1) { b.c.p.y = bn; v.c.p.y = vn; }
    else { b.c.z = bn; v.c.z = vn; }
  }
}

// which paths an element took (the host test counts them; the device passes nullptr and the bookkeeping folds away)
struct Paths {
  bool closedForm = false, identity = false, onePair = false, rangeOut = false, fallback = false, exhausted = false;
  bool completed = false, twoCollapsed = false, flipped = false, polishGuard = false;
  int sweeps = 0;
};

// The decomposition A V = B of svd3 (column i of a = what svd3 calls A[i]).  sv = |b_i|, rsv = 1 / |b_i|: columns 0, 1 as a pair,
// column 2.
PIES_ROWS_FN void svd(const Mat& a, Mat& b, Mat& v, rp& sv01, float& sv2, rp& rsv01, float& rsv2, Paths* paths) {
  const rp sd = dot_self(a);  // (s00, s11)
  const float s22 = cdot(a.c, a.c);
  const float s01 = dot_01(a);
  const rp so = dot_with2(a);  // (s02, s12)
  const float s00 = sd.x, s11 = sd.y, s02 = so.x, s12 = so.y;
  const bool n01 = pair_needs(s00, s11, s01);
  bool n02, n12;
  pair_needs2(sd, s22, so, n02, n12);
  const int cnt = (n01 ? 1 : 0) + (n02 ? 1 : 0) + (n12 ? 1 : 0);
  // (straight-line: consumed only where cnt >= 2, where svd3 computes the same values)
  const float q = ((s00 + s11) + s22) * 0.333333343f;
  const rp d01 = rp_sub(sd, rp_splat(q));
  const float d0 = d01.x, d1 = d01.y, d2 = s22 - q;
  const float p1 = rf_fma(s12, s12, rf_fma(s02, s02, s01 * s01));
  const float p2 = rf_fma(d0, d0, rf_fma(d1, d1, rf_fma(d2, d2, p1 + p1)));  // 6 p^2
  const bool closed = cnt >= 2 && p2 > 1.0e-30f && p2 < 1.0e16f;
  if (closed) {
    const float w = p2 * 0.166666672f;
    const float ip = rsqrt_nr(w);
    const float p = w * ip;
    const float det = rf_fma(d0, rf_fma(d1, d2, -(s12 * s12)), rf_fma(s02, rf_fma(s01, s12, -(d1 * s02)), -(s01 * rf_fma(s01, d2, -(s12 * s02)))));
    const float r = ((0.5f * det) * ip) * (ip * ip);
    const float x = rf_min(rf_abs(r), 1.0f);
    float c = kCos[7];
PIES_ROWS_UNROLL
    for (int k = 6; k >= 0; --k) c = rf_fma(c, x, kCos[k]);
    const float lam = q + rf_copysign((p + p) * c, r);
    // the cofactors of S - lam: (m00, m11) one pair subtraction, (c11, c00) and (c02, c12) two pair operations each
    const rp m01 = rp_sub(sd, rp_splat(lam));
    const float m00 = m01.x, m11 = m01.y, m22 = s22 - lam;
    const rp cd = rp_fma(m01, rp_splat(m22), rp_neg(rp_mul(so, so)));
    const rp co = rp_fma(rp_splat(s01), rp_swap(so), rp_neg(rp_mul(so, rp_swap(m01))));
    const float c00 = cd.y, c11 = cd.x, c22 = rf_fma(m00, m11, -(s01 * s01));
    const float c01 = rf_fma(s02, s12, -(s01 * m22)), c02 = co.x, c12 = co.y;
    const float a0 = rf_abs(c00), a1 = rf_abs(c11), a2 = rf_abs(c22);
    const bool k0 = a0 >= a1 && a0 >= a2, k1 = !k0 && a1 >= a2;
    const float v0 = k0 ? c00 : (k1 ? c01 : c02), v1 = k0 ? c01 : (k1 ? c11 : c12), v2 = k0 ? c02 : (k1 ? c12 : c22);
    const float n2 = rf_fma(v2, v2, rf_fma(v1, v1, v0 * v0));
    const bool okn = n2 > kTiny2;
    const float in = rsqrt_nr(okn ? n2 : 1.0f);
    const rp nm = rp_mul(rp_make(v0, v1), rp_splat(in));
    const float nx = okn ? nm.x : 0.0f, ny = okn ? nm.y : 0.0f, nz = okn ? v2 * in : 1.0f;
    const float sg = rf_copysign(1.0f, nz);
    const float aa = -recip12(rf_abs(nz) + 1.0f) * sg;  // -1 / (sg + nz)
    const float bb = (nx * ny) * aa;
    const float sx = sg * nx;
    // V0 = [t1, t2, n] by rows
    v.r[0] = rp_make(rf_fma(sx, nx * aa, 1.0f), bb);
    v.r[1] = rp_make(sg * bb, rf_fma(ny, ny * aa, sg));
    v.r[2] = rp_make(-sx, -ny);
    v.c.p = rp_make(nx, ny);
    v.c.z = nz;
PIES_ROWS_UNROLL
    for (int k = 0; k < 3; ++k) {  // B = A V0: row k of A splatted against the rows of V0; column 2 per entry
      const float ak0 = a.r[k].x, ak1 = a.r[k].y, ak2 = k == 0 ? a.c.p.x : k == 1 ? a.c.p.y : a.c.z;
      b.r[k] = rp_fma(rp_splat(ak2), v.r[2], rp_fma(rp_splat(ak1), v.r[1], rp_mul(rp_splat(ak0), v.r[0])));
      const float bk = rf_fma(ak2, nz, rf_fma(ak1, ny, ak0 * nx));
      if (k == 0) b.c.p.x = bk;
      else if (k == 1) b.c.p.y = bk;
      else b.c.z = bk;
    }
    test_pair01(b, v);
    polish(b, v, paths ? &paths->polishGuard : nullptr);
  }
  if (!closed) {  // rare: at most one pair out of tolerance (a rest state, an axis-aligned flat element), or p2 out of range
    PIES_RARE_PATH();
    Col bc[3], vc[3];
    to_cols(a, bc);
PIES_ROWS_UNROLL
    for (int i = 0; i < 3; ++i) {
      vc[i].p = rp_make(i == 0 ? 1.0f : 0.0f, i == 1 ? 1.0f : 0.0f);
      vc[i].z = i == 2 ? 1.0f : 0.0f;
    }
    if (n01) rotate<0, 1>(bc, vc, s00, s11, s01);
    else if (n02) rotate<0, 2>(bc, vc, s00, s22, s02);
    else if (n12) rotate<1, 2>(bc, vc, s11, s22, s12);
    from_cols(bc, b);
    from_cols(vc, v);
  }
  // The first certifying snapshot, straight-line.  (An element with cnt == 0 has B = A: the snapshot recomputes s00, s11, s22 and the
  // three tests of above from the same operands - clean, with svd3's n = s - so it needs no case of its own.)
  rp n01_ = dot_self(b);
  float n2_ = cdot(b.c, b.c);
  bool clean;
  {
    const rp g2 = dot_with2(b);
    const float g01 = dot_01(b);
    bool t02, t12;
    pair_needs2(n01_, n2_, g2, t02, t12);
    const bool t01 = pair_needs(n01_.x, n01_.y, g01);
    clean = !(int(t02) | int(t12) | int(t01));
  }
  if (!clean) {  // rare: the sweeps of the plain iteration, for the lanes whose snapshot was not clean (on columns)
    PIES_RARE_PATH();
    Col bc[3], vc[3];
    to_cols(b, bc);
    to_cols(v, vc);
    float n0 = n01_.x, n1 = n01_.y, n2 = n2_;
    for (int sweep = 1;; ++sweep) {  // (sweep = the snapshot taken next; svd3's sweep 0 is the one above)
      test_pair<0, 2>(bc, vc);
      test_pair<1, 2>(bc, vc);
      test_pair<0, 1>(bc, vc);
      n0 = cdot(bc[0], bc[0]); n1 = cdot(bc[1], bc[1]); n2 = cdot(bc[2], bc[2]);  // (sweeps exhausted: these are svd3's recomputed norms)
      if (sweep == kMaxSweeps) break;
      const float g02 = cdot(bc[0], bc[2]), g12 = cdot(bc[1], bc[2]), g01 = cdot(bc[0], bc[1]);
      const bool t02 = pair_needs(n0, n2, g02), t12 = pair_needs(n1, n2, g12), t01 = pair_needs(n0, n1, g01);
      clean = !(int(t02) | int(t12) | int(t01));
      if (paths) paths->sweeps = sweep;
      if (clean) break;
    }
    if (paths) { paths->fallback = true; paths->exhausted = !clean; }
    from_cols(bc, b);
    from_cols(vc, v);
    n01_ = rp_make(n0, n1);
    n2_ = n2;
  }
  if (paths) {
    paths->closedForm = closed;
    paths->identity = cnt == 0;
    paths->onePair = cnt == 1;
    paths->rangeOut = cnt >= 2 && !closed;
  }
  // the singular values: columns 0, 1 as one pair chain (a collapsed direction: s = 0, handled by the recomposition)
  const bool ok0 = n01_.x > kTiny2, ok1 = n01_.y > kTiny2, ok2 = n2_ > kTiny2;
  const rp r01 = rsqrt_nr2(rp_make(ok0 ? n01_.x : 1.0f, ok1 ? n01_.y : 1.0f));
  const float r2 = rsqrt_nr(ok2 ? n2_ : 1.0f);
  rsv01 = rp_make(ok0 ? r01.x : 0.0f, ok1 ? r01.y : 0.0f);
  rsv2 = ok2 ? r2 : 0.0f;
  sv01 = rp_mul(n01_, rsv01);
  sv2 = n2_ * rsv2;
}

// complete_t<K, I, J>: t[K] = sg * (u_I x u_J)
template <int K, int I, int J> PIES_ROWS_FN void complete(const Col (&b)[3], const float (&rs)[3], Col (&t)[3], const float sg) {
  const float ui0 = b[I].p.x * rs[I], ui1 = b[I].p.y * rs[I], ui2 = b[I].z * rs[I];
  const float uj0 = b[J].p.x * rs[J], uj1 = b[J].p.y * rs[J], uj2 = b[J].z * rs[J];
  t[K].p = rp_make(sg * (ui1 * uj2 - ui2 * uj1), sg * (ui2 * uj0 - ui0 * uj2));
  t[K].z = sg * (ui0 * uj1 - ui1 * uj0);
}

// svd3_recompose: out[r] = row r of U diag(snew) V^T as (columns 0, 1 | column 2)
PIES_ROWS_FN void recompose(const Mat& b, const Mat& v, const rp s01, const float s2, const rp rs01, const float rs2, const rp snew01,
                            const float snew2, Col (&out)[3], Paths* paths) {
  const bool ok0 = s01.x > kTiny, ok1 = s01.y > kTiny, ok2 = s2 > kTiny;
  const rp gm = rp_mul(snew01, rs01);
  const rp g01 = rp_make(ok0 ? gm.x : 0.0f, ok1 ? gm.y : 0.0f);
  const float g2 = ok2 ? snew2 * rs2 : 0.0f;
  Mat t;
PIES_ROWS_UNROLL
  for (int k = 0; k < 3; ++k) t.r[k] = rp_mul(b.r[k], g01);
  t.c.p = rp_mul(b.c.p, rp_splat(g2));
  t.c.z = b.c.z * g2;
  const int nbad = (ok0 ? 0 : 1) + (ok1 ? 0 : 1) + (ok2 ? 0 : 1);
  if (nbad == 1) {  // rare: a flattened element (on columns)
    PIES_RARE_PATH();
    Col bc[3], tc[3];
    to_cols(b, bc);
    to_cols(t, tc);
    const float rs[3] = {rs01.x, rs01.y, rs2};
    if (!ok0) complete<0, 1, 2>(bc, rs, tc, snew01.x);
    else if (!ok1) complete<1, 2, 0>(bc, rs, tc, snew01.y);
    else complete<2, 0, 1>(bc, rs, tc, snew2);
    from_cols(tc, t);
  }
  if (paths) { paths->completed = nbad == 1; paths->twoCollapsed = nbad >= 2; }
  // V's columns 0, 1 as (rows 0, 1): the one transposition of the common path, two pair moves
  const rp v0 = rp_make(v.r[0].x, v.r[1].x), v1 = rp_make(v.r[0].y, v.r[1].y);
PIES_ROWS_UNROLL
  for (int r = 0; r < 3; ++r) {
    const float t0 = t.r[r].x, t1 = t.r[r].y, t2 = r == 0 ? t.c.p.x : r == 1 ? t.c.p.y : t.c.z;
    out[r].p = rp_fma(rp_splat(t2), v.c.p, rp_fma(rp_splat(t1), v1, rp_mul(rp_splat(t0), v0)));
    out[r].z = rf_fma(t2, v.c.z, rf_fma(t1, v.r[2].y, t0 * v.r[2].x));
  }
}

// An element's rest constants as the projection reads them: Qinv's entries [0][j], [1][j] side by side (they multiply the same
// edge component and give rows 0, 1 of a column of the matrix handed to the SVD), Qinv[2][.], the strain limits and w.
struct Rest {
  rp q0, q1, q2;
  float q20, q21, q22, lo, hi, w;
};
// from a record (pbd_project.h: a0 = Qinv col0 + Qinv[1][0], a1 = Qinv[1][1..2] + Qinv[2][0..1], a2 = Qinv[2][2], min, max, w)
template <class V4> PIES_ROWS_FN Rest rest_of(const V4& a0, const V4& a1, const V4& a2) {
  return Rest{rp_make(a0.x, a0.w), rp_make(a0.y, a1.x), rp_make(a0.z, a1.y), a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
}
// the same record as 12 consecutive floats
PIES_ROWS_FN Rest rest_of(const float* __restrict__ r) {
  return Rest{rp_make(r[0], r[3]), rp_make(r[1], r[4]), rp_make(r[2], r[5]), r[6], r[7], r[8], r[9], r[10], r[11]};
}
// from a row of the rest dictionary as the device holds it (layer_rest.h: layer_rest_row_permute), read as three 4-word pieces:
// every pair is two neighbouring words of a piece, so it arrives as a pair
template <class V4> PIES_ROWS_FN Rest rest_of_row(const V4& r0, const V4& r1, const V4& r2) {
  return Rest{rp_make(r0.x, r0.y), rp_make(r0.z, r0.w), rp_make(r1.x, r1.y), r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
}

// tet_core<0> on node records (any type with x, y, z): TetrahedralConstraint applied as a PBD projection
template <class V4> PIES_ROWS_FN void tet_rows(V4& x1, V4& x2, V4& x3, V4& x4, const Rest& R, Paths* paths = nullptr) {
  // the edges P[j] = x_(j+2) - x1 by component; A[i] = (F[0][i], F[1][i], F[2][i]) with F[c][i] = P[0][i] q[c][0] + P[1][i] q[c][1] +
  // P[2][i] q[c][2] (mat3_mul_cm): column i of the matrix the reference hands to its SVD
  // (the x, y of a record lie side by side: the x and y components of an edge are one pair subtraction, d[j] = (e0[j], e1[j]), and
  // a product takes e0[j] / e1[j] as the pair's low / high half on both rows)
  const rp p1 = rp_make(x1.x, x1.y), p2 = rp_make(x2.x, x2.y), p3 = rp_make(x3.x, x3.y), p4 = rp_make(x4.x, x4.y);
  const rp d[3] = {rp_sub(p2, p1), rp_sub(p3, p1), rp_sub(p4, p1)};
  const float e2[3] = {x2.z - x1.z, x3.z - x1.z, x4.z - x1.z};
  // row c of the matrix, columns 0, 1 = (F[c][0], F[c][1]): the edges' pairs as they are against Qinv[c][j] splatted (a half of a
  // pair of the rest table for c = 0, 1); column 2 = e2[j] splatted against the table's pairs, and one scalar chain
  Mat A;
  A.r[0] = rp_add(rp_add(rp_mul(d[0], rp_splat(R.q0.x)), rp_mul(d[1], rp_splat(R.q1.x))), rp_mul(d[2], rp_splat(R.q2.x)));
  A.r[1] = rp_add(rp_add(rp_mul(d[0], rp_splat(R.q0.y)), rp_mul(d[1], rp_splat(R.q1.y))), rp_mul(d[2], rp_splat(R.q2.y)));
  A.r[2] = rp_add(rp_add(rp_mul(d[0], rp_splat(R.q20)), rp_mul(d[1], rp_splat(R.q21))), rp_mul(d[2], rp_splat(R.q22)));
  A.c.p = rp_add(rp_add(rp_mul(rp_splat(e2[0]), R.q0), rp_mul(rp_splat(e2[1]), R.q1)), rp_mul(rp_splat(e2[2]), R.q2));
  A.c.z = e2[0] * R.q20 + e2[1] * R.q21 + e2[2] * R.q22;
  // det3_cm(F), F[c][i] = row c of column i
  const float f00 = A.r[0].x, f10 = A.r[1].x, f20 = A.r[2].x, f01 = A.r[0].y, f11 = A.r[1].y, f21 = A.r[2].y, f02 = A.c.p.x, f12 = A.c.p.y,
              f22 = A.c.z;
  const float detF = +f00 * (f11 * f22 - f21 * f12) - f10 * (f01 * f22 - f21 * f02) + f20 * (f01 * f12 - f11 * f02);
  Mat B, V;
  rp s01, rs01;
  float s2, rs2;
  svd(A, B, V, s01, s2, rs01, rs2, paths);
  float sn0 = rf_min(rf_max(s01.x, R.lo), R.hi), sn1 = rf_min(rf_max(s01.y, R.lo), R.hi), sn2 = rf_min(rf_max(s2, R.lo), R.hi);
  if (detF < 0.0f) {  // flip the smallest singular value (Constraints.cpp:106-108)
    int k = 0;
    float m = s01.x;
    if (s01.y <= m) { k = 1; m = s01.y; }
    if (s2 <= m) { k = 2; }
    sn0 = (k == 0) ? -sn0 : sn0;
    sn1 = (k == 1) ? -sn1 : sn1;
    sn2 = (k == 2) ? -sn2 : sn2;
  }
  if (paths) paths->flipped = detF < 0.0f;
  Col Fh[3];
  recompose(B, V, s01, s2, rs01, rs2, rp_make(sn0, sn1), sn2, Fh, paths);
  // projected = (0, Fh row 0, Fh row 1, Fh row 2); pos += w * (proj - pos), x and y as a pair
  const float w = R.w;
  const rp w2 = rp_splat(w);
  const rp r1 = rp_add(p1, rp_mul(w2, rp_sub(rp_splat(0.0f), p1)));
  const rp r2 = rp_add(p2, rp_mul(w2, rp_sub(Fh[0].p, p2)));
  const rp r3 = rp_add(p3, rp_mul(w2, rp_sub(Fh[1].p, p3)));
  const rp r4 = rp_add(p4, rp_mul(w2, rp_sub(Fh[2].p, p4)));
  x1.x = r1.x; x1.y = r1.y; x1.z += w * (0.0f - x1.z);
  x2.x = r2.x; x2.y = r2.y; x2.z += w * (Fh[0].z - x2.z);
  x3.x = r3.x; x3.y = r3.y; x3.z += w * (Fh[1].z - x3.z);
  x4.x = r4.x; x4.y = r4.y; x4.z += w * (Fh[2].z - x4.z);
}

}  // namespace rows
}  // namespace pies
