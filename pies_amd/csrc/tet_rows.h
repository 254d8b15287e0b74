// The tetrahedral strain projection of k_layer on ROW PAIRS (gfx950).
//
// The operations and operands are those of tet_core<0> + svd3 + svd3_recompose (pbd_project.h, dev_math.h), one for one: an fmaf is
// an fmaf, a separate multiply and add stay separate, every per-element decision is taken from the element's own data - the
// results are bit for bit the same.  What differs is what stands around the arithmetic:
//
//  * every 3x3 quantity that is updated row by row (A, B = A V, V, the recomposition's t and out, the blend) is held per column as
//    a pair (rows 0, 1) plus a float (row 2), and the row-wise updates - a rotation, the polish, B = A V0, the recomposition, the
//    blend - are written on the pairs.  The pairs exist in the source, so the compiler has packed forms (v_pk_fma_f32 ...)
//    without assembling operands: a pair is only ever formed where its halves are produced side by side (the x, y of a node
//    record, two words of a rest-table row, the result of a pair operation), a scalar coefficient is splatted once and reused,
//    and dot products and all per-element scalar chains read the halves as plain floats.
//  * the rare paths stand behind wave-uniform tests and carry nothing through the common path: the first certifying snapshot
//    is straight-line code and the sweeps of the plain iteration run only when some lane's snapshot is not clean; the start of an
//    element with fewer than two pairs out of tolerance and the completion of a collapsed direction likewise.  A ballot only skips
//    work that no lane needs: no lane's result depends on another lane.
//
// PIES_ROWS_SCALAR (or a host compiler) turns a pair into a struct of two floats: the same code in scalar instructions.  The
// arithmetic compiles for the host (tests/cpp/tet_rows_example.cpp compares it with the oracle's bit for bit); a ballot is then the
// lane's own predicate.  Used by k_layer only: k_tet, k_wave and the experiment variants keep tet_core.
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
PIES_ROWS_FN bool any_lane(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }  // (wave-uniform)
#else
inline float rf_fma(float a, float b, float c) { return std::fmaf(a, b, c); }
inline float rf_abs(float a) { return std::fabs(a); }
inline float rf_min(float a, float b) { return std::fmin(a, b); }
inline float rf_max(float a, float b) { return std::fmax(a, b); }
inline float rf_copysign(float a, float b) { return std::copysign(a, b); }
inline int rf_bits(float a) { int32_t i; std::memcpy(&i, &a, 4); return i; }
inline float rf_float(int a) { float f; std::memcpy(&f, &a, 4); return f; }
inline bool any_lane(bool p) { return p; }
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
// jacobi_pair<P, Q>: the test, and the rotation behind a wave-uniform branch
template <int P, int Q> PIES_ROWS_FN void test_pair(Col (&b)[3], Col (&v)[3]) {
  const float alpha = cdot(b[P], b[P]);
  const float beta = cdot(b[Q], b[Q]);
  const float gamma = cdot(b[P], b[Q]);
  const bool need = pair_needs(alpha, beta, gamma);
  if (!any_lane(need)) return;
  if (need) rotate<P, Q>(b, v, alpha, beta, gamma);
}
// jacobi_polish
PIES_ROWS_FN void polish(Col (&b)[3], Col (&v)[3], bool* guarded = nullptr) {
  const float n0 = cdot(b[0], b[0]), n1 = cdot(b[1], b[1]), n2 = cdot(b[2], b[2]);
  const float g01 = cdot(b[0], b[1]), g02 = cdot(b[0], b[2]), g12 = cdot(b[1], b[2]);
  float t01 = g01 * recip_rough(n1 - n0), t02 = g02 * recip_rough(n2 - n0), t12 = g12 * recip_rough(n2 - n1);
  if (guarded) *guarded = !(rf_abs(t01) <= 3.0e38f) || !(rf_abs(t02) <= 3.0e38f) || !(rf_abs(t12) <= 3.0e38f);  // (the host test's statistics: equal norms, inf or NaN)
  if (!(rf_abs(t01) < 2.5e-4f)) t01 = 0.0f;  // (also NaN: equal norms)
  if (!(rf_abs(t02) < 2.5e-4f)) t02 = 0.0f;
  if (!(rf_abs(t12) < 2.5e-4f)) t12 = 0.0f;
  const rp p01 = rp_splat(t01), p02 = rp_splat(t02), p12 = rp_splat(t12);
  const rp m01 = rp_splat(-t01), m02 = rp_splat(-t02), m12 = rp_splat(-t12);
  const Col x = b[0], y = b[1], z = b[2];
  b[0].p = rp_fma(m02, z.p, rp_fma(m01, y.p, x.p));
  b[0].z = rf_fma(-t02, z.z, rf_fma(-t01, y.z, x.z));
  b[1].p = rp_fma(m12, z.p, rp_fma(p01, x.p, y.p));
  b[1].z = rf_fma(-t12, z.z, rf_fma(t01, x.z, y.z));
  b[2].p = rp_fma(p12, y.p, rp_fma(p02, x.p, z.p));
  b[2].z = rf_fma(t12, y.z, rf_fma(t02, x.z, z.z));
  const Col vx = v[0], vy = v[1], vz = v[2];
  v[0].p = rp_fma(m02, vz.p, rp_fma(m01, vy.p, vx.p));
  v[0].z = rf_fma(-t02, vz.z, rf_fma(-t01, vy.z, vx.z));
  v[1].p = rp_fma(m12, vz.p, rp_fma(p01, vx.p, vy.p));
  v[1].z = rf_fma(-t12, vz.z, rf_fma(t01, vx.z, vy.z));
  v[2].p = rp_fma(p12, vy.p, rp_fma(p02, vx.p, vz.p));
  v[2].z = rf_fma(t12, vy.z, rf_fma(t02, vx.z, vz.z));
}

// which paths an element took (the host test counts them; the device passes nullptr and the bookkeeping folds away)
struct Paths {
  bool closedForm = false, identity = false, onePair = false, rangeOut = false, fallback = false, exhausted = false;
  bool completed = false, twoCollapsed = false, flipped = false, polishGuard = false;
  int sweeps = 0;
};

// The decomposition A V = B of svd3: a[i] = column i of the matrix (= what svd3 calls A[i]).  s[i] = |b_i|, rs[i] = 1 / |b_i|.
PIES_ROWS_FN void svd(const Col (&a)[3], Col (&b)[3], Col (&v)[3], float (&s)[3], float (&rs)[3], Paths* paths) {
  const float s00 = cdot(a[0], a[0]), s11 = cdot(a[1], a[1]), s22 = cdot(a[2], a[2]);
  const float s01 = cdot(a[0], a[1]), s02 = cdot(a[0], a[2]), s12 = cdot(a[1], a[2]);
  const bool n01 = pair_needs(s00, s11, s01), n02 = pair_needs(s00, s22, s02), n12 = pair_needs(s11, s22, s12);
  const int cnt = (n01 ? 1 : 0) + (n02 ? 1 : 0) + (n12 ? 1 : 0);
  // (straight-line: consumed only where cnt >= 2, where svd3 computes the same values)
  const float q = ((s00 + s11) + s22) * 0.333333343f;
  const float d0 = s00 - q, d1 = s11 - q, d2 = s22 - q;
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
    const float m00 = s00 - lam, m11 = s11 - lam, m22 = s22 - lam;
    const float c00 = rf_fma(m11, m22, -(s12 * s12)), c11 = rf_fma(m00, m22, -(s02 * s02)), c22 = rf_fma(m00, m11, -(s01 * s01));
    const float c01 = rf_fma(s02, s12, -(s01 * m22)), c02 = rf_fma(s01, s12, -(s02 * m11)), c12 = rf_fma(s01, s02, -(s12 * m00));
    const float a0 = rf_abs(c00), a1 = rf_abs(c11), a2 = rf_abs(c22);
    const bool k0 = a0 >= a1 && a0 >= a2, k1 = !k0 && a1 >= a2;
    const float v0 = k0 ? c00 : (k1 ? c01 : c02), v1 = k0 ? c01 : (k1 ? c11 : c12), v2 = k0 ? c02 : (k1 ? c12 : c22);
    const float n2 = rf_fma(v2, v2, rf_fma(v1, v1, v0 * v0));
    const bool okn = n2 > kTiny2;
    const float in = rsqrt_nr(okn ? n2 : 1.0f);
    const float nx = okn ? v0 * in : 0.0f, ny = okn ? v1 * in : 0.0f, nz = okn ? v2 * in : 1.0f;
    const float sg = rf_copysign(1.0f, nz);
    const float aa = -recip12(rf_abs(nz) + 1.0f) * sg;  // -1 / (sg + nz)
    const float bb = (nx * ny) * aa;
    // V0 = [t1, t2, n]: the one place where a frame's rows 0, 1 are paired from per-element scalars
    v[0].p = rp_make(rf_fma(sg * nx, nx * aa, 1.0f), sg * bb);
    v[0].z = -(sg * nx);
    v[1].p = rp_make(bb, rf_fma(ny, ny * aa, sg));
    v[1].z = -ny;
    v[2].p = rp_make(nx, ny);
    v[2].z = nz;
PIES_ROWS_UNROLL
    for (int i = 0; i < 3; ++i) {  // B = A V0, row pairs against splatted entries of V0
      const float vi0 = v[i].p.x, vi1 = v[i].p.y, vi2 = v[i].z;
      b[i].p = rp_fma(a[2].p, rp_splat(vi2), rp_fma(a[1].p, rp_splat(vi1), rp_mul(a[0].p, rp_splat(vi0))));
      b[i].z = rf_fma(a[2].z, vi2, rf_fma(a[1].z, vi1, a[0].z * vi0));
    }
    test_pair<0, 1>(b, v);
    polish(b, v, paths ? &paths->polishGuard : nullptr);
  }
  if (any_lane(!closed)) {  // rare: at most one pair out of tolerance (a rest state, an axis-aligned flat element), or p2 out of range
    if (!closed) {
      PIES_RARE_PATH();
PIES_ROWS_UNROLL
      for (int i = 0; i < 3; ++i) {
        b[i] = a[i];
        v[i].p = rp_make(i == 0 ? 1.0f : 0.0f, i == 1 ? 1.0f : 0.0f);
        v[i].z = i == 2 ? 1.0f : 0.0f;
      }
      if (n01) rotate<0, 1>(b, v, s00, s11, s01);
      else if (n02) rotate<0, 2>(b, v, s00, s22, s02);
      else if (n12) rotate<1, 2>(b, v, s11, s22, s12);
    }
  }
  // The first certifying snapshot, straight-line.  (An element with cnt == 0 has B = A: the snapshot recomputes s00, s11, s22 and the
  // three tests of above from the same operands - clean, with svd3's n = s - so it needs no case of its own.)
  float n0 = cdot(b[0], b[0]), n1 = cdot(b[1], b[1]), n2 = cdot(b[2], b[2]);
  bool clean;
  {
    const float g02 = cdot(b[0], b[2]), g12 = cdot(b[1], b[2]), g01 = cdot(b[0], b[1]);
    const bool t02 = pair_needs(n0, n2, g02), t12 = pair_needs(n1, n2, g12), t01 = pair_needs(n0, n1, g01);
    clean = !(int(t02) | int(t12) | int(t01));
  }
  if (any_lane(!clean)) {  // rare: the sweeps of the plain iteration, for the lanes whose snapshot was not clean
    if (!clean) {
      PIES_RARE_PATH();
      for (int sweep = 1;; ++sweep) {  // (sweep = the snapshot taken next; svd3's sweep 0 is the one above)
        test_pair<0, 2>(b, v);
        test_pair<1, 2>(b, v);
        test_pair<0, 1>(b, v);
        n0 = cdot(b[0], b[0]); n1 = cdot(b[1], b[1]); n2 = cdot(b[2], b[2]);  // (sweeps exhausted: these are svd3's recomputed norms)
        if (sweep == kMaxSweeps) break;
        const float g02 = cdot(b[0], b[2]), g12 = cdot(b[1], b[2]), g01 = cdot(b[0], b[1]);
        const bool t02 = pair_needs(n0, n2, g02), t12 = pair_needs(n1, n2, g12), t01 = pair_needs(n0, n1, g01);
        clean = !(int(t02) | int(t12) | int(t01));
        if (paths) paths->sweeps = sweep;
        if (clean) break;
      }
      if (paths) { paths->fallback = true; paths->exhausted = !clean; }
    }
  }
  if (paths) {
    paths->closedForm = closed;
    paths->identity = cnt == 0;
    paths->onePair = cnt == 1;
    paths->rangeOut = cnt >= 2 && !closed;
  }
  const float nn[3] = {n0, n1, n2};
PIES_ROWS_UNROLL
  for (int i = 0; i < 3; ++i) {
    const bool ok = nn[i] > kTiny2;
    const float r = rsqrt_nr(ok ? nn[i] : 1.0f);
    rs[i] = ok ? r : 0.0f;  // a collapsed direction: s = 0, handled by the recomposition
    s[i] = nn[i] * rs[i];
  }
}

// complete_t<K, I, J>: t[K] = sg * (u_I x u_J)
template <int K, int I, int J> PIES_ROWS_FN void complete(const Col (&b)[3], const float (&rs)[3], Col (&t)[3], const float sg) {
  const float ui0 = b[I].p.x * rs[I], ui1 = b[I].p.y * rs[I], ui2 = b[I].z * rs[I];
  const float uj0 = b[J].p.x * rs[J], uj1 = b[J].p.y * rs[J], uj2 = b[J].z * rs[J];
  t[K].p = rp_make(sg * (ui1 * uj2 - ui2 * uj1), sg * (ui2 * uj0 - ui0 * uj2));
  t[K].z = sg * (ui0 * uj1 - ui1 * uj0);
}

// svd3_recompose: out[r] = row r of U diag(snew) V^T as (columns 0, 1 | column 2)
PIES_ROWS_FN void recompose(const Col (&b)[3], const Col (&v)[3], const float (&s)[3], const float (&rs)[3], const float (&snew)[3],
                            Col (&out)[3], Paths* paths) {
  const bool ok0 = s[0] > kTiny, ok1 = s[1] > kTiny, ok2 = s[2] > kTiny;
  const float g0 = ok0 ? snew[0] * rs[0] : 0.0f;
  const float g1 = ok1 ? snew[1] * rs[1] : 0.0f;
  const float g2 = ok2 ? snew[2] * rs[2] : 0.0f;
  Col t[3];
  t[0].p = rp_mul(b[0].p, rp_splat(g0)); t[0].z = b[0].z * g0;
  t[1].p = rp_mul(b[1].p, rp_splat(g1)); t[1].z = b[1].z * g1;
  t[2].p = rp_mul(b[2].p, rp_splat(g2)); t[2].z = b[2].z * g2;
  const int nbad = (ok0 ? 0 : 1) + (ok1 ? 0 : 1) + (ok2 ? 0 : 1);
  if (any_lane(nbad == 1)) {  // rare: a flattened element
    if (nbad == 1) {
      PIES_RARE_PATH();
      if (!ok0) complete<0, 1, 2>(b, rs, t, snew[0]);
      else if (!ok1) complete<1, 2, 0>(b, rs, t, snew[1]);
      else complete<2, 0, 1>(b, rs, t, snew[2]);
    }
  }
  if (paths) { paths->completed = nbad == 1; paths->twoCollapsed = nbad >= 2; }
  out[0].p = rp_fma(rp_splat(t[2].p.x), v[2].p, rp_fma(rp_splat(t[1].p.x), v[1].p, rp_mul(rp_splat(t[0].p.x), v[0].p)));
  out[0].z = rf_fma(t[2].p.x, v[2].z, rf_fma(t[1].p.x, v[1].z, t[0].p.x * v[0].z));
  out[1].p = rp_fma(rp_splat(t[2].p.y), v[2].p, rp_fma(rp_splat(t[1].p.y), v[1].p, rp_mul(rp_splat(t[0].p.y), v[0].p)));
  out[1].z = rf_fma(t[2].p.y, v[2].z, rf_fma(t[1].p.y, v[1].z, t[0].p.y * v[0].z));
  out[2].p = rp_fma(rp_splat(t[2].z), v[2].p, rp_fma(rp_splat(t[1].z), v[1].p, rp_mul(rp_splat(t[0].z), v[0].p)));
  out[2].z = rf_fma(t[2].z, v[2].z, rf_fma(t[1].z, v[1].z, t[0].z * v[0].z));
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
  const float e0[3] = {d[0].x, d[1].x, d[2].x};
  const float e1[3] = {d[0].y, d[1].y, d[2].y};
  const float e2[3] = {x2.z - x1.z, x3.z - x1.z, x4.z - x1.z};
  Col A[3];
  A[0].p = rp_add(rp_add(rp_mul(rp_splat(e0[0]), R.q0), rp_mul(rp_splat(e0[1]), R.q1)), rp_mul(rp_splat(e0[2]), R.q2));
  A[1].p = rp_add(rp_add(rp_mul(rp_splat(e1[0]), R.q0), rp_mul(rp_splat(e1[1]), R.q1)), rp_mul(rp_splat(e1[2]), R.q2));
  // (A[0].z, A[1].z) = e0[j], e1[j] against Qinv[2][j]: the edges' pairs as they are
  const rp z01 = rp_add(rp_add(rp_mul(d[0], rp_splat(R.q20)), rp_mul(d[1], rp_splat(R.q21))), rp_mul(d[2], rp_splat(R.q22)));
  A[0].z = z01.x;
  A[1].z = z01.y;
  A[2].p = rp_add(rp_add(rp_mul(rp_splat(e2[0]), R.q0), rp_mul(rp_splat(e2[1]), R.q1)), rp_mul(rp_splat(e2[2]), R.q2));
  A[2].z = e2[0] * R.q20 + e2[1] * R.q21 + e2[2] * R.q22;
  // det3_cm(F), F[c][r] = row c of A[r]
  const float f00 = A[0].p.x, f10 = A[0].p.y, f20 = A[0].z, f01 = A[1].p.x, f11 = A[1].p.y, f21 = A[1].z, f02 = A[2].p.x, f12 = A[2].p.y,
              f22 = A[2].z;
  const float detF = +f00 * (f11 * f22 - f21 * f12) - f10 * (f01 * f22 - f21 * f02) + f20 * (f01 * f12 - f11 * f02);
  Col B[3], V[3];
  float s[3], rs[3];
  svd(A, B, V, s, rs, paths);
  float sn[3];
PIES_ROWS_UNROLL
  for (int i = 0; i < 3; ++i) sn[i] = rf_min(rf_max(s[i], R.lo), R.hi);
  if (detF < 0.0f) {  // flip the smallest singular value (Constraints.cpp:106-108)
    int k = 0;
    float m = s[0];
    if (s[1] <= m) { k = 1; m = s[1]; }
    if (s[2] <= m) { k = 2; }
    sn[0] = (k == 0) ? -sn[0] : sn[0];
    sn[1] = (k == 1) ? -sn[1] : sn[1];
    sn[2] = (k == 2) ? -sn[2] : sn[2];
  }
  if (paths) paths->flipped = detF < 0.0f;
  Col Fh[3];
  recompose(B, V, s, rs, sn, Fh, paths);
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
