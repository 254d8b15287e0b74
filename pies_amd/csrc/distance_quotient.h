// Three quotients by one divisor from ONE reciprocal (distance_core, pbd_project.h).
//
// The compiler's expansion of a correctly rounded `n / d` on gfx950 is: scale both operands (v_div_scale x 2), a reciprocal seed
// (v_rcp_f32, within one unit in the last place), one refinement of the seed, the quotient with two residual corrections, undo the
// scaling (v_div_fmas), patch the special cases (v_div_fixup).  The scaling and the fix-up are the identity when the operands are
// normal and far from the exponent limits; the seed and its refinement depend on the divisor alone.  quotient() is that expansion's
// correction chain for one numerator, reciprocal() the part shared by every numerator of one divisor, and in_range() the per-lane
// test under which leaving the scaling and the fix-up away changes no bit:
//
//   * 1e-5 < d < 2^32 (d = sqrtf(dx dx + dy dy + dz dz); 1e-5 is distance_core's own threshold): the seed, its refinement and every
//     product are normal.  d itself is root(): the square root's expansion without ITS range scaling (for a sum below 2^-96) and
//     special-case patch, which are the identity for the sums this d can come from;
//   * a numerator is a zero, or 2^-32 <= |n| (and |n| <= d (1 + 2^-22) < 2^33, since n n is a term of the sum): the quotient is >= 2^-64
//     in magnitude, so the residuals are multiples of 2^-143 or more and exact (gradual underflow loses nothing), and every rounded
//     result is normal or an exact zero.  Subnormal and tiny numerators, NaN and infinities fail the test.
//   * the residuals are formed as d q - n and enter the next step negated (an operand modifier, no instruction): for a non-zero
//     numerator that is n - d q to the bit, and a zero numerator of either sign comes out as the zero of its own sign - with the
//     residual as fma(-d, q, n) a -0 numerator would come out as +0 and would have to fail the test, at two more instructions per
//     numerator.
//   * the test on the three numerators is one unsigned minimum: (bits << 1) - 1 wraps a zero of either sign to 0xFFFFFFFF and is
//     below 2 bits(2^-32) - 1 exactly for 0 < |n| < 2^-32.
//
// Lanes that fail the test take `/` and sqrtf.  The chain compiles for a host with the seeds as parameters:
// tests/cpp/distance_quotient_example.cpp runs it with the floats nearest to 1/d and to the root and both their neighbours against
// `/` and sqrtf.
#pragma once
#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define PIES_DQ_FN __device__ __forceinline__
#else
#include <cmath>
#include <cstdint>
#include <cstring>
#define PIES_DQ_FN inline
#endif

namespace pies {
namespace dq {

#if defined(__HIP__)
PIES_DQ_FN float dq_fma(float a, float b, float c) { return fmaf(a, b, c); }
PIES_DQ_FN uint32_t dq_bits(float a) { return __float_as_uint(a); }
PIES_DQ_FN float dq_float(uint32_t a) { return __uint_as_float(a); }
PIES_DQ_FN float dq_sqrt(float a) { return sqrtf(a); }
struct HardwareSeed {  // v_rcp_f32, v_sqrt_f32: within one unit in the last place of 1/d, of the root
  PIES_DQ_FN float reciprocal(float d) const { return __builtin_amdgcn_rcpf(d); }
  PIES_DQ_FN float root(float x) const { return __builtin_amdgcn_sqrtf(x); }
};
#else
inline float dq_fma(float a, float b, float c) { return std::fmaf(a, b, c); }
inline uint32_t dq_bits(float a) { uint32_t u; std::memcpy(&u, &a, 4); return u; }
inline float dq_float(uint32_t a) { float f; std::memcpy(&f, &a, 4); return f; }
inline float dq_sqrt(float a) { return std::sqrt(a); }
#endif

constexpr float kDistMin = 0.00001f;          // distance_core's threshold: at or below it the direction is (1, 0, 0)
constexpr float kDistMax = 0x1p+32f;
constexpr uint32_t kNumMinBits = 0x2F800000u;  // 2^-32: smallest magnitude of a numerator that is not a zero

PIES_DQ_FN uint32_t numerator_key(float n) { return (dq_bits(n) << 1) - 1u; }  // (one v_lshl_add_u32)
PIES_DQ_FN uint32_t dq_min3(uint32_t a, uint32_t b, uint32_t c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
// (every float comparison is false for a NaN; an infinite or NaN numerator makes dist infinite or NaN)
PIES_DQ_FN bool in_range(float dist, float dx, float dy, float dz) {
  // (& on purpose: three independent comparisons and two scalar ands, where && becomes a branch per term)
  return (dist > kDistMin) & (dist < kDistMax) & (dq_min3(numerator_key(dx), numerator_key(dy), numerator_key(dz)) >= 2u * kNumMinBits - 1u);
}

// sqrtf(x) for a normal x >= 2^-96 from a seed within one unit in the last place: the compiler's expansion - the seed's two
// neighbours, a residual each, two selects - without the scaling of a smaller x in front and the patch for 0, infinity and NaN
// behind.  For every other x the result is at most 2^-48, an infinity or a NaN, which in_range() turns away.
PIES_DQ_FN float root(float x, float seed) {
  const float below = dq_float(dq_bits(seed) - 1u), above = dq_float(dq_bits(seed) + 1u);
  const float rb = dq_fma(-below, seed, x), ra = dq_fma(-above, seed, x);
  float s = rb <= 0.0f ? below : seed;
  s = ra > 0.0f ? above : s;
  return s;
}
// the seed refined once: what every quotient by d shares
PIES_DQ_FN float reciprocal(float d, float seed) {
  const float e = dq_fma(-d, seed, 1.0f);
  return dq_fma(e, seed, seed);
}
// n / d, correctly rounded for operands in_range() admits; r = reciprocal(d, seed)
PIES_DQ_FN float quotient(float n, float d, float r) {
  const float q0 = n * r;
  const float t0 = dq_fma(d, q0, -n);
  const float q1 = dq_fma(-t0, r, q0);
  const float t1 = dq_fma(d, q1, -n);
  return dq_fma(-t1, r, q1);
}

// dist = sqrtf(sum) and the direction (dx, dy, dz) / dist of distance_core, (1, 0, 0) for dist <= 1e-5.  Returns whether the lane
// was in range.  The chain is computed by every lane - one out of range throws it away (no arithmetic traps) - so the common path is
// straight-line code with one branch around the rare one instead of an if / else, and the selects of the rare path stand inside
// its branch: hoisted in front of it they are on every lane's path.
template <class Seed>
PIES_DQ_FN bool direction(float dx, float dy, float dz, float sum, Seed seed, float& dist, float& ux, float& uy, float& uz) {
  dist = root(sum, seed.root(sum));
  const float r = reciprocal(dist, seed.reciprocal(dist));
  ux = quotient(dx, dist, r);
  uy = quotient(dy, dist, r);
  uz = quotient(dz, dist, r);
  const bool shared = in_range(dist, dx, dy, dz);
  if (!shared) {
    dist = dq_sqrt(sum);
    const bool apart = dist > kDistMin;
    const float qx = dx / dist, qy = dy / dist, qz = dz / dist;
    ux = apart ? qx : 1.0f;
    uy = apart ? qy : 0.0f;
    uz = apart ? qz : 0.0f;
  }
  return shared;
}

}  // namespace dq
}  // namespace pies
