// distance_quotient.h (the three quotients of distance_core from one reciprocal) against `/` and sqrtf, bit for bit, on a host.
// The chain takes its reciprocal and square-root seeds as parameters: here the floats nearest to 1/d and to the root and both
// their neighbours (the hardware's seeds are within one unit in the last place).  Inside the range of dq::in_range every quotient must equal `/` with every seed; outside it
// dq::direction must report the fallback and return what `/` gives.  Compiled -ffp-contract=off, as the device code is.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "distance_quotient.h"

namespace {

uint32_t bits(float a) { uint32_t u; std::memcpy(&u, &a, 4); return u; }
float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

struct HostSeed {  // the floats nearest to 1/d and to the root, moved by `rcp` and `sqrt` units in the last place
  int rcp, sqrt;
  static float moved(float s, int off) {
    if (!(std::fabs(s) > 0.0f) || !std::isfinite(s)) return s;
    return from_bits(bits(s) + static_cast<uint32_t>(off));
  }
  float reciprocal(float d) const { return moved(static_cast<float>(1.0 / static_cast<double>(d)), rcp); }
  float root(float x) const { return moved(static_cast<float>(std::sqrt(static_cast<double>(x))), sqrt); }
};
const HostSeed kSeeds[] = {{0, 0}, {-1, -1}, {1, 1}, {-1, 1}, {1, -1}};

// distance_core's direction as it was: `/` and sqrtf
void reference(float dx, float dy, float dz, float& dist, float out[3]) {
  dist = sqrtf(dx * dx + dy * dy + dz * dz);
  out[0] = 1.0f; out[1] = 0.0f; out[2] = 0.0f;
  if (dist > 0.00001f) {
    out[0] = dx / dist;
    out[1] = dy / dist;
    out[2] = dz / dist;
  }
}

bool same(float a, float b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }

long failures = 0, inRange = 0, outOfRange = 0;

// expect: +1 the triple must be in range, -1 it must not be, 0 either
void check(float dx, float dy, float dz, int expect, const char* what) {
  float dist, ref[3];
  reference(dx, dy, dz, dist, ref);
  for (const HostSeed& seed : kSeeds) {
    float u[3], d;
    const bool shared = pies::dq::direction(dx, dy, dz, dx * dx + dy * dy + dz * dz, seed, d, u[0], u[1], u[2]);
    if (&seed == kSeeds) (shared ? inRange : outOfRange) += 1;
    const bool wrongSide = (expect > 0 && !shared) || (expect < 0 && shared);
    if (!same(d, dist) || !same(u[0], ref[0]) || !same(u[1], ref[1]) || !same(u[2], ref[2]) || wrongSide) {
      if (failures++ < 20)
        std::printf("MISMATCH (%s) d = (%a, %a, %a) seeds %+d %+d in range %d (expected %+d): dist %a, (%a, %a, %a) against %a, (%a, %a, %a)\n", what, dx,
                    dy, dz, seed.rcp, seed.sqrt, shared ? 1 : 0, expect, d, u[0], u[1], u[2], dist, ref[0], ref[1], ref[2]);
    }
  }
}

float up(float a) { return std::nextafter(a, std::numeric_limits<float>::infinity()); }
float down(float a) { return std::nextafter(a, -std::numeric_limits<float>::infinity()); }

}  // namespace

int main() {
  using pies::dq::in_range;
  std::mt19937_64 rng(20261021u);
  std::uniform_real_distribution<float> unit(-1.0f, 1.0f), expo(-31.0f, 30.0f), expoApart(-16.0f, 30.0f);
  std::uniform_int_distribution<int> scale(-20, 20), pick(0, 15);

  // ---- 1.2e7 triples inside the range: positions' differences at every scale, components log-uniform over the whole range, zeros
  const long before = inRange;
  for (int i = 0; i < 7000000; ++i) {  // differences of coordinates of one scale, some components zero (axis-aligned pairs)
    const float s = std::ldexp(1.0f, scale(rng));
    float d[3] = {unit(rng) * s, unit(rng) * s, unit(rng) * s};
    const int z = pick(rng);
    if (z < 3) d[z] = 0.0f;
    if (z == 3) d[0] = d[1] = 0.0f;
    if (z == 4) d[1] = -0.0f;
    check(d[0], d[1], d[2], 0, "one scale");
  }
  for (int i = 0; i < 6000000; ++i) {  // every component log-uniform in [2^-31, 2^30], one at least 2^-16 > 1e-5: the quotients span the range
    float d[3];
    for (float& c : d) c = std::copysign(std::exp2(expo(rng)), unit(rng));
    d[i % 3] = std::copysign(std::exp2(expoApart(rng)), unit(rng));
    check(d[0], d[1], d[2], 1, "log-uniform");
  }
  const long sampled = inRange - before;
  if (sampled < 10000000) { std::printf("only %ld of the sampled triples were in range\n", sampled); ++failures; }

  // ---- both sides of every boundary of the range
  const float kMin = pies::dq::kDistMin, kMax = pies::dq::kDistMax, nMin = 0x1p-32f;
  // dist around the 1e-5 threshold: at and below it the direction is (1, 0, 0) and the lane is out of range
  {
    float below = kMin, above = up(kMin);
    for (int k = 0; k < 200; ++k, below = down(below), above = up(above)) {
      check(below, 0.0f, 0.0f, -1, "threshold and below");
      check(0.0f, -above, 0.0f, 1, "above the threshold");
    }
  }
  check(kMin, 0.0f, 0.0f, -1, "threshold");
  check(up(kMin), 0.0f, 0.0f, 1, "threshold + 1");
  check(6.0e-6f, 6.0e-6f, 6.0e-6f, 1, "components below the threshold, dist above");
  check(5.0e-6f, 5.0e-6f, 5.0e-6f, -1, "dist below the threshold");
  // dist around 2^32
  check(down(kMax), 0.0f, 0.0f, 1, "2^32 - 1 ulp");
  check(kMax, 0.0f, 0.0f, -1, "2^32");
  check(up(kMax), 0.0f, 0.0f, -1, "2^32 + 1 ulp");
  check(0x1p31f, 0x1p31f, 0x1p31f, 1, "dist 2^31 sqrt 3");
  check(0x1.8p31f, 0x1.8p31f, 0x1.8p31f, -1, "dist above 2^32");
  // a numerator around 2^-32, beside one that keeps dist above the threshold
  for (float other : {1.0f, 0.001f, 0x1p31f})
    for (float sign : {1.0f, -1.0f}) {
      check(sign * nMin, other, 0.0f, 1, "numerator 2^-32");
      check(sign * up(nMin), 0.0f, other, 1, "numerator 2^-32 + 1 ulp");
      check(sign * down(nMin), other, 0.0f, -1, "numerator 2^-32 - 1 ulp");
      check(other, sign * down(nMin), 0.0f, -1, "numerator 2^-32 - 1 ulp (y)");
      check(other, 0.0f, sign * down(nMin), -1, "numerator 2^-32 - 1 ulp (z)");
      check(sign * 1.0e-20f, other, 0.0f, -1, "numerator 1e-20");
      check(sign * 1.0e-40f, other, other, -1, "subnormal numerator");
      check(sign * std::numeric_limits<float>::denorm_min(), other, 0.0f, -1, "smallest subnormal numerator");
    }
  // zeros of either sign: in range, and each comes out as the zero of its own sign
  for (float other : {1.0f, -0.37f, 3.0e-5f, 0x1p31f}) {
    check(0.0f, other, 0.0f, 1, "+0 numerators");
    check(-0.0f, other, 0.0f, 1, "-0 numerator");
    check(-0.0f, -0.0f, other, 1, "-0 numerators");
    check(other, -0.0f, 0.0f, 1, "-0, +0");
  }
  check(0.0f, 0.0f, 0.0f, -1, "coincident nodes");
  check(-0.0f, -0.0f, -0.0f, -1, "coincident nodes, -0");
  // sums of squares that are subnormal, underflow, approach the overflow, overflow
  check(1.0e-20f, 1.0e-20f, 0.0f, -1, "sum 2e-40 (subnormal)");
  check(1.0e-23f, 0.0f, 0.0f, -1, "sum underflows");
  check(1.0e-18f, 1.0e-19f, 0.0f, -1, "sum 1e-36");
  check(1.0e18f, 1.0e18f, -1.0e18f, -1, "sum 3e36");
  check(1.8e19f, 0.0f, 1.0e-3f, -1, "sum 3.2e38");
  check(1.9e19f, 1.0f, 0.0f, -1, "sum overflows");
  check(3.0e38f, -3.0e38f, 0.0f, -1, "sum overflows");
  // infinities and NaN
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  check(inf, 0.0f, 1.0f, -1, "infinite numerator");
  check(-inf, inf, 1.0f, -1, "infinite numerators");
  check(nan, 0.0f, 1.0f, -1, "NaN numerator");
  check(1.0f, nan, 0.0f, -1, "NaN numerator");
  check(-nan, 1.0f, 1.0f, -1, "NaN numerator, sign set");
  // the test itself, on operands that need no direction
  if (in_range(1.0f, 0.0f, down(nMin), 1.0f) || !in_range(1.0f, 0.0f, nMin, 1.0f) || in_range(nan, 1.0f, 1.0f, 1.0f) || in_range(inf, inf, 0.0f, 0.0f)) {
    std::printf("in_range answers wrongly on its own boundary\n");
    ++failures;
  }

  std::printf("%ld triples in range, %ld out of range, %ld mismatches\n", inRange, outOfRange, failures);
  if (failures) return 1;
  std::printf("distance quotient ok\n");
  return 0;
}
