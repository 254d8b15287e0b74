// The rule of pies_drive_actuators for one actuator, as include/pies_hip.h states it and tests/test_actuators.py restates it in numpy.
// Host-and-device inline functions on plain floats: the kernel (actuator_kernels.hip) and the C++ host program of
// tests/test_actuators_cpp.py call the same text.  Everything is the IEEE sequence written (-ffp-contract=off), every test the
// positive form, so a NaN anywhere is "not live".  Includes nothing of the library.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PIES_ACTUATOR_FN __host__ __device__ inline
#else
#define PIES_ACTUATOR_FN inline
#endif

namespace pies {

constexpr unsigned int kActuatorOffset = 1u;  // PIES_ACTUATOR_OFFSET

// LIVE: the activation is finite (inf - inf and NaN - NaN are NaN, which equals nothing)
PIES_ACTUATOR_FN bool actuator_live(float u) { return u - u == 0.0f; }

// the rest datum a live actuator writes
PIES_ACTUATOR_FN float actuator_rest(float base, float gain, float lo, float hi, unsigned int flags, float u) {
  const float gu = gain * u;
  const float r = (flags & kActuatorOffset) ? base + gu : base * (1.0f + gu);
  return fminf(fmaxf(r, lo), hi);
}

// DISTANCE: the length of the constraint, from its two positions
PIES_ACTUATOR_FN float actuator_length(const float a[3], const float b[3]) {
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return sqrtf(dx * dx + dy * dy + dz * dz);
}

// BEND: the cosine of the dihedral angle as the bend projection forms it before its acos, from the four positions
PIES_ACTUATOR_FN float actuator_cosine(const float x1[3], const float x2[3], const float x3[3], const float x4[3]) {
  const float p2[3] = {x2[0] - x1[0], x2[1] - x1[1], x2[2] - x1[2]};
  const float p3[3] = {x3[0] - x1[0], x3[1] - x1[1], x3[2] - x1[2]};
  const float p4[3] = {x4[0] - x1[0], x4[1] - x1[1], x4[2] - x1[2]};
  const float c[3] = {p2[1] * p3[2] - p3[1] * p2[2], p2[2] * p3[0] - p3[2] * p2[0], p2[0] * p3[1] - p3[0] * p2[1]};
  const float e[3] = {p2[1] * p4[2] - p4[1] * p2[2], p2[2] * p4[0] - p4[2] * p2[0], p2[0] * p4[1] - p4[0] * p2[1]};
  const float lc = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  const float le = sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
  const float n1[3] = {c[0] / lc, c[1] / lc, c[2] / lc};
  const float n2[3] = {e[0] / le, e[1] / le, e[2] / le};
  return n1[0] * n2[0] + n1[1] * n2[1] + n1[2] * n2[2];
}

}  // namespace pies
