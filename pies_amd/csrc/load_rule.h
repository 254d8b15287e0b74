// The rule of pies_apply_surface_loads for one (triangle, load) pair, as include/pies_hip.h states it and tests/test_loads.py
// restates it in numpy.  Included by .hip files only; everything is the IEEE sequence written (-ffp-contract=off), every test the
// positive form, so a NaN anywhere is "not affected".
#pragma once
#include "../../include/pies_hip.h"
#include "force_rule.h"
#include "load_kernels.h"

namespace pies {

// the corners of a triangle as load L reads them: (a, b, c), with PIES_LOAD_INWARD (a, c, b)
PIES_DEV void load_corners(const pies_surface_load_t& L, const uint32_t* id, uint32_t& ia, uint32_t& ib, uint32_t& ic) {
  const bool inward = L.flags & PIES_LOAD_INWARD;
  ia = id[0];
  ib = inward ? id[2] : id[1];
  ic = inward ? id[1] : id[2];
}

// six_t and area_t of a triangle of a range whose first triangle's corner a is o
PIES_DEV void load_measure(V3 o, V3 a, V3 b, V3 c, float& six, float& area) {
  six = dot(sub(a, o), cross(sub(b, o), sub(c, o)));
  const V3 N = cross(sub(b, a), sub(c, a));
  area = 0.5f * sqrtf(dot(N, N));
}

// V_k, A_k and the pressure from the folded sums
PIES_DEV LoadState load_state(const pies_surface_load_t& L, float sixSum, float areaSum) {
  LoadState S;
  S.volume = sixSum / 6.0f;
  S.area = areaSum;
  S.pressure = L.strength;
  S.acts = 1u;
  if (L.type == PIES_LOAD_GAS) {
    S.acts = S.volume > 0.0f ? 1u : 0u;
    S.pressure = L.strength * (L.rest_volume / S.volume - 1.0f);
  }
  return S;
}

// Whether triangle a b c contributes to load L (S.acts is the caller's test): N, nn and the pressure on it.  The velocities are
// not needed to know.
PIES_DEV bool load_face(const pies_surface_load_t& L, const LoadState& S, V3 a, V3 b, V3 c, V3& N, float& nn, float& p) {
  N = cross(sub(b, a), sub(c, a));
  nn = dot(N, N);
  p = S.pressure;
  if (L.type == PIES_LOAD_FLUID) {
    const V3 x = over(add(add(a, b), c), 3.0f);
    const float depth = dot(sub(load3(L.point), x), load3(L.up));
    if (!(depth > 0.0f)) return false;
    p = -(L.strength * depth);
  }
  return nn > 0.0f;
}
// the pressure's F of such a triangle
PIES_DEV V3 load_force(V3 N, float p) { return scale(N, 0.5f * p); }
// ... and with the drag of a PIES_LOAD_FLUID whose drag != 0, the corners' velocities va vb vc
PIES_DEV V3 load_force_drag(const pies_surface_load_t& L, V3 F, float nn, V3 va, V3 vb, V3 vc) {
  const float area = 0.5f * sqrtf(nn);
  const V3 rel = sub(load3(L.velocity), over(add(add(va, vb), vc), 3.0f));
  return add(F, scale(rel, L.drag * area));
}
// what a corner with invMass w receives
PIES_DEV V3 load_share(V3 F, float dt, float w) { return scale(over(F, 3.0f), dt * w); }

}  // namespace pies
