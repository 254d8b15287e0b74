// The rule of pies_apply_ties for one tie, as include/pies_hip.h states it and tests/test_ties.py restates it in numpy.  Included by
// .hip files only; everything is the IEEE sequence written (-ffp-contract=off), every test the positive form, so a NaN anywhere is
// "not live" and "not broken".
#pragma once
#include "tie_kernels.h"
#include "prop_rule.h"

namespace pies {

// the carried point (of positions) or its velocity (of velocities): (b0 * beta0 + b1 * beta1) + b2 * beta2
PIES_DEV V3 tie_carried(V3 b0, V3 b1, V3 b2, const float* beta) { return add(add(scale(b0, beta[0]), scale(b1, beta[1])), scale(b2, beta[2])); }

// W: the tie's share of its nodes' inverse masses under mass splitting (cnt: how many entries of the set each node takes part in)
PIES_DEV float tie_inverse_mass(const TieRecord& R, float wa, float w0, float w1, float w2) {
  const float* b = R.weight;
  return wa * R.cntNode + (((b[0] * b[0]) * (w0 * R.cntTo[0]) + (b[1] * b[1]) * (w1 * R.cntTo[1])) + (b[2] * b[2]) * (w2 * R.cntTo[2]));
}

struct TieSpring {
  float k, a;  // stiffness * strength; c + k h
};
PIES_DEV TieSpring tie_spring(const TieRecord& R, float strength, float h) {
  TieSpring S;
  S.k = R.stiffness * strength;
  const float c = R.damping * strength;
  S.a = c + S.k * h;
  return S;
}
PIES_DEV float tie_den(const TieSpring& S, float h, float W) { return 1.0f + (h * S.a) * W; }

PIES_DEV bool tie_breaks(float stretch, float breakStretch) { return breakStretch > 0.0f && stretch > breakStretch; }
PIES_DEV bool tie_live(bool broken, float strength, float W) { return !broken && strength > 0.0f && W > 0.0f; }

// step 1: the change of J from the relative velocity r = v_a - uq the previous iteration left
PIES_DEV V3 tie_delta(const TieSpring& S, V3 x, V3 r, float h, V3 J, float den) {
  const V3 rho = add(scale(add(scale(x, S.k), scale(r, S.a)), h), J);
  return V3{-(rho.x / den), -(rho.y / den), -(rho.z / den)};
}

}  // namespace pies
