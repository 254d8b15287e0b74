// The rule of pies_apply_anchors for one node and its anchors, as include/pies_hip.h states it and tests/test_anchors.py restates it
// in numpy.  Included by .hip files only; everything is the IEEE sequence written (-ffp-contract=off), every test the positive
// form, so a NaN anywhere is "not live".
#pragma once
#include "anchor_kernels.h"
#include "prop_rule.h"

namespace pies {

struct AnchorTarget {  // where anchor i's attachment point is and how it moves, and how far the node is from it
  V3 t, arm, u, x;     // arm = t - pivot, x = p - t
  float stretch;
};

PIES_DEV AnchorTarget anchor_target(const pies_anchor_frame_t& f, const float* local, V3 p) {
  AnchorTarget T;
  T.t = add(add(add(load3(f.origin), scale(load3(f.axes), local[0])), scale(load3(f.axes + 3), local[1])), scale(load3(f.axes + 6), local[2]));
  T.arm = sub(T.t, load3(f.pivot));
  T.u = add(load3(f.velocity), cross(load3(f.angular), T.arm));
  T.x = sub(p, T.t);
  T.stretch = sqrtf(dot(T.x, T.x));
  return T;
}

PIES_DEV bool anchor_live(float w, float strength) { return w > 0.0f && strength > 0.0f; }

struct AnchorSpring {
  float a;  // c + k h
  V3 g;     // x k + (v - u) a
};

PIES_DEV AnchorSpring anchor_spring(float stiffness, float damping, float strength, float h, const AnchorTarget& T, V3 v) {
  const float k = stiffness * strength, c = damping * strength;
  AnchorSpring S;
  S.a = c + k * h;
  S.g = add(scale(T.x, k), scale(sub(v, T.u), S.a));
  return S;
}

// e, the velocity change of a node held by springs whose a and g sum to A and G
PIES_DEV V3 anchor_solve(V3 G, float A, float h, float w) {
  const float hw = h * w;
  const float den = 1.0f + hw * A;
  return V3{-((G.x * hw) / den), -((G.y * hw) / den), -((G.z * hw) / den)};
}

PIES_DEV V3 anchor_spring_impulse(const AnchorSpring& S, V3 e, float h) { return scale(add(S.g, scale(e, S.a)), -h); }
PIES_DEV V3 anchor_pin_impulse(V3 u, V3 v, float w) { return scale(sub(u, v), 1.0f / w); }

}  // namespace pies
