// The rule of pies_apply_forces for one (node, force) and one (triangle, force) pair, as include/pies_hip.h states it and
// tests/test_forces.py restates it in numpy.  Included by .hip files only; everything is the IEEE sequence written
// (-ffp-contract=off), every test the positive form, so a NaN anywhere is "not affected".
#pragma once
#include "../../include/pies_hip.h"
#include "prop_rule.h"

namespace pies {

PIES_DEV V3 over(V3 a, float k) { return {a.x / k, a.y / k, a.z / k}; }

// the region of force f at x: d = x - centre, dd = d.d, and the falloff there
PIES_DEV bool force_region(const pies_force_t& f, V3 x, V3& d, float& dd, float& fall) {
  d = sub(x, load3(f.centre));
  dd = dot(d, d);
  const float rr = f.radius * f.radius;
  if (!(dd < rr)) return false;
  fall = 1.0f;
  if (f.falloff == PIES_FALLOFF_LINEAR) {
    fall = 1.0f - sqrtf(dd) / f.radius;
  } else if (f.falloff == PIES_FALLOFF_SMOOTH) {
    const float u = 1.0f - dd / rr;
    fall = u * u;
  }
  return true;
}

// dv of a point force (every type but the wind) on a node inside its region (force_region at the node's position gave d, dd and
// fall) with velocity v and invMass w != 0
PIES_DEV bool force_point(const pies_force_t& f, float dt, V3 d, float dd, float fall, V3 v, float w, V3& dv) {
  if (f.type == PIES_FORCE_DRAG) {
    const float k = fminf(f.strength * dt, 1.0f);
    dv = scale(sub(load3(f.vector), v), k * fall);
    return true;
  }
  V3 a = load3(f.vector);
  if (f.type == PIES_FORCE_RADIAL) {
    if (!(dd > 0.0f)) return false;
    a = scale(over(d, sqrtf(dd)), f.strength);
  } else if (f.type == PIES_FORCE_VORTEX) {
    a = scale(cross(a, d), f.strength);
  }
  if (f.flags & PIES_FORCE_IS_FORCE) a = scale(a, w);
  dv = scale(a, fall * dt);
  return true;
}

// whether the triangle a b c contributes to wind f: its unit normal and area * fall (the velocities are not needed to know)
PIES_DEV bool force_wind_face(const pies_force_t& f, V3 a, V3 b, V3 c, V3& n, float& weight) {
  const V3 N = cross(sub(b, a), sub(c, a));
  const float nn = dot(N, N);
  if (!(nn > 0.0f)) return false;
  const float len = sqrtf(nn);
  n = over(N, len);
  const float area = 0.5f * len;
  V3 d;
  float dd, fall;
  if (!force_region(f, over(add(add(a, b), c), 3.0f), d, dd, fall)) return false;
  weight = area * fall;
  return true;
}
// F / 3 of such a triangle, the corners' velocities va vb vc: what every corner receives before its own dt * invMass
PIES_DEV V3 force_wind_third(const pies_force_t& f, V3 n, float weight, V3 va, V3 vb, V3 vc) {
  const V3 rel = sub(load3(f.vector), over(add(add(va, vb), vc), 3.0f));
  const float vn = dot(rel, n);
  const V3 F = scale(add(scale(n, f.strength * vn), scale(sub(rel, scale(n, vn)), f.shear)), weight);
  return over(F, 3.0f);
}

}  // namespace pies
