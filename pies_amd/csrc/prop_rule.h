// The rule of pies_collide_props for one (node, prop) pair, as include/pies_hip.h states it and tests/test_props.py restates it in
// numpy.  Included by .hip files only (prop_respond also answers for the field props, field_rule.h); everything is the IEEE
// sequence written (-ffp-contract=off), every test the positive form, so a NaN anywhere is "not touched".
#pragma once
#include "../../include/pies_hip.h"
#include "dev_math.h"
#include "surface_device.h"

namespace pies {

PIES_DEV V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
PIES_DEV V3 scale(V3 a, float k) { return {a.x * k, a.y * k, a.z * k}; }

struct PropNode {  // the state of one node as the props find and leave it
  V3 p, v;
  float invMass, r;
};
struct PropTouch {  // what a touch hands to the sums
  V3 impulse, torque;
};

// the sphere rule: centre c, R = prop.radius + r
PIES_DEV bool prop_sphere_rule(V3 p, V3 c, float R, V3& n, V3& q) {
  const V3 d = sub(p, c);
  const float dd = dot(d, d);
  if (!(dd < R * R)) return false;
  n = V3{0.0f, 1.0f, 0.0f};
  if (dd > 0.0f) {
    const float len = sqrtf(dd);
    n = V3{d.x / len, d.y / len, d.z / len};
  }
  q = add(c, scale(n, R));
  return true;
}

// where prop P pushes a node at p with radius r: the contact normal n and the new position q
PIES_DEV bool prop_contact(const pies_prop_t& P, V3 p, float r, V3& n, V3& q) {
  const float R = P.radius + r;
  const V3 centre = load3(P.centre);
  if (P.shape == PIES_PROP_SPHERE) return prop_sphere_rule(p, centre, R, n, q);
  if (P.shape == PIES_PROP_CAPSULE) {
    const V3 ab = sub(load3(P.end), centre), ap = sub(p, centre);
    const float den = dot(ab, ab);
    const float t = den > 0.0f ? fminf(fmaxf(dot(ap, ab) / den, 0.0f), 1.0f) : 0.0f;
    return prop_sphere_rule(p, add(centre, scale(ab, t)), R, n, q);
  }
  const V3 a0 = load3(P.axes), a1 = load3(P.axes + 3), a2 = load3(P.axes + 6);
  const V3 d = sub(p, centre);
  const float l0 = dot(a0, d), l1 = dot(a1, d), l2 = dot(a2, d);
  const float h0 = P.half[0], h1 = P.half[1], h2 = P.half[2];
  if (fabsf(l0) <= h0 && fabsf(l1) <= h1 && fabsf(l2) <= h2) {
    const float e0 = h0 - fabsf(l0), e1 = h1 - fabsf(l1), e2 = h2 - fabsf(l2);
    float e = e0, l = l0;
    V3 axis = a0;
    if (e1 < e) { e = e1; l = l1; axis = a1; }
    if (e2 < e) { e = e2; l = l2; axis = a2; }
    n = l >= 0.0f ? axis : V3{-axis.x, -axis.y, -axis.z};
    q = add(p, scale(n, e + R));
    return true;
  }
  const float k0 = fminf(fmaxf(l0, -h0), h0), k1 = fminf(fmaxf(l1, -h1), h1), k2 = fminf(fmaxf(l2, -h2), h2);
  const V3 c = add(add(add(centre, scale(a0, k0)), scale(a1, k1)), scale(a2, k2));
  return prop_sphere_rule(p, c, R, n, q);
}

// A touch of prop P (prop_contact gave n and q): N moves to q, its velocity answers relative to the moving prop, and the touch's
// impulse and torque go to T.  The caller has excluded invMass == 0.
PIES_DEV void prop_respond(const pies_prop_t& P, V3 n, V3 q, PropNode& N, PropTouch& T) {
  const V3 arm = sub(q, load3(P.pivot));
  const V3 u = add(load3(P.velocity), cross(load3(P.angular), arm));
  const V3 rel = sub(N.v, u);
  const float vn = dot(rel, n);
  const V3 tang = sub(rel, scale(n, vn));
  const V3 v1 = add(u, add(scale(tang, 1.0f - P.friction), scale(n, fmaxf(vn, 0.0f))));
  T.impulse = scale(sub(N.v, v1), 1.0f / N.invMass);
  T.torque = cross(arm, T.impulse);
  N.p = q;
  N.v = v1;
}

}  // namespace pies
