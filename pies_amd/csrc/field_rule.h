// The rule of pies_collide_field_props for one (node, field prop) pair, as include/pies_hip.h states it and tests/test_fields.py
// restates it in numpy.  Included by .hip files only; everything is the IEEE sequence written (-ffp-contract=off), every test the
// positive form, so a NaN anywhere is "not touched".  The response to a touch is prop_respond (prop_rule.h) as it stands: a
// field prop's record begins with a pies_prop_t that holds the motion.
#pragma once
#include "field_kernels.h"
#include "prop_rule.h"

namespace pies {

PIES_DEV float field_lerp(float a, float b, float f) { return a + (b - a) * f; }

// where field prop F pushes a node at p with radius r: the contact normal n and the new position q
PIES_DEV bool field_contact(const FieldPropRecord& F, V3 p, float r, V3& n, V3& q) {
  const float R = F.prop.radius + r;
  const V3 a0 = load3(F.prop.axes), a1 = load3(F.prop.axes + 3), a2 = load3(F.prop.axes + 6);
  const V3 d = sub(p, load3(F.prop.centre));
  const float g0 = (dot(a0, d) - F.origin[0]) / F.cell;
  const float g1 = (dot(a1, d) - F.origin[1]) / F.cell;
  const float g2 = (dot(a2, d) - F.origin[2]) / F.cell;
  const uint32_t d0 = F.dims[0], d1 = F.dims[1];
  if (!(g0 >= 0.0f && g0 < static_cast<float>(d0 - 1u) && g1 >= 0.0f && g1 < static_cast<float>(d1 - 1u) && g2 >= 0.0f &&
        g2 < static_cast<float>(F.dims[2] - 1u)))
    return false;  // outside the lattice (or a NaN)
  const uint32_t i0 = static_cast<uint32_t>(g0), i1 = static_cast<uint32_t>(g1), i2 = static_cast<uint32_t>(g2);  // <= dims - 2
  const float f0 = g0 - static_cast<float>(i0), f1 = g1 - static_cast<float>(i1), f2 = g2 - static_cast<float>(i2);
  // the cell's eight samples, s_abc at (i0 + a, i1 + b, i2 + c): four pairs of neighbours along the fastest axis
  const float* s = F.samples + (static_cast<size_t>(i2) * d1 + i1) * d0 + i0;
  const size_t row = d0, slab = static_cast<size_t>(d0) * d1;
  const float s000 = s[0], s100 = s[1], s010 = s[row], s110 = s[row + 1];
  const float s001 = s[slab], s101 = s[slab + 1], s011 = s[slab + row], s111 = s[slab + row + 1];
  const float m0 = field_lerp(field_lerp(s000, s100, f0), field_lerp(s010, s110, f0), f1);
  const float m1 = field_lerp(field_lerp(s001, s101, f0), field_lerp(s011, s111, f0), f1);
  const float phi = field_lerp(m0, m1, f2);
  if (!(phi < R)) return false;
  const V3 G{field_lerp(field_lerp(s100 - s000, s110 - s010, f1), field_lerp(s101 - s001, s111 - s011, f1), f2),
             field_lerp(field_lerp(s010 - s000, s110 - s100, f0), field_lerp(s011 - s001, s111 - s101, f0), f2),
             field_lerp(field_lerp(s001 - s000, s101 - s100, f0), field_lerp(s011 - s010, s111 - s110, f0), f1)};
  const float GG = dot(G, G);
  V3 nl{0.0f, 1.0f, 0.0f};
  if (GG > 0.0f) {
    const float len = sqrtf(GG);
    nl = V3{G.x / len, G.y / len, G.z / len};
  }
  n = add(add(scale(a0, nl.x), scale(a1, nl.y)), scale(a2, nl.z));
  q = add(p, scale(n, R - phi));
  return true;
}

}  // namespace pies
