// The rule of one node-node visit (Solver.cpp:88-126): node a visits node b, and if they overlap both are pushed apart along
// the line between them and friction works on their relative tangential velocity.  Written once per LANE LAYOUT - all of a visit
// in one lane, one component per lane of a quad, the fifteen divisions dealt to the lanes of a wavefront -, every layout the same
// IEEE operations on the same operands in the reference's statement order (-ffp-contract=off): the same bits.  Included by .hip
// files only (group_resolve.hip, and pair_lists.hip / pair_levels.hip / pair_turns.hip through pair_device.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pies {

#ifndef PIES_DEV
#define PIES_DEV __device__ __forceinline__
#endif

constexpr float kPairShare = 0.85f;          // the part of an overlap one visit takes out (Solver.cpp:107-108)
constexpr float kPairDegenerate = 0.00001f;  // centres nearer than this: the direction is (1, 0, 0) (Solver.cpp:98-101)

struct NodeState {
  float px, py, pz, w, vx, vy, vz, r;  // position, inverse mass, velocity, radius
};

// The friction coefficient of a visit: below the static threshold the nodes stick.  qq() is |q|^2, q the relative tangential
// velocity; it is asked for only under a positive threshold (the usual scene has none, and the norm stays off the visit's chain:
// handed in as a value, the compiler computes it and the square root for every visit).
template <class NormSquared>
PIES_DEV float pair_friction(float friction, float staticThreshold, NormSquared qq) {
  float fr = friction;
  if (staticThreshold > 0.0f)  // sqrt(x) < t is false for every t <= 0
    if (sqrtf(qq()) < staticThreshold) fr = 1.0f;
  return fr;
}

// ---- all of a visit in one lane ---------------------------------------------------------------------------------------
// node a visits node b; b may BE a (a node meets itself, quirk Q3: `other` aliases `node`, so the second update of each line
// sees the first).  Returns whether the pair was resolved.
PIES_DEV bool visit(NodeState& a, NodeState& b, float friction, float staticThreshold) {
  const float dx = b.px - a.px, dy = b.py - a.py, dz = b.pz - a.pz;
  const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
  const float disp = a.r + b.r - dist;
  if (!(disp > 0.0f)) return false;
  float ux = 1.0f, uy = 0.0f, uz = 0.0f;
  if (dist > kPairDegenerate) { ux = dx / dist; uy = dy / dist; uz = dz / dist; }
  const float wSum = a.w + b.w;
  const float sa = kPairShare * -disp, sb = kPairShare * disp;
  const float rx = b.vx - a.vx, ry = b.vy - a.vy, rz = b.vz - a.vz;
  const float rd = rx * ux + ry * uy + rz * uz;
  const float qx = rx - rd * ux, qy = ry - rd * uy, qz = rz - rd * uz;
  const float fr = pair_friction(friction, staticThreshold, [&] { return qx * qx + qy * qy + qz * qz; });
  a.px += ((sa * ux) * a.w) / wSum; a.py += ((sa * uy) * a.w) / wSum; a.pz += ((sa * uz) * a.w) / wSum;
  b.px += ((sb * ux) * b.w) / wSum; b.py += ((sb * uy) * b.w) / wSum; b.pz += ((sb * uz) * b.w) / wSum;
  a.vx += ((-fr * qx) * a.w) / wSum; a.vy += ((-fr * qy) * a.w) / wSum; a.vz += ((-fr * qz) * a.w) / wSum;
  b.vx += ((fr * qx) * b.w) / wSum; b.vy += ((fr * qy) * b.w) / wSum; b.vz += ((fr * qz) * b.w) / wSum;
  return true;
}

// ---- one component per lane of a quad (pair_levels.hip: pair_level4) ------------------------------------------------------
PIES_DEV float quad_lane(float v, int j) {  // the value of lane j (0-3) of the lane's quad
  switch (j) {
    case 0: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x00, 0xf, 0xf, false));
    case 1: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x55, 0xf, 0xf, false));
    case 2: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xaa, 0xf, 0xf, false));
    default: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xff, 0xf, 0xf, false));
  }
}
PIES_DEV float quad_sum3(float t) { return (quad_lane(t, 0) + quad_lane(t, 1)) + quad_lane(t, 2); }  // x + y + z in visit()'s order
struct QuadNode {
  float p, v;  // component k of position and velocity
  float w, r;  // inverse mass, radius (every lane)
};
// node a visits node b (a != b), component k in this lane; the result of the overlap test is the same in the quad's lanes
PIES_DEV bool visit_quad(QuadNode& a, QuadNode& b, int k, float friction, float staticThreshold) {
  const float d = b.p - a.p;
  const float dist = sqrtf(quad_sum3(d * d));
  const float disp = a.r + b.r - dist;
  if (!(disp > 0.0f)) return false;
  float u = k == 0 ? 1.0f : 0.0f;
  if (dist > kPairDegenerate) u = d / dist;
  const float wSum = a.w + b.w;
  const float sa = kPairShare * -disp, sb = kPairShare * disp;
  const float r = b.v - a.v;
  const float rd = quad_sum3(r * u);
  const float q = r - rd * u;
  const float fr = pair_friction(friction, staticThreshold, [&] { return quad_sum3(q * q); });
  a.p += ((sa * u) * a.w) / wSum;
  b.p += ((sb * u) * b.w) / wSum;
  a.v += ((-fr * q) * a.w) / wSum;
  b.v += ((fr * q) * b.w) / wSum;
  return true;
}

// ---- the fifteen divisions of a visit dealt to the lanes of a wavefront (pair_turns.hip: turn_cell; group_resolve.hip) --------
// visit() runs ~350 instructions in one lane, and the orders that resolve one visit after the other per wavefront (a turn of config
// 4: ~20 of them, 15 us of a 45-us level) have 63 lanes idle meanwhile.  Here lane t computes ONE quotient - the three components
// of the direction on lanes 0-2, then the twelve corrections ((coef * vec_k) * mass) / wSum on lanes 0-11 - and the quotients are
// broadcast.
PIES_DEV float lane_value(float v, uint32_t srcLane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), static_cast<int>(srcLane))); }
PIES_DEV float pick3(int k, float x, float y, float z) { return k == 0 ? x : (k == 1 ? y : z); }
// the node lane `src` holds, to every lane
PIES_DEV NodeState lane_node(const NodeState& b, uint32_t src) {
  return NodeState{lane_value(b.px, src), lane_value(b.py, src), lane_value(b.pz, src), lane_value(b.w, src),
                   lane_value(b.vx, src), lane_value(b.vy, src), lane_value(b.vz, src), lane_value(b.r, src)};
}
// the twelve corrections (lanes 0-11 of corr) in the reference's statement order; b may be a
PIES_DEV void wide_apply(NodeState& a, NodeState& b, float corr) {
  a.px += lane_value(corr, 0); a.py += lane_value(corr, 1); a.pz += lane_value(corr, 2);
  b.px += lane_value(corr, 3); b.py += lane_value(corr, 4); b.pz += lane_value(corr, 5);
  a.vx += lane_value(corr, 6); a.vy += lane_value(corr, 7); a.vz += lane_value(corr, 8);
  b.vx += lane_value(corr, 9); b.vy += lane_value(corr, 10); b.vz += lane_value(corr, 11);
}
// node a visits node o, both wave uniform, and the overlap is known (the caller's test): the visit resolves.  self: o is a copy
// of a, and everything is folded into a.  The caller brings o in (lane_node) and writes it out from one lane.  Distance and overlap
// are computed again here from the uniform states (the callers' lanes tested with the same operations on the same operands).
PIES_DEV void visit_wide(NodeState& a, NodeState& o, bool self, float friction, float staticThreshold, int lane) {
  const float dx = o.px - a.px, dy = o.py - a.py, dz = o.pz - a.pz;
  const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
  const float disp = a.r + o.r - dist;
  const int k3 = lane % 3, kind = (lane / 3) & 3;  // kind 0: a's position, 1: o's position, 2: a's velocity, 3: o's velocity
  float ux = 1.0f, uy = 0.0f, uz = 0.0f;
  if (dist > kPairDegenerate) {
    const float quot = pick3(k3, dx, dy, dz) / dist;
    ux = lane_value(quot, 0); uy = lane_value(quot, 1); uz = lane_value(quot, 2);
  }
  const float wSum = a.w + o.w;
  const float sa = kPairShare * -disp, sb = kPairShare * disp;
  const float rx = o.vx - a.vx, ry = o.vy - a.vy, rz = o.vz - a.vz;  // friction works on the velocities as they are before the pair
  const float rd = rx * ux + ry * uy + rz * uz;
  const float qx = rx - rd * ux, qy = ry - rd * uy, qz = rz - rd * uz;
  const float fr = pair_friction(friction, staticThreshold, [&] { return qx * qx + qy * qy + qz * qz; });
  const float vec = kind < 2 ? pick3(k3, ux, uy, uz) : pick3(k3, qx, qy, qz);
  const float coef = kind == 0 ? sa : (kind == 1 ? sb : (kind == 2 ? -fr : fr));
  const float mass = (kind & 1) ? o.w : a.w;
  const float corr = ((coef * vec) * mass) / wSum;
  if (self) wide_apply(a, a, corr);
  else wide_apply(a, o, corr);
}

}  // namespace pies
