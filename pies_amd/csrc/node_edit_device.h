// What a between-tick edit of node state is on the device, shared by k_prop_collide, k_field_collide,
// k_force_evaluate and k_load_evaluate: one lane per HOST node id, one workgroup per tile of kPropTile ids, the call's records
// staged in LDS once and read as wave-wide broadcasts.  First pass, the edit: a lane walks the records in ascending index on its own
// node, reads the velocity when the first record reaches the node and stores on a change only.  Second pass, only when the host
// asked for the reaction (one test, uniform over the workgroup): the changed lanes walk their records again from the state they
// loaded - the same functions on the same operands, the same bits - and prop_tile_sums.h takes the tile's sums in ascending node
// id.  No atomics.  A kernel keeps its __shared__ arrays, its staging and what is particular to its rule.  Included by .hip files
// only.
#pragma once
#include "force_kernels.h"
#include "prop_tile_sums.h"

namespace pies {

static_assert(kPropTile == 256, "the workgroup stage_records (dev_math.h) copies with by default");

PIES_DEV V3 xyz(const float4& a) { return V3{a.x, a.y, a.z}; }

// The lane's node.  A lane past the last node stays (no early return: every lane meets the barriers) and is not movable.
struct EditLane {
  uint32_t h = 0;  // host id
  bool live = false;
  uint32_t i = 0;  // device index
  V3 p{};
  float w = 0.0f;
  bool movable = false;  // w != 0; a kernel may ask for more
  // the velocity the call found, read at the first record that reaches the node (need_velocity)
  V3 v{};
  float velW = 0.0f;
  bool haveVel = false;
};

// (h: a host id below P.nd.n when `live`)
PIES_DEV EditLane edit_lane_at(const PropPass& P, uint32_t h, bool live) {
  EditLane L;
  L.h = h;
  L.live = live;
  if (L.live) {
    L.i = P.inv ? P.inv[L.h] : L.h;
    const float4 p4 = P.nd.pos[L.i];
    L.p = xyz(p4);
    L.w = p4.w;
    L.movable = !(L.w == 0.0f);
  }
  return L;
}
PIES_DEV EditLane edit_lane(const PropPass& P) {
  const uint32_t h = blockIdx.x * kPropTile + threadIdx.x;
  return edit_lane_at(P, h, h < P.nd.n);
}

PIES_DEV void need_velocity(const PropPass& P, EditLane& L) {
  if (L.haveVel) return;
  const float4 v4 = P.nd.vel[L.i];
  L.v = xyz(v4);
  L.velW = v4.w;
  L.haveVel = true;
}

// The body of a collide kernel after its records are staged (records: LDS).  contact(record, p, r, n, q): whether the record's
// shape touches a node at p with radius r, the normal and the new position; prop_of(record): the pies_prop_t prop_respond answers
// for.  A node meets the props in ascending index, each on the state the previous one left; position, previous position and
// velocity are stored on a touch only, and P.nodeProp gets the last prop that touched the node.
template <class Record, class Contact, class PropOf>
PIES_DEV void collide_pass(const PropPass& P, const Record* records, PropTileLds& lds, Contact&& contact, PropOf&& prop_of) {
  const EditLane L = edit_lane(P);
  PropNode N0{};
  if (L.live) {
    N0.p = L.p;
    N0.invMass = L.w;
    N0.r = P.nd.radius[L.i];
  }

  // ---- first pass: the edit ----
  uint64_t touchedBy = 0;
  uint32_t last = PIES_PROP_NONE;
  float velW = 0.0f;
  if (L.movable) {
    PropNode N = N0;
    for (uint32_t k = 0; k < P.nProps; ++k) {
      V3 n, q;
      if (!contact(records[k], N.p, N.r, n, q)) continue;
      if (!touchedBy) {
        const float4 v4 = P.nd.vel[L.i];
        N0.v = N.v = xyz(v4);
        velW = v4.w;
      }
      PropTouch T;
      prop_respond(prop_of(records[k]), n, q, N, T);
      touchedBy |= 1ull << k;
      last = k;
    }
    if (touchedBy) {
      P.nd.pos[L.i] = make_float4(N.p.x, N.p.y, N.p.z, N0.invMass);
      P.nd.prev[L.i] = make_float4(N.p.x, N.p.y, N.p.z, 0.0f);  // (.w unused: 0 as the predict kernels and the upload write it)
      P.nd.vel[L.i] = make_float4(N.v.x, N.v.y, N.v.z, velW);
    }
  }
  if (P.nodeProp && L.live) P.nodeProp[L.h] = last;
  if (!P.tileMask) return;  // (uniform: a kernel argument)

  // ---- second pass: the tile's set of props and its sums ----
  PropNode N = N0;
  prop_tile_sums(lds, P.tileMask, P.tileSums, P.nProps, touchedBy, [&](uint32_t k, PropTouch& T) {
    V3 n, q;
    (void)contact(records[k], N.p, N.r, n, q);  // the touch of the first pass, once more
    prop_respond(prop_of(records[k]), n, q, N, T);
  });
}

// The body of a velocity edit after its records are staged and its lane is set up.  evaluate(k, dv): the velocity change of record
// k on the lane's (movable) node from the state the call found, false: not affected; it calls need_velocity(P, L) before it reads
// L.v and whenever it returns true.  Every record reads that state, so the walk keeps one sum of changes.  kScratch: the new
// velocity goes to S.newVel[host id] and the wave's ballot of affected lanes to S.affected; otherwise it is stored in place.  The
// reaction of record k is dv / w, its torque taken about centre_of(k).
template <bool kScratch, class Evaluate, class CentreOf>
PIES_DEV void velocity_edit_pass(const PropPass& P, const VelocityScratch& S, PropTileLds& lds, EditLane& L, Evaluate&& evaluate,
                                 CentreOf&& centre_of) {  // (L: evaluate fills its velocity)
  // ---- first pass: the edit ----
  uint64_t affectedBy = 0;
  if (L.movable) {
    V3 sum{0.0f, 0.0f, 0.0f};
    for (uint32_t k = 0; k < P.nProps; ++k) {
      V3 dv;
      if (!evaluate(k, dv)) continue;
      sum = add(sum, dv);
      affectedBy |= 1ull << k;
    }
    if (affectedBy) {
      const V3 v1 = add(L.v, sum);
      if (kScratch) S.newVel[L.h] = make_float4(v1.x, v1.y, v1.z, L.velW);
      else P.nd.vel[L.i] = make_float4(v1.x, v1.y, v1.z, L.velW);
    }
  }
  if (kScratch) {
    const uint64_t ballot = __builtin_amdgcn_ballot_w64(affectedBy != 0);
    if ((threadIdx.x & 63u) == 0) S.affected[blockIdx.x * kForceWaves + (threadIdx.x >> 6)] = ballot;
  }
  if (!P.tileMask) return;  // (uniform: a kernel argument)

  // ---- second pass: the tile's set of records and its sums ----
  prop_tile_sums(lds, P.tileMask, P.tileSums, P.nProps, affectedBy, [&](uint32_t k, PropTouch& T) {
    V3 dv{};
    (void)evaluate(k, dv);  // the change of the first pass, once more
    T.impulse = scale(dv, 1.0f / L.w);
    T.torque = cross(sub(L.p, centre_of(k)), T.impulse);
  });
}

}  // namespace pies
