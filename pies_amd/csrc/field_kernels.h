// Signed distance fields and field props (pies_add_field_tri_mesh, pies_collide_field_props; extensions): the device side.  A field
// is a lattice of fp32 samples in HBM; a field prop is a rigid placement of one.  The rule for one (node, field prop) pair is
// stated in pies_hip.h and lives in field_rule.h; the edit, the reaction's two-level order and its records are the props'
// (prop_kernels.h, prop_tile_sums.h), and launch_prop_fold folds the tile records of either kernel.  The mesh build adds two
// small kernels around the distance and winding launches of near_kernels.h.  Launch wrappers like kernels.h: no allocation, no
// synchronisation, everything on the caller's stream.
#pragma once
#include "prop_kernels.h"

namespace pies {

constexpr uint32_t kFieldMaxSamples = 1u << 24;
constexpr uint32_t kFieldMaxTriangles = 1u << 24;

// What k_field_collide stages per field prop: the host's record as a pies_prop_t (radius, centre, axes, velocity, angular, pivot,
// friction; shape, end and half are not read), so that prop_respond answers for it as it stands, and the prop's field.
struct FieldPropRecord {
  pies_prop_t prop;
  float origin[3];
  float cell;
  uint32_t dims[3];
  uint32_t spare;
  const float* samples;  // HBM; sample (i, j, k) at (k * dims[1] + j) * dims[0] + i
};
static_assert(sizeof(FieldPropRecord) == 160 && sizeof(FieldPropRecord) % sizeof(uint32_t) == 0, "FieldPropRecord is 40 words without padding");

struct FieldPass {
  PropPass base;  // nd, inv, nProps, tileMask, tileSums, nodeProp as for props; base.props is not read
  const FieldPropRecord* records = nullptr;  // base.nProps records in HBM
};

// One lane per host node id, one workgroup per tile: the records staged in LDS once; a node outside a prop's lattice costs three
// dot products, inside it the cell's eight samples are gathered; velocity read at the first touch; position, previous position
// and velocity stored on a touch only.
void launch_field_collide(hipStream_t st, const FieldPass& P);

// The mesh build.  points[3 s ..]: the local position origin + (float)(i, j, k) * cell of sample s = (k * dims[1] + j) * dims[0] + i.
void launch_field_points(hipStream_t st, const float origin[3], float cell, const uint32_t dims[3], float* points);
// samples[s] = -distance[s] where |winding[s]| > 0.5, else distance[s]
void launch_field_combine(hipStream_t st, uint32_t n, const float* distance, const float* winding, float* samples);

}  // namespace pies
