// Schedule LAYERED: the rest dictionary of the tetrahedral container.  The 48 bytes of rest constants of an element (Qinv, min
// strain, max strain, w) are the same for every element of one shape and material; with few distinct sets k_layer keeps them in
// LDS and an element's record is its tc_lid entry alone.  A tile-local node id is below 8 192 (the tile's node records fit LDS),
// so the three high bits of each of the four 16-bit ids carry three bits of a 12-bit set index.  Host and device code.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PIES_REST_HD __host__ __device__ inline
#else
#define PIES_REST_HD inline
#endif

namespace pies {

constexpr uint32_t kLayerRestIdBits = 13;
constexpr uint32_t kLayerRestIdMask = (1u << kLayerRestIdBits) - 1u;  // 8 191
// Sets of one scene at most.  The index has room for 4 096; the table (48 B per set) shares LDS with the node records, and 64 sets
// are 192 float4: one per lane of the narrowest workgroup, so the prologue requests the table with one load per lane.
constexpr uint32_t kLayerRestMaxSets = 64;

// ids[k] <= kLayerRestIdMask, set < 4 096
PIES_REST_HD void layer_rest_pack(const uint32_t ids[4], uint32_t set, uint32_t out[2]) {
  out[0] = (ids[0] | ((set & 7u) << kLayerRestIdBits)) | ((ids[1] | (((set >> 3) & 7u) << kLayerRestIdBits)) << 16);
  out[1] = (ids[2] | (((set >> 6) & 7u) << kLayerRestIdBits)) | ((ids[3] | (((set >> 9) & 7u) << kLayerRestIdBits)) << 16);
}
PIES_REST_HD uint32_t layer_rest_set(uint32_t x, uint32_t y) {
  return ((x >> 13) & 7u) | ((x >> 29) << 3) | (((y >> 13) & 7u) << 6) | ((y >> 29) << 9);
}
// The set index of a scene that takes the dictionary: layer_rest_usable refuses more than kLayerRestMaxSets = 64 sets, so only the
// two 3-bit fields of the first word can be non-zero and the second word need not be read.  (set < 64; the format is unchanged.)
PIES_REST_HD uint32_t layer_rest_set6(uint32_t x) { return ((x >> 13) & 7u) | ((x >> 29) << 3); }
PIES_REST_HD void layer_rest_unpack(const uint32_t in[2], uint32_t ids[4], uint32_t* set) {
  ids[0] = in[0] & kLayerRestIdMask; ids[1] = (in[0] >> 16) & kLayerRestIdMask;
  ids[2] = in[1] & kLayerRestIdMask; ids[3] = (in[1] >> 16) & kLayerRestIdMask;
  *set = layer_rest_set(in[0], in[1]);
}

static_assert(kLayerRestMaxSets <= 64, "layer_rest_set6 reads six bits of the set index");

// A table row in the order of the row-pair form.  A set is 12 floats r[0..11] = Qinv (9, as in tc_q0..2), min strain, max strain, w.  The
// projection on row pairs (tet_rows.h) multiplies (r0, r3), (r1, r4), (r2, r5) as pairs; this order stores each pair side by
// side so that it is one aligned two-word LDS read:  r0 r3 r1 r4 | r2 r5 r6 r7 | r8 r9 r10 r11.
// (pies_finalize uploads the table twice, 3 float4 per set each time: plain, then in this order.  An instantiation of k_layer copies
// the one it reads into LDS.  The per-element arrays tc_q0..2 keep their layout.)
PIES_REST_HD void layer_rest_row_permute(const float plain[12], float row[12]) {
  const uint32_t order[12] = {0, 3, 1, 4, 2, 5, 6, 7, 8, 9, 10, 11};  // order[k] = the plain row's word that stands at word k
  for (int k = 0; k < 12; ++k) row[k] = plain[order[k]];
}

// LDS of a gfx950 workgroup (= of a compute unit): what a host-only handle, which has no device to ask, decides with
constexpr uint32_t kLayerLdsBytes = 160u * 1024u;

// Whether a scene takes the dictionary (all or nothing): `sets` distinct sets over `count` elements, tiles of up to maxGroupNodes
// nodes, ldsBase / ldsDict = the bytes a launch asks for without / with the table, ldsMax = what a workgroup may have (= a compute
// unit's).  The table must be a real compression (the rule of the PD dictionary), the ids must leave their high bits free, and a
// scene whose launches fit a compute unit twice - the four-wavefronts-per-SIMD variants count on that - must still do so.
inline bool layer_rest_usable(uint64_t sets, uint64_t count, uint32_t maxGroupNodes, uint64_t ldsBase, uint64_t ldsDict, uint64_t ldsMax) {
  if (sets == 0 || sets > kLayerRestMaxSets || sets * 16 > count) return false;
  if (maxGroupNodes > kLayerRestIdMask + 1u) return false;
  if (ldsDict > ldsMax) return false;
  if (2 * ldsBase <= ldsMax && 2 * ldsDict > ldsMax) return false;
  return true;
}

}  // namespace pies
