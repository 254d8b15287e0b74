// layer_rest.h and tet_rows.h, the parts k_layer's tetrahedral colour step leans on, on a host:
//  * layer_rest_set6 (the set index from the record's first word alone) equals layer_rest_set for every set below
//    kLayerRestMaxSets = 64, over the id patterns of tests/test_layer_rest_dict.py::test_pack_round_trip, and differs from it for
//    a set of 64 or more (the invariant is needed: layer_rest_usable refuses such a scene);
//  * a table row in pair order (layer_rest_row_permute) read back as rows::Rest by rest_of_row equals rest_of on the plain row,
//    word for word, for rows whose 12 words are all different.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "layer_rest.h"
#include "tet_rows.h"

namespace {

struct V4 {
  float x, y, z, w;
};

bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

bool same_rest(const pies::rows::Rest& a, const pies::rows::Rest& b) {
  return same(a.q0.x, b.q0.x) && same(a.q0.y, b.q0.y) && same(a.q1.x, b.q1.x) && same(a.q1.y, b.q1.y) && same(a.q2.x, b.q2.x) &&
         same(a.q2.y, b.q2.y) && same(a.q20, b.q20) && same(a.q21, b.q21) && same(a.q22, b.q22) && same(a.lo, b.lo) && same(a.hi, b.hi) &&
         same(a.w, b.w);
}

}  // namespace

int main() {
  using namespace pies;
  int failures = 0;
  const uint32_t patterns[5][4] = {{0, 0, 0, 0}, {8191, 8191, 8191, 8191}, {8191, 0, 8191, 0}, {1, 4097, 4096, 8190}, {5461, 2730, 5461, 2730}};
  for (const auto& ids : patterns) {
    for (uint32_t set = 0; set < 4096; ++set) {
      uint32_t w[2], back[4], set12;
      layer_rest_pack(ids, set, w);
      layer_rest_unpack(w, back, &set12);
      if (set12 != set || std::memcmp(back, ids, sizeof(back)) != 0) { std::printf("round trip: set %u\n", set); ++failures; }
      const uint32_t set6 = layer_rest_set6(w[0]);
      if (set < kLayerRestMaxSets ? set6 != set : set6 == set) { std::printf("set6: set %u gives %u\n", set, set6); ++failures; }
      if (set6 != (set & 63u)) { std::printf("set6: set %u gives %u, not its low six bits\n", set, set6); ++failures; }
    }
  }
  // rows of 12 distinct words (so that a misplaced word shows), signs and a denormal among them
  for (int r = 0; r < 64; ++r) {
    float plain[12], row[12];
    for (int k = 0; k < 12; ++k) plain[k] = (k % 2 ? -1.0f : 1.0f) * (1.0f + 0.0625f * k + 13.0f * r);
    if (r == 7) plain[4] = 1.0e-40f;
    if (r == 9) plain[3] = -0.0f;
    layer_rest_row_permute(plain, row);
    const V4 a0{plain[0], plain[1], plain[2], plain[3]}, a1{plain[4], plain[5], plain[6], plain[7]}, a2{plain[8], plain[9], plain[10], plain[11]};
    const V4 r0{row[0], row[1], row[2], row[3]}, r1{row[4], row[5], row[6], row[7]}, r2{row[8], row[9], row[10], row[11]};
    const rows::Rest want = rows::rest_of(a0, a1, a2), want2 = rows::rest_of(plain), got = rows::rest_of_row(r0, r1, r2);
    if (!same_rest(want, want2) || !same_rest(want, got)) { std::printf("row %d: the pair-ordered row reads back differently\n", r); ++failures; }
    // every pair of the row-pair form is two neighbouring words of the permuted row, on an even word
    if (!(same(row[0], want.q0.x) && same(row[1], want.q0.y) && same(row[2], want.q1.x) && same(row[3], want.q1.y) && same(row[4], want.q2.x) &&
          same(row[5], want.q2.y))) { std::printf("row %d: a pair is not two neighbouring words\n", r); ++failures; }
  }
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("layer rest row ok\n");
  return 0;
}
