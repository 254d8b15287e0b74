// follow() (pies_amd/csrc/follow_rule.h) against the three rules it replaced, as they stood in adapt_pair_rounds (patience 3),
// adapt_sort_passes and adapt_nc_rounds (patience 8): grow at once, shrink after `patience` calm synchronisations, else start over.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "follow_rule.h"

static int failures = 0;
#define CHECK(cond) \
  do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// the rule as the three adaptations spelled it out
static bool spelled_out(bool grow, uint32_t want, uint32_t& value, uint32_t& calm, uint32_t patience) {
  uint32_t v = value;
  if (grow) { v = want; calm = 0; }
  else if (want < v) { if (++calm >= patience) { v = want; calm = 0; } }
  else calm = 0;
  if (v != value) { value = v; return true; }
  return false;
}

int main() {
  for (uint32_t patience : {3u, 8u}) {
    uint32_t value = 16, calm = 2;
    CHECK(pies::follow(true, 24, value, calm, patience) && value == 24 && calm == 0);  // grows at once, a calm run is forgotten
    for (uint32_t k = 1; k < patience; ++k) CHECK(!pies::follow(false, 8, value, calm, patience) && value == 24 && calm == k);  // not one earlier
    CHECK(pies::follow(false, 8, value, calm, patience) && value == 8 && calm == 0);  // exactly at `patience`
    calm = patience - 1;
    CHECK(!pies::follow(false, 8, value, calm, patience) && value == 8 && calm == 0);  // want == value clears calm
    calm = patience - 1;
    CHECK(!pies::follow(false, 9, value, calm, patience) && value == 8 && calm == 0);  // more wanted, but no reason to grow: clears calm
    // a grow in the middle of a calm run restarts the count
    value = 32; calm = 0;
    for (uint32_t k = 1; k < patience; ++k) CHECK(!pies::follow(false, 8, value, calm, patience));
    CHECK(pies::follow(true, 40, value, calm, patience) && value == 40 && calm == 0);
    for (uint32_t k = 1; k < patience; ++k) CHECK(!pies::follow(false, 8, value, calm, patience) && value == 40);
    CHECK(pies::follow(false, 8, value, calm, patience) && value == 8);
    // a grow that asks for what is captured already (the caps of the pair and contact rounds) changes nothing
    value = 1024; calm = 1;
    CHECK(!pies::follow(true, 1024, value, calm, patience) && value == 1024 && calm == 0);
  }
  // every short sequence of looks, against the spelled-out rule with each adaptation's own grow condition
  uint32_t seed = 12345;
  auto next = [&] { seed = seed * 1664525u + 1013904223u; return seed >> 24; };
  for (int rule = 0; rule < 3; ++rule) {
    const uint32_t patience = rule == 0 ? 3u : 8u;
    uint32_t a = 8, ca = 0, b = 8, cb = 0;
    for (int i = 0; i < 20000; ++i) {
      const uint32_t seen = next() % 24u;
      // pair rounds: deepest > rounds, want = deepest + 8 in steps of 8; sort passes: want > passes; contact rounds: depth > rounds, want = depth + 2
      const uint32_t want = rule == 0 ? ((seen + 8u + 7u) / 8u) * 8u : rule == 1 ? 1u + seen % 6u : (seen == 0 ? 1u : seen + 2u);
      const bool grow = rule == 1 ? want > a : seen > a;
      CHECK(pies::follow(grow, want, a, ca, patience) == spelled_out(grow, want, b, cb, patience) && a == b && ca == cb);
    }
  }
  if (failures == 0) std::printf("follow rule ok\n");
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
