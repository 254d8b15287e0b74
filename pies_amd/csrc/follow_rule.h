// How a captured launch count (level launches of the pair order, radix passes of the node grid, friction rounds of the PD node
// contacts) follows what the scene needs, at host synchronisations: it grows at once and shrinks only after `patience`
// synchronisations in a row at which less would have done.  Host arithmetic only: no HIP header.
#pragma once
#include <cstdint>

namespace pies {

// `want`: what the last look asks for; `grow`: the caller's own condition for taking it at once.  Returns whether `value` changed.
inline bool follow(bool grow, uint32_t want, uint32_t& value, uint32_t& calm, uint32_t patience) {
  const uint32_t before = value;
  if (grow) { value = want; calm = 0; }
  else if (want < value) { if (++calm >= patience) { value = want; calm = 0; } }
  else calm = 0;
  return value != before;
}

}  // namespace pies
