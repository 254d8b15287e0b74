// pies_amd/csrc/actuator_rule.h compiled for the host: the functions the kernel calls, on vectors read from standard input as
// hexadecimal fp32 words, answered as hexadecimal words - tests/test_actuators_cpp.py compares the bits with the numpy restatement
// of the rule on the same vectors.  One query per line:
//   R base gain lo hi flags u      ->  live rest
//   D ax ay az bx by bz            ->  length
//   B 12 words (x1 x2 x3 x4)       ->  cosine
// Exit code 0 on success.
#include "../../pies_amd/csrc/actuator_rule.h"

#include <cstdint>
#include <cstdio>
#include <cstring>

static float word(uint32_t w) {
  float f;
  std::memcpy(&f, &w, sizeof(f));
  return f;
}
static uint32_t bits(float f) {
  uint32_t w;
  std::memcpy(&w, &f, sizeof(w));
  return w;
}

int main() {
  char kind = 0;
  while (std::scanf(" %c", &kind) == 1) {
    uint32_t w[12] = {0};
    const int count = kind == 'R' ? 6 : kind == 'D' ? 6 : kind == 'B' ? 12 : -1;
    if (count < 0) return 2;
    for (int k = 0; k < count; ++k)
      if (std::scanf("%x", &w[k]) != 1) return 3;
    float v[12];
    for (int k = 0; k < 12; ++k) v[k] = word(w[k]);
    if (kind == 'R') {
      const float u = v[5];
      std::printf("%d %08x\n", pies::actuator_live(u) ? 1 : 0, bits(pies::actuator_rest(v[0], v[1], v[2], v[3], w[4], u)));
    } else if (kind == 'D') {
      std::printf("%08x\n", bits(pies::actuator_length(v, v + 3)));
    } else {
      std::printf("%08x\n", bits(pies::actuator_cosine(v, v + 3, v + 6, v + 9)));
    }
  }
  return 0;
}
