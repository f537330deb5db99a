// flatten_math_test.cc -- sjpeg_amd/csrc/flatten_math.h against the plain 64-bit division: the division-free / 255 over
// every numerator it is defined for, both formulas over all 2^24 triples (alpha, sample, background), and the end
// values.  Host only; built under UndefinedBehaviorSanitizer by tests/test_flatten_cxx.py.
#include <stdint.h>
#include <stdio.h>

#include "flatten_math.h"

using sjpeg_internal::flatten_byte;
using sjpeg_internal::flatten_div255;
using sjpeg_internal::flatten_premultiplied;
using sjpeg_internal::flatten_straight;

int main() {
  unsigned long long quotients = 0, triples = 0;
  for (uint32_t t = 0; t <= 65535u; ++t, ++quotients) {
    if (flatten_div255(t) != t / 255u) { printf("div255(%u) = %u, not %u\n", t, flatten_div255(t), t / 255u); return 1; }
  }
  uint64_t top = 0;
  for (uint64_t a = 0; a < 256; ++a) {
    for (uint64_t s = 0; s < 256; ++s) {
      for (uint64_t bg = 0; bg < 256; ++bg, ++triples) {
        // straight: the nearest integer to (a s + (255 - a) bg) / 255 -- twice the distance is below 255, so no ties
        const uint64_t num = a * s + (255 - a) * bg, want = (num + 127) / 255;
        if (num + 127 > top) top = num + 127;
        const uint32_t got = flatten_straight(a, s, bg);
        const int64_t twice = 2 * static_cast<int64_t>(got) * 255 - 2 * static_cast<int64_t>(num);
        if (got != want || got > 255 || twice >= 255 || twice <= -255) {
          printf("straight(%d, %d, %d) = %u, not %d\n", (int)a, (int)s, (int)bg, got, (int)want);
          return 1;
        }
        uint64_t pre = s + ((255 - a) * bg + 127) / 255;
        if (pre > 255) pre = 255;
        if (flatten_premultiplied(a, s, bg) != pre) {
          printf("premultiplied(%d, %d, %d) = %u, not %d\n", (int)a, (int)s, (int)bg, flatten_premultiplied(a, s, bg), (int)pre);
          return 1;
        }
        if (flatten_byte(a, s, bg, false) != got || flatten_byte(a, s, bg, true) != pre) { printf("flatten_byte picks the wrong formula\n"); return 1; }
      }
    }
  }
  if (top != 65152) { printf("the largest numerator is %llu, not 65152\n", (unsigned long long)top); return 1; }
  // the end values
  for (uint32_t s = 0; s < 256; ++s) {
    for (uint32_t bg = 0; bg < 256; ++bg) {
      if (flatten_straight(0, s, bg) != bg || flatten_straight(255, s, bg) != s) { printf("straight: an end value is off\n"); return 1; }
      if (flatten_premultiplied(255, s, bg) != s) { printf("premultiplied: opaque is not the sample\n"); return 1; }
      if (flatten_premultiplied(0, s, bg) != (s + bg > 255 ? 255 : s + bg)) { printf("premultiplied: transparent is not sample + background\n"); return 1; }
    }
  }
  if (flatten_premultiplied(0, 255, 255) != 255 || flatten_premultiplied(1, 200, 255) != 255) { printf("premultiplied does not saturate\n"); return 1; }
  printf("flatten math ok: %llu quotients, %llu triples\n", quotients, triples);
  return 0;
}
