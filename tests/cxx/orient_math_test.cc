// The eight orientations of sjpeg_amd/csrc/orient_math.h on the host: for every o and every w, h in 1..9, and for
// 65535 x 1 and 1 x 65535, the mapping of the upright picture U onto the stored one R is a bijection, the inverse
// function inverts it, o in {1, 2, 3, 4, 5, 7} is its own inverse while 6 and 8 invert each other, and it equals the
// table of sjpeg_hip.h, written out here a second time.  A stand-alone program; built under -fsanitize=undefined.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "orient_math.h"

using sjpeg_internal::orient_source;
using sjpeg_internal::orient_upright;
using sjpeg_internal::oriented_size;

static long long g_samples = 0;

// the table, once more: U(x, y) = R(sx, sy)
static void table(long long x, long long y, long long w, long long h, int o, long long* sx, long long* sy) {
  switch (o) {
    case 1: *sx = x; *sy = y; break;
    case 2: *sx = w - 1 - x; *sy = y; break;
    case 3: *sx = w - 1 - x; *sy = h - 1 - y; break;
    case 4: *sx = x; *sy = h - 1 - y; break;
    case 5: *sx = y; *sy = x; break;
    case 6: *sx = y; *sy = h - 1 - x; break;
    case 7: *sx = w - 1 - y; *sy = h - 1 - x; break;
    default: *sx = w - 1 - y; *sy = x; break;
  }
}

#define CHECK(c) do { if (!(c)) { printf("FAILED %s (o %d, %u x %u, line %d)\n", #c, o, w, h, __LINE__); return 1; } } while (0)

static int walk(uint32_t w, uint32_t h) {
  static const int kInverse[9] = {0, 1, 2, 3, 4, 5, 8, 7, 6};
  for (int o = 1; o <= 8; ++o) {
    uint32_t uw, uh;
    oriented_size(w, h, o, &uw, &uh);
    CHECK(uw == (o >= 5 ? h : w) && uh == (o >= 5 ? w : h));
    CHECK(sjpeg_internal::orient_transposes(o) == (o >= 5));
    std::vector<uint8_t> hit(static_cast<size_t>(w) * h, 0);
    for (uint32_t y = 0; y < uh; ++y) {
      for (uint32_t x = 0; x < uw; ++x) {
        uint32_t sx, sy, bx, by;
        orient_source(x, y, w, h, o, &sx, &sy);
        CHECK(sx < w && sy < h);
        long long tx, ty;
        table(x, y, w, h, o, &tx, &ty);
        CHECK(tx == sx && ty == sy);
        CHECK(hit[static_cast<size_t>(sy) * w + sx] == 0);          // no stored sample twice: with the count, a bijection
        hit[static_cast<size_t>(sy) * w + sx] = 1;
        orient_upright(sx, sy, w, h, o, &bx, &by);
        CHECK(bx == x && by == y);
        // turning the upright picture by the inverse orientation gives the stored one back
        uint32_t ix, iy;
        orient_source(sx, sy, uw, uh, kInverse[o], &ix, &iy);
        CHECK(ix == x && iy == y);
        ++g_samples;
      }
    }
    for (uint8_t v : hit) CHECK(v == 1);
  }
  return 0;
}

int main() {
  for (uint32_t w = 1; w <= 9; ++w) {
    for (uint32_t h = 1; h <= 9; ++h) {
      if (walk(w, h)) return 1;
    }
  }
  if (walk(65535, 1) || walk(1, 65535)) return 1;
  printf("orient math ok: %lld samples\n", g_samples);
  return 0;
}
