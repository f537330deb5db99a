// The arithmetic of the video colour conversion (sjpeg_amd/csrc/yuv_colour_math.h) alone, under AddressSanitizer and
// UndefinedBehaviorSanitizer: tests/test_yuv_colour_cxx.py builds this file by the host compiler.  For each of the
// four sources, over all 2^24 triples (Y, U, V), the header's luma and chroma are held to the contract written with a
// 64-bit floor division that never shifts a negative number; then the end values, and the identity.
#include <stdint.h>
#include <stdio.h>

#include "../../sjpeg_amd/csrc/yuv_colour_math.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static int64_t floor_div(int64_t n, int64_t d) {                   // d > 0
  const int64_t q = n / d;
  return n % d < 0 ? q - 1 : q;
}
static int64_t clamp8(int64_t v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

int main() {
  using namespace sjpeg_internal;
  long triples = 0;
  for (int matrix = 0; matrix < 2; ++matrix) {
    for (int range = 0; range < 2; ++range) {
      const YuvColourTable t = yuv_colour_table(matrix, range);
      CHECK(t.y0 == (range == 1 ? 16 : 0));
      CHECK(t.k[1][0] == 0 && t.k[2][0] == 0);                      // the chroma rows never read luma
      CHECK(yuv_colour_is_identity(matrix, range) == (matrix == 0 && range == 0));
      int64_t lo = 0, hi = 0;
      for (int y = 0; y < 256; ++y) {
        for (int cu = 0; cu < 256; ++cu) {
          for (int cv = 0; cv < 256; ++cv, ++triples) {
            const int64_t u = cu - 128, v = cv - 128;
            const int64_t sy = static_cast<int64_t>(t.k[0][0]) * (y - t.y0) + t.k[0][1] * u + t.k[0][2] * v + 8192;
            const int64_t su = static_cast<int64_t>(t.k[1][1]) * u + t.k[1][2] * v + 8192;
            const int64_t sv = static_cast<int64_t>(t.k[2][1]) * u + t.k[2][2] * v + 8192;
            lo = sy < lo ? sy : lo; hi = sy > hi ? sy : hi;
            const int32_t gy = yuv_colour_luma(t, y, static_cast<int32_t>(u), static_cast<int32_t>(v));
            const int32_t gu = yuv_colour_chroma(t, 1, static_cast<int32_t>(u), static_cast<int32_t>(v));
            const int32_t gv = yuv_colour_chroma(t, 2, static_cast<int32_t>(u), static_cast<int32_t>(v));
            if (gy != clamp8(floor_div(sy, 16384)) || gu != clamp8(128 + floor_div(su, 16384)) || gv != clamp8(128 + floor_div(sv, 16384))) {
              printf("FAILED: matrix %d range %d (%d, %d, %d) -> (%d, %d, %d)\n", matrix, range, y, cu, cv, gy, gu, gv);
              return 1;
            }
            if (matrix == 0 && range == 0) CHECK(gy == y && gu == cu && gv == cv);
          }
        }
      }
      CHECK(lo > -(1ll << 23) && hi < (1ll << 23));                 // every sum fits 32 bits, with room
    }
  }
  // studio black and white, and the clamps
  const YuvColourTable v709 = yuv_colour_table(1, 1), l601 = yuv_colour_table(0, 1);
  CHECK(yuv_colour_luma(v709, 16, 0, 0) == 0 && yuv_colour_luma(v709, 235, 0, 0) == 255);
  CHECK(yuv_colour_luma(l601, 0, 0, 0) == 0 && yuv_colour_luma(l601, 255, 0, 0) == 255 && yuv_colour_luma(l601, 126, 0, 0) == 128);
  CHECK(yuv_colour_chroma(l601, 1, 112, 0) == 255 && yuv_colour_chroma(l601, 1, -112, 0) == 1 && yuv_colour_chroma(l601, 2, 0, -128) == 0);
  CHECK(yuv_colour_floor14(-1) == -1 && yuv_colour_floor14(-16384) == -1 && yuv_colour_floor14(-16385) == -2 && yuv_colour_floor14(16383) == 0);
  printf("yuv colour math ok: %ld triples\n", triples);
  return 0;
}
