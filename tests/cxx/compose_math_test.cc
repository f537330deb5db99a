// compose_math.h alone, under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_compose_cxx.py builds and runs
// it): the blend against its other statement for all 256^3 triples, and that it is NOT the sum of two rounded products;
// the luma's ends; the rounding, half to even; the anchors; the tile count; and ImageOps.contain's sizes and
// ImageOps.pad's places against what tests/compose_model.py computes in Python doubles, read from the file argv[1]
// names: int32 count, then count records of int32 w, h, bw, bh, double cx, cy, int32 w', h', px, py.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../sjpeg_amd/csrc/compose_math.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

using namespace sjpeg_internal;

int main(int argc, char** argv) {
  long long two_products_differ = 0;
  for (uint32_t a = 0; a < 256; ++a) for (uint32_t d = 0; d < 256; ++d) for (uint32_t s = 0; s < 256; ++s) {
    const uint32_t got = compose_blend(d, s, a);
    if (got != (d * (255 - a) + s * a + 127) / 255) { printf("blend(%u, %u, %u) = %u\n", d, s, a, got); return 1; }
    auto mul = [](uint32_t x, uint32_t y) { const uint32_t t = x * y + 128; return ((t >> 8) + t) >> 8; };
    if (got != mul(d, 255 - a) + mul(s, a)) ++two_products_differ;
  }
  CHECK(two_products_differ > 4000000);
  for (uint32_t v = 0; v < 256; ++v) {
    CHECK(compose_blend(v, 77, 0) == v && compose_blend(77, v, 255) == v && compose_luma(v, v, v) == v);
  }
  CHECK(compose_blend(compose_blend(0, 255, 128), 0, 128) == 64 && compose_blend(compose_blend(0, 0, 128), 255, 128) == 128);
  CHECK(compose_luma(255, 0, 0) == 76 && compose_luma(0, 255, 0) == 150 && compose_luma(0, 0, 255) == 29);
  CHECK(compose_round(0.5) == 0 && compose_round(1.5) == 2 && compose_round(2.5) == 2 && compose_round(-0.5) == 0 && compose_round(197.5) == 198);
  long long x, y;
  compose_anchor(0, 10, 8, 4, 2, 1, 2, &x, &y); CHECK(x == 1 && y == 2);
  compose_anchor(1, 10, 8, 4, 2, 1, 2, &x, &y); CHECK(x == 5 && y == 2);
  compose_anchor(2, 10, 8, 4, 2, 1, 2, &x, &y); CHECK(x == 1 && y == 4);
  compose_anchor(3, 10, 8, 4, 2, 1, 2, &x, &y); CHECK(x == 5 && y == 4);
  compose_anchor(4, 10, 8, 4, 2, 1, 2, &x, &y); CHECK(x == 4 && y == 5);
  compose_anchor(4, 4, 3, 7, 8, 0, 0, &x, &y); CHECK(x == -2 && y == -3);          // floor((4 - 7) / 2), floor((3 - 8) / 2)
  compose_anchor(3, 65535, 65535, 1, 1, -2147483647 - 1, 2147483647, &x, &y); CHECK(x == 65534ll + 2147483648ll && y == 65534ll - 2147483647ll);
  CHECK(compose_tiles(1, 1) == 1 && compose_tiles(64, 16) == 1 && compose_tiles(65, 17) == 4 && compose_tiles(226, 40) == 12);
  CHECK(compose_tiles(49152, 65535) == 768ull * 4096ull);
  if (argc < 2) { printf("no file of cases\n"); return 1; }
  FILE* f = fopen(argv[1], "rb");
  CHECK(f != nullptr);
  int32_t n = 0;
  CHECK(fread(&n, 4, 1, f) == 1 && n > 0);
  for (int i = 0; i < n; ++i) {
    struct { int32_t w, h, bw, bh; double cx, cy; int32_t ow, oh, px, py; } r;
    static_assert(sizeof(r) == 48, "the record");
    CHECK(fread(&r, sizeof(r), 1, f) == 1);
    long long ow, oh;
    compose_contain_size(r.w, r.h, r.bw, r.bh, &ow, &oh);
    if (ow != r.ow || oh != r.oh) { printf("contain %dx%d in %dx%d: %lldx%lld, the model %dx%d\n", r.w, r.h, r.bw, r.bh, ow, oh, r.ow, r.oh); return 1; }
    if (ow < 1 || oh < 1) continue;
    const long long px = compose_pad_offset(r.bw, (int)ow, r.cx), py = compose_pad_offset(r.bh, (int)oh, r.cy);
    if (px != r.px || py != r.py) { printf("pad %dx%d in %dx%d: (%lld, %lld), the model (%d, %d)\n", r.w, r.h, r.bw, r.bh, px, py, r.px, r.py); return 1; }
  }
  fclose(f);
  printf("compose math ok: %d sizes and places equal to the model's\n", n);
  return 0;
}
