// sjpeg_amd/csrc/pillow_filter_math.h alone, under AddressSanitizer and UndefinedBehaviorSanitizer
// (tests/test_pillow_filter_cxx.py builds it with the host compiler): the weights of an axis against those
// tests/pillow_filter_model.py computed for a sweep of radii and sigmas (argv[1]: rows of int32 kind, float32 radius,
// uint32 r, ww, fw, passes), the bound the kernel's uint32 relies on for every r <= 63, the sample of a pass at its
// largest, and the unsharp sample against its definition written with a wider type.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../../sjpeg_amd/csrc/pillow_filter_math.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

using namespace sjpeg_internal;

int main(int argc, char** argv) {
  CHECK(argc == 2);
  FILE* f = fopen(argv[1], "rb");
  CHECK(f != nullptr);
  int32_t n = 0;
  CHECK(fread(&n, 4, 1, f) == 1 && n > 1000);
  int skipped = 0, r63 = 0;
  for (int k = 0; k < n; ++k) {
    int32_t kind; float radius; uint32_t want[4];
    CHECK(fread(&kind, 4, 1, f) == 1 && fread(&radius, 4, 1, f) == 1 && fread(want, 4, 4, f) == 4);
    const PillowFilterAxis a = pillow_filter_axis(kind, radius);
    if (a.r != want[0] || a.ww != want[1] || a.fw != want[2] || a.passes != want[3]) {
      printf("kind %d radius %.9g: r %u ww %u fw %u passes %u, the model has %u %u %u %u\n", kind, radius, a.r, a.ww, a.fw, a.passes, want[0], want[1],
             want[2], want[3]);
      return 1;
    }
    skipped += a.passes == 0;
    r63 += a.r == 63;
    if (a.r <= kPillowFilterRadiusMax) CHECK(pillow_filter_axis_bound(a));
  }
  fclose(f);
  CHECK(skipped > 0 && r63 > 0);
  // the worked values
  CHECK(pillow_gaussian_radius(2.0f) == 1.375f && std::fabs(pillow_gaussian_radius(1.0f) - 0.25f) < 1e-6f && std::fabs(pillow_gaussian_radius(63.0f) - 62.496f) < 1e-3f);
  // trap 1: divided in double, 0.3 and 2.7 give another weight
  for (float fr : {0.3f, 2.7f}) {
    uint32_t r, ww, fw;
    pillow_box_weights(fr, &r, &ww, &fw);
    CHECK(ww != (uint32_t)(16777216.0 / ((double)fr * 2.0 + 1.0)));
  }
  // the bound for every r <= 63: whole radii, the floats just above them and just below the next, and a fine sweep;
  // with it the largest sample of a pass is 255 and nothing leaves uint32
  long axes = 0;
  auto hold = [&](float fr) {
    uint32_t r, ww, fw;
    pillow_box_weights(fr, &r, &ww, &fw);
    const PillowFilterAxis a = {r, ww, fw, 1};
    if (!pillow_filter_axis_bound(a)) return false;
    const uint64_t top = (uint64_t)ww * (2 * r + 1) * 255 + (uint64_t)fw * 510 + (1u << 23);
    if (top >> 32 || (uint64_t)ww * (2 * r + 1) + 2 * (uint64_t)fw > (1u << 24)) return false;
    if (pillow_box_sample(ww, fw, (2 * r + 1) * 255, 510) > 255 || pillow_box_sample(ww, fw, 0, 0) != 0) return false;
    ++axes;
    return true;
  };
  for (int r = 0; r <= 63; ++r) {
    CHECK(hold((float)r) || r == 0);
    CHECK(hold(std::nextafterf((float)r, 100.0f)) && hold(std::nextafterf((float)(r + 1), 0.0f)));
  }
  for (float fr = 1e-6f; fr < 64.0f; fr += 0.00137f) CHECK(hold(fr));
  // a constant picture stays constant: the weights sum to 2^24 but for the truncation, which the rounding term covers
  for (float fr : {0.3f, 1.375f, 2.7f, 17.3f, 63.9f}) {
    uint32_t r, ww, fw;
    pillow_box_weights(fr, &r, &ww, &fw);
    for (uint32_t v : {0u, 1u, 128u, 255u}) CHECK(pillow_box_sample(ww, fw, (2 * r + 1) * v, 2 * v) == v);
  }
  // the unsharp sample: strict threshold (trap 3), C's division, both clips
  for (int p = 0; p < 256; ++p) for (int b = 0; b < 256; b += 3) for (int percent : {0, 80, 150, 500, 65535}) for (int threshold : {0, 1, 3, 52, 255}) {
    const long long d = p - b;
    long long want = p;
    if ((d < 0 ? -d : d) > threshold) { want = p + d * percent / 100; want = want < 0 ? 0 : want > 255 ? 255 : want; }
    CHECK(pillow_unsharp_sample(p, b, percent, threshold) == (uint32_t)want);
  }
  CHECK(pillow_unsharp_sample(160, 108, 150, 52) == 160 && pillow_unsharp_sample(160, 108, 150, 51) == 238);
  CHECK(pillow_unsharp_sample(10, 13, 80, 0) == 8);                 // -3 * 80 / 100 = -2 toward zero, not -3
  printf("pillow filter math ok: %d axes equal to the model's, %ld hold the bound\n", n, axes);
  return 0;
}
