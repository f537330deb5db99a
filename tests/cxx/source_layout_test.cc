// The plane arithmetic of sjpeg_amd/csrc/source_layout.h, on the host alone: for every SJPEG_HIP_SRC_* value the
// kernels' three planes and strides that layout_planes() makes of the caller's, with strides of either sign, with and
// without frame strides; where G and B lie (layout_rgb_offsets); the bytes of a row (row_bytes).  The expected values are
// written out: they are what the entry points computed before the formats moved into one table.
//   g++ -std=c++17 -I include -I sjpeg_amd/csrc tests/cxx/source_layout_test.cc -o source_layout_test && ./source_layout_test
#include <stdint.h>
#include <stdio.h>

#include "source_layout.h"

using namespace sjpeg_internal;

namespace {

constexpr uintptr_t P0 = 0x1000000, P1 = 0x1100000, P2 = 0x1200000;
constexpr int64_t kRow[3] = {1024, 512, 256}, kFrame[3] = {65536, 32768, 16384};

struct Plane { uintptr_t at; long long row, frame; };
struct Want {
  Plane plane[3];
  bool rgb_like;
  long long g_off, b_off;        // (rgb_like alone)
  int64_t row17[3];              // row_bytes of the planes that are read at width 17 (0: not read)
};

const Want kWant[kSourceFormats] = {
    /* RGB */ {{{P0, 1024, 65536}, {0, 0, 0}, {0, 0, 0}}, true, 1, 2, {51, 0, 0}},
    /* BGRA */ {{{P0, 1024, 65536}, {0, 0, 0}, {0, 0, 0}}, true, 1, 0, {68, 0, 0}},
    /* RGBA */ {{{P0, 1024, 65536}, {0, 0, 0}, {0, 0, 0}}, true, 1, 2, {68, 0, 0}},
    /* GRAY */ {{{P0, 1024, 65536}, {0, 0, 0}, {0, 0, 0}}, false, 0, 0, {17, 0, 0}},
    /* YUV444 */ {{{P0, 1024, 65536}, {P1, 512, 32768}, {P2, 256, 16384}}, false, 0, 0, {17, 17, 17}},
    /* YUV420 */ {{{P0, 1024, 65536}, {P1, 512, 32768}, {P2, 256, 16384}}, false, 0, 0, {17, 9, 9}},
    /* NV12 */ {{{P0, 1024, 65536}, {P1, 512, 32768}, {P1, 512, 32768}}, false, 0, 0, {17, 18, 0}},
    /* NV21 */ {{{P0, 1024, 65536}, {P1, 512, 32768}, {P1, 512, 32768}}, false, 0, 0, {17, 18, 0}},
    /* RGB_PLANAR */ {{{P0, 1024, 65536}, {P1, 512, 32768}, {P2, 256, 16384}}, true, 0x100000, 0x200000, {17, 17, 17}},
    /* RGB_PLANAR_F32 */ {{{P0, 1024, 65536}, {P1, 512, 32768}, {P2, 256, 16384}}, true, 0x100000, 0x200000, {68, 68, 68}},
    /* RGB_PLANAR_F16 */ {{{P0, 1024, 65536}, {P1, 512, 32768}, {P2, 256, 16384}}, true, 0x100000, 0x200000, {34, 34, 34}},
    /* RGB_PLANAR_BF16 */ {{{P0, 1024, 65536}, {P1, 512, 32768}, {P2, 256, 16384}}, true, 0x100000, 0x200000, {34, 34, 34}},
    /* RGB_F32 */ {{{P0, 1024, 65536}, {P0 + 4, 1024, 65536}, {P0 + 8, 1024, 65536}}, true, 4, 8, {204, 0, 0}},
    /* RGB_F16 */ {{{P0, 1024, 65536}, {P0 + 2, 1024, 65536}, {P0 + 4, 1024, 65536}}, true, 2, 4, {102, 0, 0}},
    /* RGB_BF16 */ {{{P0, 1024, 65536}, {P0 + 2, 1024, 65536}, {P0 + 4, 1024, 65536}}, true, 2, 4, {102, 0, 0}},
    /* RGBA_F32 */ {{{P0, 1024, 65536}, {P0 + 4, 1024, 65536}, {P0 + 8, 1024, 65536}}, true, 4, 8, {268, 0, 0}},
    /* RGBA_F16 */ {{{P0, 1024, 65536}, {P0 + 2, 1024, 65536}, {P0 + 4, 1024, 65536}}, true, 2, 4, {134, 0, 0}},
    /* RGBA_BF16 */ {{{P0, 1024, 65536}, {P0 + 2, 1024, 65536}, {P0 + 4, 1024, 65536}}, true, 2, 4, {134, 0, 0}},
    /* GRAY_F32 */ {{{P0, 1024, 65536}, {P0, 1024, 65536}, {P0, 1024, 65536}}, false, 0, 0, {68, 0, 0}},
    /* GRAY_F16 */ {{{P0, 1024, 65536}, {P0, 1024, 65536}, {P0, 1024, 65536}}, false, 0, 0, {34, 0, 0}},
    /* GRAY_BF16 */ {{{P0, 1024, 65536}, {P0, 1024, 65536}, {P0, 1024, 65536}}, false, 0, 0, {34, 0, 0}},
};

int failures = 0;
void check(bool ok, int format, const char* what, int i, long long got, long long want) {
  if (ok) return;
  ++failures;
  fprintf(stderr, "format %d: %s[%d] is %lld, not %lld\n", format, what, i, got, want);
}

}  // namespace

int main() {
  if (source_layout(-1) != nullptr || source_layout(kSourceFormats) != nullptr) { fprintf(stderr, "a row for a value that is no format\n"); return 1; }
  const void* const plane[3] = {reinterpret_cast<const void*>(P0), reinterpret_cast<const void*>(P1), reinterpret_cast<const void*>(P2)};
  for (int format = 0; format < kSourceFormats; ++format) {
    const SourceLayout* const L = source_layout(format);
    if (L == nullptr || L->format != format) { fprintf(stderr, "format %d: no row\n", format); return 1; }
    const Want& w = kWant[format];
    for (int sign = 1; sign >= -1; sign -= 2) {
      const int64_t row[3] = {sign * kRow[0], sign * kRow[1], sign * kRow[2]}, frame[3] = {sign * kFrame[0], sign * kFrame[1], sign * kFrame[2]};
      // a uniform batch: planes, row strides, frame strides
      const uint8_t* out[3] = {reinterpret_cast<const uint8_t*>(1), reinterpret_cast<const uint8_t*>(1), reinterpret_cast<const uint8_t*>(1)};
      long long out_row[3] = {-7, -7, -7}, out_frame[3] = {-7, -7, -7};
      layout_planes(*L, plane, row, frame, out, out_row, out_frame);
      for (int i = 0; i < 3; ++i) {
        check(reinterpret_cast<uintptr_t>(out[i]) == w.plane[i].at, format, "plane", i, static_cast<long long>(reinterpret_cast<uintptr_t>(out[i])), static_cast<long long>(w.plane[i].at));
        check(out_row[i] == sign * w.plane[i].row, format, "row_stride", i, out_row[i], sign * w.plane[i].row);
        check(out_frame[i] == sign * w.plane[i].frame, format, "frame_stride", i, out_frame[i], sign * w.plane[i].frame);
      }
      // one picture of a ragged batch: no frame strides
      const uint8_t* one[3] = {reinterpret_cast<const uint8_t*>(1), reinterpret_cast<const uint8_t*>(1), reinterpret_cast<const uint8_t*>(1)};
      long long one_row[3] = {-7, -7, -7};
      layout_planes(*L, plane, row, nullptr, one, one_row, nullptr);
      for (int i = 0; i < 3; ++i) {
        check(one[i] == out[i], format, "ragged plane", i, static_cast<long long>(reinterpret_cast<uintptr_t>(one[i])), static_cast<long long>(w.plane[i].at));
        check(one_row[i] == out_row[i], format, "ragged row_stride", i, one_row[i], out_row[i]);
      }
    }
    check(L->rgb_like == w.rgb_like, format, "rgb_like", 0, L->rgb_like, w.rgb_like);
    if (L->rgb_like) {
      long long g = -7, b = -7;
      layout_rgb_offsets(*L, plane, &g, &b);
      check(g == w.g_off, format, "g_off", 0, g, w.g_off);
      check(b == w.b_off, format, "b_off", 0, b, w.b_off);
    }
    for (int i = 0; i < 3; ++i) {
      const int64_t got = i < L->planes ? row_bytes(*L, i, 17) : 0;
      check(got == w.row17[i], format, "row_bytes at width 17", i, got, w.row17[i]);
    }
  }
  if (failures != 0) return 1;
  printf("source_layout_test: %d formats ok\n", kSourceFormats);
  return 0;
}
