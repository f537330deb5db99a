// compose_math.h -- the arithmetic of the compose stage (sjpeg_hip_compose_ragged_src and the _composed_ entries;
// compose.hip, compose_plan.cc), stated once for the kernel, the host and the tests: Pillow 12.2.0's paste of an RGBA
// overlay with itself as mask, its conversion of the overlay's colour for a gray base, ImageOps.contain's size,
// ImageOps.pad's place and the anchors of an overlay place.  Integers per sample, one right answer; the two rules of
// size and place are double work done once on the host.  Plain C++ (a host compiler reads it as it is:
// tests/cxx/compose_math_test.cc).
#ifndef SJPEG_AMD_COMPOSE_MATH_H_
#define SJPEG_AMD_COMPOSE_MATH_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SJPEG_COMPOSE_HD __host__ __device__
#else
#define SJPEG_COMPOSE_HD
#endif

namespace sjpeg_internal {

constexpr int kComposePlacesMax = 8;              // overlay places one frame may have
constexpr int kComposeAnchors = 5;                // top-left, top-right, bottom-left, bottom-right, centre

// out = (dst * (255 - a) + src * a + 127) / 255, as Pillow computes it: NOT the sum of two rounded products.
// a = 0 leaves dst, a = 255 gives src.
SJPEG_COMPOSE_HD inline uint32_t compose_blend(uint32_t dst, uint32_t src, uint32_t a) {
  const uint32_t t = dst * (255u - a) + src * a + 128u;
  return ((t >> 8) + t) >> 8;
}

// the overlay's colour on a gray base: Pillow's convert("L")
SJPEG_COMPOSE_HD inline uint32_t compose_luma(uint32_t r, uint32_t g, uint32_t b) {
  return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16;
}

// Python's round() of a double: half to even -- C's nearbyint in the default rounding mode
inline long long compose_round(double v) { return static_cast<long long>(nearbyint(v)); }

// ImageOps.contain's target for a w x h picture in the box bw x bh (all 1 and more); a side may come out 0, which the
// caller refuses as Pillow raises
inline void compose_contain_size(int w, int h, int bw, int bh, long long* ow, long long* oh) {
  const double im = static_cast<double>(w) / static_cast<double>(h), dest = static_cast<double>(bw) / static_cast<double>(bh);
  *ow = bw; *oh = bh;
  if (im == dest) return;
  if (im > dest) *oh = compose_round(static_cast<double>(h) / static_cast<double>(w) * static_cast<double>(bw));
  else *ow = compose_round(static_cast<double>(w) / static_cast<double>(h) * static_cast<double>(bh));
}

// ImageOps.pad's place of a w x h picture on a cw x ch canvas it lies inside: round((cw - w) * cx) with the centering
// clamped into 0..1, per axis.  (Pillow moves along one axis only: along the other cw - w is 0.)
inline long long compose_pad_offset(int canvas, int picture, double centering) {
  const double c = centering < 0.0 ? 0.0 : centering > 1.0 ? 1.0 : centering;
  return compose_round(static_cast<double>(canvas - picture) * c);
}

// The top-left of an overlay ow x oh on a canvas cw x ch from its anchor and the margin (x, y) inward from it.  64-bit:
// the sum of three int32 cannot wrap.
inline void compose_anchor(int anchor, long long cw, long long ch, long long ow, long long oh, long long x, long long y, long long* ox, long long* oy) {
  const bool right = anchor == 1 || anchor == 3, bottom = anchor == 2 || anchor == 3;
  if (anchor == 4) {
    // floor((cw - ow) / 2), also where the overlay is the wider one
    const long long dx = cw - ow, dy = ch - oh;
    *ox = (dx >= 0 ? dx / 2 : -((-dx + 1) / 2)) + x;
    *oy = (dy >= 0 ? dy / 2 : -((-dy + 1) / 2)) + y;
    return;
  }
  *ox = right ? cw - ow - x : x;
  *oy = bottom ? ch - oh - y : y;
}

// ---- the tiles of the launch (compose.hip): kComposeTileDwords dwords of a canvas row x kComposeTileRows rows, a
// workgroup of 256 lanes; a lane makes one dword column of kComposeTileRows / 4 rows
constexpr unsigned kComposeTileDwords = 64, kComposeTileRows = 16;

inline unsigned long long compose_tiles(unsigned row_dwords, unsigned rows) {
  return static_cast<unsigned long long>((row_dwords + kComposeTileDwords - 1) / kComposeTileDwords) * ((rows + kComposeTileRows - 1) / kComposeTileRows);
}

}  // namespace sjpeg_internal

#endif  // SJPEG_AMD_COMPOSE_MATH_H_
