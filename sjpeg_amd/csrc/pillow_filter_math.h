// pillow_filter_math.h -- the arithmetic of Pillow 12.2.0's BoxBlur, GaussianBlur and UnsharpMask on pictures of bytes
// (sjpeg_hip_filter_ragged_src; pillow_filter.hip, pillow_filter_plan.cc), stated once for the kernel, the host and the
// tests.  The weights of an axis are float32 work done once on the host; everything per sample is integers, one right
// answer.  Plain C++ (a host compiler reads it as it is: tests/cxx/pillow_filter_math_test.cc).
#ifndef SJPEG_AMD_PILLOW_FILTER_MATH_H_
#define SJPEG_AMD_PILLOW_FILTER_MATH_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SJPEG_PFILTER_HD __host__ __device__
#else
#define SJPEG_PFILTER_HD
#endif

namespace sjpeg_internal {

constexpr uint32_t kPillowFilterRadiusMax = 63;   // the largest integer box radius of an axis the kernel's LDS holds

// One box pass of an axis: r = (int) fr, ww = (uint32) (2^24 / (fr * 2 + 1)) -- the division and the sum in FLOAT32,
// truncated; divided in double, radii 0.3 and 2.7 give other bytes --, fw what is left of 2^24, halved: the weight of
// the two samples r + 1 away.  passes: how often the pass runs along the axis, 0: the axis is skipped.
struct PillowFilterAxis {
  uint32_t r, ww, fw, passes;
};

// volatile: every operation below is rounded to float32 where it stands, whatever the compiler's float mode
inline void pillow_box_weights(float fr, uint32_t* r, uint32_t* ww, uint32_t* fw) {
  volatile float twice = fr * 2.0f;
  volatile float width = twice + 1.0f;
  volatile float q = 16777216.0f / width;
  *r = static_cast<uint32_t>(static_cast<int>(fr));
  *ww = static_cast<uint32_t>(q);
  *fw = ((1u << 24) - (2u * *r + 1u) * *ww) / 2u;
}

// The box radius three passes of which make a Gaussian of `sigma` (Pillow's _gaussian_blur_radius, 3 passes): every
// operation rounded to float32 but sqrt and floor, which take and return double as C's do.  In doubles 714 of 4 024
// sigmas give another radius.
inline float pillow_gaussian_radius(float sigma) {
  volatile float sq = sigma * sigma;
  volatile float s2 = sq / 3.0f;
  volatile float t = 12.0f * s2;
  volatile float u = t + 1.0f;
  volatile float L = static_cast<float>(sqrt(static_cast<double>(u)));
  volatile float Lm = L - 1.0f;
  volatile float half = Lm / 2.0f;
  volatile float l = static_cast<float>(floor(static_cast<double>(half)));
  volatile float a1 = 2.0f * l;
  volatile float a2 = a1 + 1.0f;                  // 2 l + 1
  volatile float b1 = l + 1.0f;
  volatile float b2 = l * b1;                     // l (l + 1)
  volatile float b3 = 3.0f * s2;
  volatile float b4 = b2 - b3;
  volatile float a = a2 * b4;
  volatile float c1 = b1 * b1;                    // (l + 1) (l + 1)
  volatile float c2 = s2 - c1;
  volatile float c3 = 6.0f * c2;
  volatile float q = a / c3;
  volatile float fr = l + q;
  return fr;
}

// The axis of a filter kind (1 box, 2 gaussian, 3 unsharp mask) with `radius` -- a box radius for kind 1, a sigma for 2
// and 3; finite and not negative, the caller's to check.  A box radius of 0 skips the axis.
inline PillowFilterAxis pillow_filter_axis(int kind, float radius) {
  PillowFilterAxis a = {0u, 1u << 24, 0u, 0u};
  if (kind < 1 || kind > 3) return a;
  const PillowFilterAxis beyond = {0xffffffffu, 0u, 0u, 1u};       // (no box radius the kernel takes: refused by its r)
  // a sigma far beyond what r <= kPillowFilterRadiusMax allows (about 64.6) does not enter the formula: from about
  // 1.4e15 on, sigma * sigma / 3 cancels or overflows in float32 and the radius comes out as -inf or NaN
  if (kind != 1 && radius > 1024.0f) return beyond;
  const float fr = kind == 1 ? radius : pillow_gaussian_radius(radius);
  if (fr != fr) return beyond;
  if (!(fr > 0.0f)) return a;
  if (!(fr < 16777216.0f)) return beyond;
  pillow_box_weights(fr, &a.r, &a.ww, &a.fw);
  a.passes = kind == 1 ? 1u : 3u;
  return a;
}

// what the kernel's uint32 relies on: the 2 r + 1 inner weights do not exceed 2^24, so the sum with the two outer ones
// is at most 255 * 2^24 and the rounding term fits above it
inline bool pillow_filter_axis_bound(const PillowFilterAxis& a) {
  return static_cast<uint64_t>(2u * static_cast<uint64_t>(a.r) + 1u) * a.ww <= (1u << 24);
}

// A sample of one pass: S the sum of the 2 r + 1 samples around it, edge the sum of the two r + 1 away (indices clamped
// into the line).  At most 255 * 2^24 + 2^23.
SJPEG_PFILTER_HD inline uint32_t pillow_box_sample(uint32_t ww, uint32_t fw, uint32_t S, uint32_t edge) {
  return (ww * S + fw * edge + (1u << 23)) >> 24;
}

// UnsharpMask's sample from the picture's p and the blurred b: the comparison is STRICT, the division C's (toward zero)
SJPEG_PFILTER_HD inline uint32_t pillow_unsharp_sample(int32_t p, int32_t b, int32_t percent, int32_t threshold) {
  const int32_t d = p - b;
  if ((d < 0 ? -d : d) <= threshold) return static_cast<uint32_t>(p);
  const int32_t v = p + d * percent / 100;
  return static_cast<uint32_t>(v < 0 ? 0 : v > 255 ? 255 : v);
}

// ---- the tiles of the two launches (pillow_filter.hip).  The row launch: kRowTilePixels pixels x kRowTileRows rows of a
// plane; the column launch: kColTileDwords dwords x kColTileRows rows.  A workgroup stages its tile and a halo of
// passes * (r + 1) samples on each side along the axis, cut off at the line's ends.
constexpr unsigned kPillowRowTilePixels = 128, kPillowRowTileRows = 4, kPillowColTileDwords = 4, kPillowColTileRows = 64;
constexpr unsigned kPillowHaloMax = 3 * (kPillowFilterRadiusMax + 1);
// bytes a staged row of the row launch takes at most: the tile and both halos of three-byte pixels, and the bytes in
// front of and behind them up to whole dwords
constexpr unsigned kPillowRowLineBytes = (kPillowRowTilePixels + 2 * kPillowHaloMax) * 3 + 8;
// ... and a staged row of the column launch: the tile's dwords and one dword of padding.  The lanes of a wave make
// runs 8 rows apart of 16 byte columns: 8 rows of 5 dwords are 40 dwords, so the four runs read banks 0.., 40.., 16..
// and 56.. of 64 (0, 8, 16, 24 of 32) and never the same one; rows of 4 dwords would put all four on the same banks.
// (At r = 1 and r = 7 the padding measured no gain -- profiles/HISTORY.md; it is kept for large r, which was not timed.)
constexpr unsigned kPillowColLineBytes = 4 * kPillowColTileDwords + 4;
constexpr unsigned kPillowStageBytes = kPillowRowLineBytes * kPillowRowTileRows > kPillowColLineBytes * (kPillowColTileRows + 2 * kPillowHaloMax)
                                           ? kPillowRowLineBytes * kPillowRowTileRows
                                           : kPillowColLineBytes * (kPillowColTileRows + 2 * kPillowHaloMax);
static_assert(kPillowRowTilePixels % 4 == 0 && kPillowRowLineBytes % 4 == 0 && kPillowStageBytes % 4 == 0, "tiles begin at whole dwords");

inline unsigned long long pillow_row_tiles(unsigned width, unsigned rows) {
  return static_cast<unsigned long long>((width + kPillowRowTilePixels - 1) / kPillowRowTilePixels) * ((rows + kPillowRowTileRows - 1) / kPillowRowTileRows);
}
inline unsigned long long pillow_col_tiles(unsigned row_dwords, unsigned rows) {
  return static_cast<unsigned long long>((row_dwords + kPillowColTileDwords - 1) / kPillowColTileDwords) * ((rows + kPillowColTileRows - 1) / kPillowColTileRows);
}

}  // namespace sjpeg_internal

#endif  // SJPEG_AMD_PILLOW_FILTER_MATH_H_
