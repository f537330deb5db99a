// resize_math.h -- the arithmetic of the ragged resize (sjpeg_hip_resize_ragged_src, resize.hip), stated once for the
// kernel and for the host: the exact area average of a picture of n_src samples an axis made n_dst <= n_src samples
// long.  Both pictures lie on a grid of n_src * n_dst units: source index x covers [x * n_dst, (x + 1) * n_dst), output
// index xo covers [xo * n_src, (xo + 1) * n_src).  Every axis is 1..65535 long, so every product below stays inside 32
// bits (65535 * 65535 + 65534 < 2^32).  Plain C++ (a host compiler reads it as it is: tests/cxx/resize_math_test.cc).
#ifndef SJPEG_AMD_RESIZE_MATH_H_
#define SJPEG_AMD_RESIZE_MATH_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define SJPEG_RESIZE_HD __host__ __device__
#else
#define SJPEG_RESIZE_HD
#endif

namespace sjpeg_internal {

// how many grid units source index x and output cell xo share: the weight of x in xo.  Over x it sums to n_src.
SJPEG_RESIZE_HD inline uint32_t resize_weight(uint32_t xo, uint32_t x, uint32_t n_src, uint32_t n_dst) {
  const uint32_t a = x * n_dst, b = xo * n_src;
  const uint32_t lo = a > b ? a : b;
  const uint32_t hi = a + n_dst < b + n_src ? a + n_dst : b + n_src;
  return hi > lo ? hi - lo : 0u;
}

// the first source index of output cell xo with a weight above 0, and how many there are: at most
// ceil(n_src / n_dst) + 1, consecutive cells share at most one index
SJPEG_RESIZE_HD inline uint32_t resize_first(uint32_t xo, uint32_t n_src, uint32_t n_dst) { return xo * n_src / n_dst; }
SJPEG_RESIZE_HD inline uint32_t resize_count(uint32_t xo, uint32_t n_src, uint32_t n_dst) {
  return ((xo + 1u) * n_src + n_dst - 1u) / n_dst - resize_first(xo, n_src, n_dst);
}

// (2 S + W H) / (2 W H) for S = the weighted sum of a cell, at most 255 W H: round half up, exact.  The quotient is at
// most 255, the divisor up to 2^33 and the same for a whole frame, so no 64-bit division: the quotient of the two as
// floats is off by less than 2^-13 (three roundings of 2^-24 each on a value below 256), its floor by at most one, and
// two compares of exact 64-bit products (q * d < 2^42) put it right.  The loops end after one step; they are loops so
// that the result does not rest on how a float division rounds.
SJPEG_RESIZE_HD inline uint32_t resize_round(uint64_t S, uint32_t W, uint32_t H) {
  const uint64_t area = static_cast<uint64_t>(W) * H, d = 2u * area, n = 2u * S + area;
  uint64_t q = static_cast<uint64_t>(static_cast<float>(n) / static_cast<float>(d));
  while (q * d > n) --q;
  while ((q + 1u) * d <= n) ++q;
  return static_cast<uint32_t>(q);
}

// The same for 16-bit samples whose byte lies `shift` = 0..8 bits up (sjpeg_hip_yuv_depth): min(255, floor((2 S +
// A 2^s) / (A 2^(s+1)))), A = W H -- the exact average of the words, divided by 2^s, rounded half up ONCE, then
// clamped (a full-scale picture gives 256 before the clamp).  S is at most 65535 A < 2^48, so the numerator is below
// 2^50 and the divisor at most 2^41.  A quotient of 256 or more is decided by one compare of exact values (256 d <
// 2^49); below that the quotient is at most 255 and the float estimate with its two exact compares is resize_round's,
// bound for bound (q * d < 2^49).
SJPEG_RESIZE_HD inline uint32_t resize_round_deep(uint64_t S, uint32_t W, uint32_t H, uint32_t shift) {
  const uint64_t area = static_cast<uint64_t>(W) * H, d = (2u * area) << shift, n = 2u * S + (area << shift);
  if (n >= 256u * d) return 255u;
  uint64_t q = static_cast<uint64_t>(static_cast<float>(n) / static_cast<float>(d));
  while (q * d > n) --q;
  while ((q + 1u) * d <= n) ++q;
  return static_cast<uint32_t>(q);
}

}  // namespace sjpeg_internal

#endif  // SJPEG_AMD_RESIZE_MATH_H_
