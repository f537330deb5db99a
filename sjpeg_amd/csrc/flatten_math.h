// flatten_math.h -- the arithmetic of alpha flattening (sjpeg_hip_flatten_ragged_src; resize.hip, resize_plan.cc),
// stated once for the kernel, the host and the test: a colour byte s of a pixel with alpha byte a laid over a
// background byte bg.  Integers only, one right answer.  Plain C++ (a host compiler reads it as it is:
// tests/cxx/flatten_math_test.cc).
#ifndef SJPEG_AMD_FLATTEN_MATH_H_
#define SJPEG_AMD_FLATTEN_MATH_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define SJPEG_FLATTEN_HD __host__ __device__
#else
#define SJPEG_FLATTEN_HD
#endif

namespace sjpeg_internal {

// t / 255 for t in 0..65535 without a division: t * 0x8081 < 2^32, and (t * 0x8081) >> 23 is the quotient for every
// such t (the test runs through all of them)
SJPEG_FLATTEN_HD inline uint32_t flatten_div255(uint32_t t) { return (t * 0x8081u) >> 23; }

// straight alpha: (a s + (255 - a) bg) / 255 rounded to nearest -- 255 is odd, so there are no ties.  The numerator
// is at most 255 * 255 + 127 = 65152 < 2^16; a = 255 gives s and a = 0 gives bg exactly, and the result never
// exceeds 255.
SJPEG_FLATTEN_HD inline uint32_t flatten_straight(uint32_t a, uint32_t s, uint32_t bg) {
  return flatten_div255(a * s + (255u - a) * bg + 127u);
}

// premultiplied alpha: s is a * colour / 255 already, so only the background is weighted; a source whose samples are
// above their alpha saturates at 255
SJPEG_FLATTEN_HD inline uint32_t flatten_premultiplied(uint32_t a, uint32_t s, uint32_t bg) {
  const uint32_t b = s + flatten_div255((255u - a) * bg + 127u);
  return b < 255u ? b : 255u;
}

SJPEG_FLATTEN_HD inline uint32_t flatten_byte(uint32_t a, uint32_t s, uint32_t bg, bool premultiplied) {
  return premultiplied ? flatten_premultiplied(a, s, bg) : flatten_straight(a, s, bg);
}

}  // namespace sjpeg_internal

#endif  // SJPEG_AMD_FLATTEN_MATH_H_
