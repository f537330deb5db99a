// unsharp_math.h -- the arithmetic of the unsharp mask behind the resize (sjpeg_hip_unsharp_ragged_src; unsharp.hip,
// unsharp_plan.cc), stated once for the kernel, the host and the test: a sample and the 3 x 3 neighbourhood of its
// channel, edge replicated, become the sharpened sample.  Integers only, one right answer.  Plain C++ (a host compiler
// reads it as it is: tests/cxx/unsharp_math_test.cc).
#ifndef SJPEG_AMD_UNSHARP_MATH_H_
#define SJPEG_AMD_UNSHARP_MATH_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define SJPEG_UNSHARP_HD __host__ __device__
#else
#define SJPEG_UNSHARP_HD
#endif

namespace sjpeg_internal {

// S of a neighbourhood from its three row sums h = left + 2 * middle + right: the weights [1 2 1] x [1 2 1], sum 16
SJPEG_UNSHARP_HD inline int32_t unsharp_blur16(int32_t h_above, int32_t h_at, int32_t h_below) { return h_above + 2 * h_at + h_below; }

// The sample p (0..255) whose neighbourhood sums to S (0..4080), amount 0..255 in 32nds, threshold 0..255 in byte
// levels: D = 16 p - S is sixteen times p minus the blur; below the threshold p stays, else p + amount * D / 512
// rounded half up (an arithmetic shift: a true floor for negative sums too) and clamped.  |amount * D| <= 1 040 400.
SJPEG_UNSHARP_HD inline int32_t unsharp_apply(int32_t p, int32_t S, int32_t amount, int32_t threshold) {
  const int32_t D = 16 * p - S;
  if ((D < 0 ? -D : D) < 16 * threshold) return p;
  const int32_t v = (512 * p + amount * D + 256) >> 9;
  return v < 0 ? 0 : v > 255 ? 255 : v;
}

// ... from the nine samples n[3 * i + j], row i above / at / below, column j left / at / right: n[4] is p
SJPEG_UNSHARP_HD inline int32_t unsharp_sample(const uint8_t n[9], int32_t amount, int32_t threshold) {
  const int32_t h0 = n[0] + 2 * n[1] + n[2], h1 = n[3] + 2 * n[4] + n[5], h2 = n[6] + 2 * n[7] + n[8];
  return unsharp_apply(n[4], unsharp_blur16(h0, h1, h2), amount, threshold);
}

}  // namespace sjpeg_internal

#endif  // SJPEG_AMD_UNSHARP_MATH_H_
