// light_math.h -- the arithmetic of the resize in linear light (sjpeg_hip_linear_ragged_src; sjpeg_hip.h, "resize in
// linear light"), stated once for the kernel (resize.hip) and for the host: the table that takes an sRGB byte to the
// light it stands for, and the exact inverse that takes a cell's weighted sum of table values back to a byte.  Integers
// only, no pow at run time on either side: one right answer.  Plain C++ (a host compiler reads it as it is:
// tests/cxx/light_math_test.cc).
#ifndef SJPEG_AMD_LIGHT_MATH_H_
#define SJPEG_AMD_LIGHT_MATH_H_

#include <stdint.h>

#include "resize_math.h"

namespace sjpeg_internal {

// L[b] = floor(65535 f(b / 255) + 1/2), f the sRGB decoding function of IEC 61966-2-1: c / 12.92 up to 0.04045,
// ((c + 0.055) / 1.055)^2.4 above.  Evaluated with 60-digit decimals; no entry lies closer than 0.0016 to a rounding
// tie.  Strictly increasing, smallest step 19, sum 5217863.
constexpr uint16_t kLightSrgb[256] = {
        0,    20,    40,    60,    80,    99,   119,   139,   159,   179,   199,   219,   241,   264,   288,   313,
      340,   367,   396,   427,   458,   491,   526,   562,   599,   637,   677,   718,   761,   805,   851,   898,
      947,   997,  1048,  1101,  1156,  1212,  1270,  1330,  1391,  1453,  1517,  1583,  1651,  1720,  1790,  1863,
     1937,  2013,  2090,  2170,  2250,  2333,  2418,  2504,  2592,  2681,  2773,  2866,  2961,  3058,  3157,  3258,
     3360,  3464,  3570,  3678,  3788,  3900,  4014,  4129,  4247,  4366,  4488,  4611,  4736,  4864,  4993,  5124,
     5257,  5392,  5530,  5669,  5810,  5953,  6099,  6246,  6395,  6547,  6700,  6856,  7014,  7174,  7335,  7500,
     7666,  7834,  8004,  8177,  8352,  8528,  8708,  8889,  9072,  9258,  9445,  9635,  9828, 10022, 10219, 10417,
    10619, 10822, 11028, 11235, 11446, 11658, 11873, 12090, 12309, 12530, 12754, 12980, 13209, 13440, 13673, 13909,
    14146, 14387, 14629, 14874, 15122, 15371, 15623, 15878, 16135, 16394, 16656, 16920, 17187, 17456, 17727, 18001,
    18277, 18556, 18837, 19121, 19407, 19696, 19987, 20281, 20577, 20876, 21177, 21481, 21787, 22096, 22407, 22721,
    23038, 23357, 23678, 24002, 24329, 24658, 24990, 25325, 25662, 26001, 26344, 26688, 27036, 27386, 27739, 28094,
    28452, 28813, 29176, 29542, 29911, 30282, 30656, 31033, 31412, 31794, 32179, 32567, 32957, 33350, 33745, 34143,
    34544, 34948, 35355, 35764, 36176, 36591, 37008, 37429, 37852, 38278, 38706, 39138, 39572, 40009, 40449, 40891,
    41337, 41785, 42236, 42690, 43147, 43606, 44069, 44534, 45002, 45473, 45947, 46423, 46903, 47385, 47871, 48359,
    48850, 49344, 49841, 50341, 50844, 51349, 51858, 52369, 52884, 53401, 53921, 54445, 54971, 55500, 56032, 56567,
    57105, 57646, 58190, 58737, 59287, 59840, 60396, 60955, 61517, 62082, 62650, 63221, 63795, 64372, 64952, 65535,
};

// The byte whose light is nearest a cell's exact average S / A, A = W H, S = the weighted sum of the table values of
// the cell, at most 65535 A < 2^48: the number of k in 1..255 with 2 S >= (L[k-1] + L[k]) A.  The midpoints rise with
// k, so that number is the largest such k (0: none), found by 8 halvings: 128 + 64 + .. + 1 = 255, so k never leaves
// the table.  A tie goes to the larger byte.  Every compare is of exact 64-bit values: L[k-1] + L[k] < 2^17 and
// A < 2^32, so the product is one 32 x 32 -> 64 multiply and both sides stay below 2^49.  `table` is kLightSrgb or a
// copy of it (the kernel's lies in LDS).  S = L[b] A gives b: L[b-1] + L[b] <= 2 L[b] < L[b] + L[b+1].
SJPEG_RESIZE_HD inline uint32_t light_round(uint64_t S, uint32_t W, uint32_t H, const uint16_t* table) {
  const uint32_t A = W * H;
  const uint64_t n = 2u * S;
  uint32_t k = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t step = 128u; step != 0u; step >>= 1) {
    const uint32_t t = k + step, m = static_cast<uint32_t>(table[t - 1u]) + table[t];
    if (n >= static_cast<uint64_t>(m) * A) k = t;
  }
  return k;
}

}  // namespace sjpeg_internal

#endif  // SJPEG_AMD_LIGHT_MATH_H_
