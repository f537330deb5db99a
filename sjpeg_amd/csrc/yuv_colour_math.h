// yuv_colour_math.h -- the arithmetic of the video colour conversion (sjpeg_hip_convert_ragged_yuv_src; yuv_colour.hip,
// yuv_colour_plan.cc), stated once for the kernel, the host and the test: a (Y, U, V) sample of a BT.601 or BT.709
// source in full or limited range becomes the full-range BT.601 sample that a JFIF file holds.  Integers only, Q14, one
// right answer.  Plain C++ (a host compiler reads it as it is: tests/cxx/yuv_colour_math_test.cc).
#ifndef SJPEG_AMD_YUV_COLOUR_MATH_H_
#define SJPEG_AMD_YUV_COLOUR_MATH_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define SJPEG_YUV_COLOUR_HD __host__ __device__
#else
#define SJPEG_YUV_COLOUR_HD
#endif

namespace sjpeg_internal {

// y0 and k = rint(M * 16384): rows Y, U, V of the output, columns Y, U, V of the source; the chroma rows never read
// luma.  M is source Y'CbCr -> R'G'B' by the source's Kr, Kb, then R'G'B' -> full-range BT.601 YCbCr, the columns
// scaled by 255/219 (Y) and 255/224 (chroma) for a limited-range source (tests/test_yuv_colour_host.py derives them).
struct YuvColourTable {
  int32_t y0;
  int32_t k[3][3];
};

// matrix: SJPEG_HIP_MATRIX_BT601 (0) or _BT709 (1); range: SJPEG_HIP_RANGE_FULL (0) or _LIMITED (1)
SJPEG_YUV_COLOUR_HD inline bool yuv_colour_is_identity(int matrix, int range) { return matrix == 0 && range == 0; }

SJPEG_YUV_COLOUR_HD inline YuvColourTable yuv_colour_table(int matrix, int range) {
  if (matrix == 0) {
    if (range == 0) return {0, {{16384, 0, 0}, {0, 16384, 0}, {0, 0, 16384}}};          // (the formula then gives the sample back)
    return {16, {{19077, 0, 0}, {0, 18651, 0}, {0, 0, 18651}}};
  }
  if (range == 0) return {0, {{16384, 1664, 3213}, {0, 16218, -1813}, {0, -1187, 16112}}};
  return {16, {{19077, 1895, 3657}, {0, 18462, -2064}, {0, -1351, 18342}}};
}

SJPEG_YUV_COLOUR_HD inline int32_t yuv_colour_clamp8(int32_t v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// floor(n / 16384) of a sum that has its rounding term already: an arithmetic shift, a true floor for negative n too.
// The largest sum is 19077 * 255 + (1895 + 3657) * 128 + 8192 < 2^23 in magnitude: 32 bits hold every one.
// On the device the quotient passes through an empty asm, which the optimizer cannot see through: without it hipcc
// (ROCm 7.2, gfx950) fuses shift, clamp and the packing of two luma bytes into v_ashr_pk_u8_i32 and then assumes the
// upper half of that instruction's result to be zero, while the hardware leaves there what the register held -- bits
// 16..31 of the first sum came out OR-ed into the third and fourth byte of every stored luma dword (seen on an MI355X;
// profiles/HISTORY.md).  The asm is no instruction; the shift and the v_med3_i32 clamp stay separate.
SJPEG_YUV_COLOUR_HD inline int32_t yuv_colour_floor14(int32_t n) {
  int32_t q = n >> 14;
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(q));
#endif
  return q;
}

// u = U - 128 and v = V - 128 of the UNCONVERTED chroma sample
SJPEG_YUV_COLOUR_HD inline int32_t yuv_colour_luma(const YuvColourTable& t, int32_t y, int32_t u, int32_t v) {
  return yuv_colour_clamp8(yuv_colour_floor14(t.k[0][0] * (y - t.y0) + t.k[0][1] * u + t.k[0][2] * v + 8192));
}
// row 1: U', row 2: V'
SJPEG_YUV_COLOUR_HD inline int32_t yuv_colour_chroma(const YuvColourTable& t, int row, int32_t u, int32_t v) {
  return yuv_colour_clamp8(128 + yuv_colour_floor14(t.k[row][1] * u + t.k[row][2] * v + 8192));
}

}  // namespace sjpeg_internal

#endif  // SJPEG_AMD_YUV_COLOUR_MATH_H_
