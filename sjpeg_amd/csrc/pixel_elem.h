// pixel_elem.h -- float picture elements (SJPEG_HIP_SRC_RGB_PLANAR_F*, _RGB_F*, _RGBA_F*, _GRAY_F*): how one sample
// becomes the byte the encoder sees.  The contract (sjpeg_hip.h), scale and bias being those of the sample's channel:
//   t  = fmaf((float)x, scale, bias)                 ONE fp32 rounding; (float)x is exact for half and bfloat16
//   u8 = isnan(t) ? 0 : (uint8) rint(min(max(t, 0), 255))          round half to even; +-inf saturate
// On gfx950 that is v_fma_f32 (v_fma_mix_f32 straight from a half) and v_cvt_pk_u8_f32, which alone rounds to nearest
// even, saturates and turns NaN into 0 while it puts the byte into its place in a dword (seen on an MI355X: no
// v_rndne_f32 and no NaN select is needed in front of it; subnormal inputs are kept).  What holds the helpers
// to the contract: tests/float_contract.py computes it exactly (the product and sum unrounded, then ONE rounding to
// fp32) and tests/test_float_contract.py compares every helper with it bit for bit -- on every float16 and bfloat16
// bit pattern and 65 536 float32 ones, under transforms on which two roundings, flushed subnormals, ties away from
// zero, truncation and a NaN that is not 0 each change bytes (the runs: profiles/HISTORY.md, "The float pixel
// transform held to its contract").  The scan kernels' loader (scan_device.h),
// the ragged riskiness, the ragged sharp conversion and the reduce kernel all convert through these helpers.
#ifndef SJPEG_AMD_PIXEL_ELEM_H_
#define SJPEG_AMD_PIXEL_ELEM_H_

#include <stdint.h>

#include "sjpeg_hip.h"

namespace sjpeg_internal {

// element kinds of a source: bytes as they are, or floats through the engine's pixel transform
enum { kElemU8 = 0, kElemF32 = 1, kElemF16 = 2, kElemBF16 = 3 };

#if defined(__HIPCC__)
// fmaf(x, scale, bias) as byte `pos` (0..3, a constant) of `old`
template <int POS>
__device__ __forceinline__ uint32_t elem_put_u8(float x, float scale, float bias, uint32_t old) {
  return __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaf(x, scale, bias), static_cast<uint32_t>(POS), old);
}
__device__ __forceinline__ float elem_bf16_lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float elem_bf16_hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
__device__ __forceinline__ float elem_f16_lo(uint32_t w) { return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(w))); }
__device__ __forceinline__ float elem_f16_hi(uint32_t w) { return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(w >> 16))); }

// eight consecutive elements at p (aligned to the element only) as eight bytes in w[0..1]; kind is wave-uniform
__device__ __forceinline__ void elem_load8(const uint8_t* p, int kind, float scale, float bias, uint32_t* w) {
  uint32_t lo = 0, hi = 0;
  if (kind == kElemF32) {
    float f[8];
    __builtin_memcpy(f, p, 32);
    lo = elem_put_u8<0>(f[0], scale, bias, lo); lo = elem_put_u8<1>(f[1], scale, bias, lo);
    lo = elem_put_u8<2>(f[2], scale, bias, lo); lo = elem_put_u8<3>(f[3], scale, bias, lo);
    hi = elem_put_u8<0>(f[4], scale, bias, hi); hi = elem_put_u8<1>(f[5], scale, bias, hi);
    hi = elem_put_u8<2>(f[6], scale, bias, hi); hi = elem_put_u8<3>(f[7], scale, bias, hi);
  } else {
    uint32_t h[4];
    __builtin_memcpy(h, p, 16);
    if (kind == kElemF16) {
      lo = elem_put_u8<0>(elem_f16_lo(h[0]), scale, bias, lo); lo = elem_put_u8<1>(elem_f16_hi(h[0]), scale, bias, lo);
      lo = elem_put_u8<2>(elem_f16_lo(h[1]), scale, bias, lo); lo = elem_put_u8<3>(elem_f16_hi(h[1]), scale, bias, lo);
      hi = elem_put_u8<0>(elem_f16_lo(h[2]), scale, bias, hi); hi = elem_put_u8<1>(elem_f16_hi(h[2]), scale, bias, hi);
      hi = elem_put_u8<2>(elem_f16_lo(h[3]), scale, bias, hi); hi = elem_put_u8<3>(elem_f16_hi(h[3]), scale, bias, hi);
    } else {
      lo = elem_put_u8<0>(elem_bf16_lo(h[0]), scale, bias, lo); lo = elem_put_u8<1>(elem_bf16_hi(h[0]), scale, bias, lo);
      lo = elem_put_u8<2>(elem_bf16_lo(h[1]), scale, bias, lo); lo = elem_put_u8<3>(elem_bf16_hi(h[1]), scale, bias, lo);
      hi = elem_put_u8<0>(elem_bf16_lo(h[2]), scale, bias, hi); hi = elem_put_u8<1>(elem_bf16_hi(h[2]), scale, bias, hi);
      hi = elem_put_u8<2>(elem_bf16_lo(h[3]), scale, bias, hi); hi = elem_put_u8<3>(elem_bf16_hi(h[3]), scale, bias, hi);
    }
  }
  w[0] = lo; w[1] = hi;
}

// eight interleaved pixels at p, STEP (3 or 4) elements each, R G B first: 8 * STEP elements in one piece -- but for
// the last pixel's fourth, which may lie outside the allocation (31 elements, not 32) -- as the planar class's six
// dwords, w[0..1] R, w[2..3] G, w[4..5] B; channel c through scale[c], bias[c]
template <int STEP>
__device__ __forceinline__ void elem_load8x3(const uint8_t* p, int kind, const float* scale, const float* bias, uint32_t* w) {
  constexpr int kN = 8 * STEP - (STEP == 4 ? 1 : 0);
  uint32_t o[6] = {0, 0, 0, 0, 0, 0};
  if (kind == kElemF32) {
    float f[kN];
    __builtin_memcpy(f, p, 4 * kN);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        o[2 * c + (i >> 2)] = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaf(f[i * STEP + c], scale[c], bias[c]), static_cast<uint32_t>(i & 3), o[2 * c + (i >> 2)]);
      }
    }
  } else {
    uint32_t h[4 * STEP];
    h[4 * STEP - 1] = 0;
    __builtin_memcpy(h, p, 2 * kN);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int k = i * STEP + c;
        const uint32_t hw = h[k >> 1];
        const float x = (kind == kElemF16) ? ((k & 1) ? elem_f16_hi(hw) : elem_f16_lo(hw)) : ((k & 1) ? elem_bf16_hi(hw) : elem_bf16_lo(hw));
        o[2 * c + (i >> 2)] = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaf(x, scale[c], bias[c]), static_cast<uint32_t>(i & 3), o[2 * c + (i >> 2)]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) w[k] = o[k];
}

// one element at p as a float (kind: one of the float kinds)
__device__ __forceinline__ float elem_load_float(const uint8_t* p, int kind) {
  if (kind == kElemF32) {
    float f;
    __builtin_memcpy(&f, p, 4);
    return f;
  }
  uint16_t h;
  __builtin_memcpy(&h, p, 2);
  return kind == kElemF16 ? elem_f16_lo(h) : elem_bf16_lo(h);
}

// the byte (0..255) the encoder sees at p: the sample itself, or the float there through the pixel transform
__device__ __forceinline__ int elem_load_u8(const uint8_t* p, int kind, float scale, float bias) {
  if (kind == kElemU8) return *p;
  return static_cast<int>(elem_put_u8<0>(elem_load_float(p, kind), scale, bias, 0u));
}
#endif  // __HIPCC__

}  // namespace sjpeg_internal

#endif  // SJPEG_AMD_PIXEL_ELEM_H_
