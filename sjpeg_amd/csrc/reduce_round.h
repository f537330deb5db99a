// reduce_round.h -- the arithmetic of the ragged reduction (sjpeg_hip_reduce_ragged_src, reduce.hip), stated once for
// the kernel and for the host: how the sum of an s x s box of bytes becomes a byte, and where the reduced pictures lie
// in their buffer.  Plain C++ (a host compiler reads it as it is: tests/cxx/reduce_round_test.cc).
#ifndef SJPEG_AMD_REDUCE_ROUND_H_
#define SJPEG_AMD_REDUCE_ROUND_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SJPEG_REDUCE_HD __host__ __device__
#else
#define SJPEG_REDUCE_HD
#endif

namespace sjpeg_internal {

constexpr int kReduceMax = 8;   // SJPEG_HIP_REDUCE_MAX

// ceil(2^20 / (s * s)): the division by the box's area as a multiplication and a shift.  With x = sum + s*s/2 at most
// 255 * 64 + 32 the product stays below 2^32, and the error x * (magic - 2^20 / n) / 2^20 stays below 0.008, less than
// the 1 / n by which a quotient's fraction stops short of the next integer: the result is floor(x / n) for every sum a
// box can have (the host test walks all of them).
SJPEG_REDUCE_HD inline uint32_t reduce_magic(int s) {
  switch (s) {
    case 1: return 1048576u;
    case 2: return 262144u;
    case 3: return 116509u;
    case 4: return 65536u;
    case 5: return 41944u;
    case 6: return 29128u;
    case 7: return 21400u;
    default: return 16384u;
  }
}

// (sum + s*s/2) / (s*s) for the sum of s * s bytes, s in 1..8: round half up, exact
SJPEG_REDUCE_HD inline uint32_t reduce_round(uint32_t sum, int s) {
  const uint32_t n = static_cast<uint32_t>(s * s);
  return ((sum + (n >> 1)) * reduce_magic(s)) >> 20;
}

// a side of the reduced picture
SJPEG_REDUCE_HD inline int reduced_dim(int v, int s) { return (v + s - 1) / s; }

// The reduced pictures in their buffer (sjpeg_hip.h): interleaved R, G, B (channels = 3) or one gray plane (1), rows
// reduced_row_stride() bytes apart -- the row's bytes rounded up to whole dwords --, every picture at a multiple of 16.
inline size_t reduced_row_stride(int w2, int channels) { return (static_cast<size_t>(w2) * channels + 3) & ~static_cast<size_t>(3); }
inline size_t reduced_picture_bytes(int w2, int h2, int channels) {
  return (reduced_row_stride(w2, channels) * static_cast<size_t>(h2) + 15) & ~static_cast<size_t>(15);
}

}  // namespace sjpeg_internal

#endif  // SJPEG_AMD_REDUCE_ROUND_H_
