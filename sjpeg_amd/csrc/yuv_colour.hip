// yuv_colour.hip -- the made planes of a ragged batch of video frames converted to JFIF's colour on gfx950: BT.601 or
// BT.709, full or limited range, to full-range BT.601, in ONE launch behind the resize launch, in place
// (sjpeg_hip_convert_ragged_yuv_src, sjpeg_hip_encode_ragged_yuv_converted_src, the _yuv_colour sheet entries;
// sjpeg_hip.h).
//
// Reference: none -- the reference codes the samples it is given.  The contract is on the bytes: every converted sample
// is yuv_colour_math.h's formula of the made planes' samples, integers only, one right answer.
//
// Shape: a flat grid over the batch's tiles, a workgroup one tile of 256 lanes of one frame, found by the binary
// search over the frames' first tiles that resize.hip uses -- so the table, the sizes and the sampling are
// wave-uniform; a frame with identity colour has no tiles.  A lane owns four chroma samples of a row -- one dword of U,
// one of V -- and the luma samples above them: two dwords in each of two rows for the 4:2:0 formats, one dword for
// 4:4:4.  It loads all of them, converts -- luma from the chroma it loaded, not from what it stores --, and stores
// them.  No lane reads a sample another lane writes: there is no ordering between lanes to keep.  No atomics, no LDS.
//
// A picture of its own starts at a multiple of 16 with rows whole dwords apart: every access is an aligned dword, the
// row's padding is converted and written along, and a dword that begins at or beyond the row's stride, or a row beyond
// the plane, is not touched (a luma row of 9..12 samples over a chroma row of 5: the second lane's second luma dword).
// A PLACED picture (a sheet's thumbnail) starts at any byte of its sheet plane: a lane owns the chroma samples of one
// ALIGNED dword of the sheet plane's row, `lead` says how the rectangle lies against those, and only the rectangle's
// own bytes are loaded and stored -- whole dwords inside the span, single bytes at its two ends, as resize.hip's
// turned store does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ragged_aux.h"
#include "yuv_colour_math.h"

namespace {

using sjpeg_internal::YuvColourFrame;
using sjpeg_internal::YuvColourTable;

struct YuvColourArgs {
  const YuvColourFrame* frames;
  int nframes;
};

// The planes lie in device memory (reduce.hip says why this is said)
typedef __attribute__((address_space(1))) uint32_t* GlobalDword;
typedef __attribute__((address_space(1))) uint8_t* GlobalByte;

// The four bytes of a plane's row from sample p on (n samples a row), as one dword.
// A picture of its own: p is a multiple of 4 and the row starts at a dword boundary; the dword is loaded when it
// begins below the stride -- what it holds behind the n samples is row padding.
// A placed picture: the dword when all four bytes are samples of the rectangle (and it is aligned: it is, for the
// placement sheet_plan.cc makes), else the rectangle's own bytes one by one; the others read as 0.
template <bool kPlaced>
__device__ __forceinline__ bool whole_dword(const uint8_t* row, int p, int n, unsigned stride) {
  if (!kPlaced) return static_cast<unsigned>(p) < stride;
  return p >= 0 && p + 4 <= n && (reinterpret_cast<uintptr_t>(row + p) & 3u) == 0u;
}
template <bool kPlaced>
__device__ __forceinline__ uint32_t load4(uint8_t* row, int p, int n, unsigned stride) {
  if (whole_dword<kPlaced>(row, p, n, stride)) return *((GlobalDword)(row + p));
  uint32_t v = 0u;
  if constexpr (kPlaced) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (p + b >= 0 && p + b < n) v |= static_cast<uint32_t>(((GlobalByte)(row))[p + b]) << (8 * b);
    }
  }
  return v;
}
// ... and stored: the same bytes that load4 read, no other
template <bool kPlaced>
__device__ __forceinline__ void store4(uint8_t* row, int p, int n, unsigned stride, uint32_t v) {
  if (whole_dword<kPlaced>(row, p, n, stride)) { *((GlobalDword)(row + p)) = v; return; }
  if constexpr (kPlaced) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (p + b >= 0 && p + b < n) ((GlobalByte)(row))[p + b] = static_cast<uint8_t>(v >> (8 * b));
    }
  }
}

template <bool kPlaced>
__global__ __launch_bounds__(256) void yuv_colour_kernel(const YuvColourArgs a) {
  const unsigned wg = blockIdx.x, tid = threadIdx.x;
  int flo = 0, fhi = a.nframes - 1;
  while (flo < fhi) {                                              // (the LAST frame whose first tile is not behind wg:
    const int mid = (flo + fhi + 1) >> 1;                          // a frame without tiles is never the one found)
    if (a.frames[mid].tile_base <= wg) flo = mid; else fhi = mid - 1;
  }
  const YuvColourFrame d = a.frames[flo];
  const unsigned lane = (wg - d.tile_base) * 256u + tid;
  const unsigned j = lane / d.groups, g = lane - j * d.groups;     // my chroma row, my group of four in it
  if (j >= static_cast<unsigned>(d.ch)) return;
  const YuvColourTable t = d.table;
  // my first chroma sample, counted from the rectangle's first (placed: the first lane's may lie in front of it)
  const int p = 4 * static_cast<int>(g) - (kPlaced ? d.lead : 0);
  uint8_t* const urow = d.u + static_cast<size_t>(j) * d.c_stride;
  uint8_t* const vrow = d.v + static_cast<size_t>(j) * d.c_stride;
  const uint32_t ud = load4<kPlaced>(urow, p, d.cw, d.c_stride), vd = load4<kPlaced>(vrow, p, d.cw, d.c_stride);
  // my luma: s rows of s dwords, from sample s * p on
  const bool half = d.s == 2;
  const int nrows = half ? 2 : 1, ndw = half ? 2 : 1, l0 = half ? 2 * p : p;
  const unsigned r0 = half ? 2u * j : j;
  uint32_t yd[2][2] = {{0u, 0u}, {0u, 0u}};
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (r >= nrows || r0 + r >= static_cast<unsigned>(d.uh)) continue;
    uint8_t* const yrow = d.y + static_cast<size_t>(r0 + r) * d.y_stride;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (k < ndw) yd[r][k] = load4<kPlaced>(yrow, l0 + 4 * k, d.uw, d.y_stride);
    }
  }
  int32_t u[4], v[4];
  uint32_t uo = 0u, vo = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u[i] = static_cast<int32_t>((ud >> (8 * i)) & 255u) - 128;
    v[i] = static_cast<int32_t>((vd >> (8 * i)) & 255u) - 128;
    uo |= static_cast<uint32_t>(sjpeg_internal::yuv_colour_chroma(t, 1, u[i], v[i])) << (8 * i);
    vo |= static_cast<uint32_t>(sjpeg_internal::yuv_colour_chroma(t, 2, u[i], v[i])) << (8 * i);
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (r >= nrows || r0 + r >= static_cast<unsigned>(d.uh)) continue;
    uint8_t* const yrow = d.y + static_cast<size_t>(r0 + r) * d.y_stride;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (k >= ndw) continue;
      uint32_t yo = 0u;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i = half ? 2 * k + (b >> 1) : b;                 // the chroma sample whose block luma byte b lies in
        const int32_t y = static_cast<int32_t>((yd[r][k] >> (8 * b)) & 255u);
        yo |= static_cast<uint32_t>(sjpeg_internal::yuv_colour_luma(t, y, u[i], v[i])) << (8 * b);
      }
      store4<kPlaced>(yrow, l0 + 4 * k, d.uw, d.y_stride, yo);
    }
  }
  store4<kPlaced>(urow, p, d.cw, d.c_stride, uo);
  store4<kPlaced>(vrow, p, d.cw, d.c_stride, vo);
}

}  // namespace

namespace sjpeg_internal {

int yuv_colour_launch(bool placed, const YuvColourFrame* d_frames, int nframes, unsigned tiles, hipStream_t st) {
  YuvColourArgs a;
  a.frames = d_frames;
  a.nframes = nframes;
  if (placed) {
    hipLaunchKernelGGL((yuv_colour_kernel<true>), dim3(tiles), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((yuv_colour_kernel<false>), dim3(tiles), dim3(256), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace sjpeg_internal
