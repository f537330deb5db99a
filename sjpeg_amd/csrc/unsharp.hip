// unsharp.hip -- the made pictures of a ragged batch sharpened on gfx950: the 3 x 3 unsharp mask of unsharp_math.h in
// ONE launch behind the launch that made them, out of place (sjpeg_hip_unsharp_ragged_src and the other _unsharp
// entries; sjpeg_hip.h).
//
// Reference: none -- the reference codes the samples it is given.  The contract is on the bytes: every sample is
// unsharp_math.h's formula of the made plane's samples, integers only, one right answer.
//
// Shape: a flat grid over the batch's tiles, a workgroup one tile of 64 dwords x 16 rows of one plane, found by the
// binary search over the planes' first tiles that resize.hip uses -- so the descriptor, the channel step and the
// parameters are wave-uniform.  The workgroup stages its tile's rows plus one above and below, and one dword left and
// right, into LDS: 18 x 66 dwords, consecutive lanes consecutive dwords of a row, row and dword indices clamped into the
// plane -- which replicates the edge rows and keeps every load inside the plane.  Behind the barrier a wave owns four
// rows of the tile and a lane one dword column of them: it reads its column and the two beside it from six staged
// rows (consecutive lanes consecutive dwords: conflict-free), forms the six row sums [1 2 1] of its four bytes once and
// the four outputs from them, and stores four aligned dwords.  No lane reads what another writes to global memory,
// no atomics.
//
// A made picture starts at a multiple of 16 with rows whole dwords apart: every access is an aligned dword.  The
// neighbour of a sample in the row's first or last pixel is the sample itself -- never the row's padding, never the
// clamped dword beside the plane.  The last dword of a row is written whole: what lands in the row's padding is
// unspecified.  A dword that begins at or beyond the row's samples, or a row beyond the plane, is not touched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ragged_aux.h"
#include "unsharp_math.h"

namespace {

using sjpeg_internal::UnsharpPlane;

constexpr int kTileDwords = static_cast<int>(sjpeg_internal::kUnsharpTileDwords), kTileRows = static_cast<int>(sjpeg_internal::kUnsharpTileRows);
constexpr int kStageDwords = kTileDwords + 2, kStageRows = kTileRows + 2;
constexpr int kLaneRows = kTileRows / 4;                            // rows a lane makes: four waves share the tile's
static_assert(kTileDwords == 64 && kTileRows % 4 == 0, "a wave is a row of the tile's dwords; four waves share its rows");

struct UnsharpArgs {
  const UnsharpPlane* planes;
  int nplanes;
};

// The planes lie in device memory (reduce.hip says why this is said)
typedef const __attribute__((address_space(1))) uint32_t* GlobalIn;
typedef __attribute__((address_space(1))) uint32_t* GlobalOut;

// byte i of the twelve that three consecutive dwords hold
template <int I>
__device__ __forceinline__ int32_t byte_at(uint32_t lo, uint32_t mid, uint32_t hi) {
  static_assert(I >= 0 && I < 12, "a window of three dwords");
  return static_cast<int32_t>(((I < 4 ? lo : I < 8 ? mid : hi) >> (8 * (I & 3))) & 255u);
}

// The row sums left + 2 * at + right of the four samples of `mid`, the channel's neighbours kStep bytes away; x0 is
// the byte of the row that `mid` begins at, n the row's samples.  A neighbour outside the row is the sample itself.
template <int kStep, int B>
__device__ __forceinline__ int32_t row_sum(uint32_t lo, uint32_t mid, uint32_t hi, unsigned x0, unsigned n) {
  const int32_t at = byte_at<4 + B>(lo, mid, hi);
  const int32_t left = x0 + B >= static_cast<unsigned>(kStep) ? byte_at<4 + B - kStep>(lo, mid, hi) : at;
  const int32_t right = x0 + B + kStep < n ? byte_at<4 + B + kStep>(lo, mid, hi) : at;
  return left + 2 * at + right;
}

template <int kStep>
__device__ __forceinline__ void sharpen_column(const uint32_t (*stage)[kStageDwords], const UnsharpPlane& d, unsigned gx, unsigned gy0, int r0,
                                               int k) {
  const unsigned x0 = 4u * gx, n = d.width_bytes;
  const int32_t amount = static_cast<int32_t>(d.amount), threshold = static_cast<int32_t>(d.threshold);
  int32_t h[kLaneRows + 2][4];
  uint32_t at[kLaneRows + 2];
#pragma unroll
  for (int r = 0; r < kLaneRows + 2; ++r) {
    const uint32_t lo = stage[r0 + r][k], mid = stage[r0 + r][k + 1], hi = stage[r0 + r][k + 2];
    at[r] = mid;
    h[r][0] = row_sum<kStep, 0>(lo, mid, hi, x0, n);
    h[r][1] = row_sum<kStep, 1>(lo, mid, hi, x0, n);
    h[r][2] = row_sum<kStep, 2>(lo, mid, hi, x0, n);
    h[r][3] = row_sum<kStep, 3>(lo, mid, hi, x0, n);
  }
#pragma unroll
  for (int j = 0; j < kLaneRows; ++j) {
    if (gy0 + j >= d.rows) break;
    uint32_t out = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int32_t p = static_cast<int32_t>((at[j + 1] >> (8 * b)) & 255u);
      const int32_t S = sjpeg_internal::unsharp_blur16(h[j][b], h[j + 1][b], h[j + 2][b]);
      out |= static_cast<uint32_t>(sjpeg_internal::unsharp_apply(p, S, amount, threshold)) << (8 * b);
    }
    *((GlobalOut)(d.dst + static_cast<size_t>(gy0 + j) * d.dst_stride + 4u * gx)) = out;
  }
}

__global__ __launch_bounds__(256) void unsharp_kernel(const UnsharpArgs a) {
  __shared__ uint32_t stage[kStageRows][kStageDwords];
  const unsigned wg = blockIdx.x, tid = threadIdx.x;
  int lo = 0, hi = a.nplanes - 1;
  while (lo < hi) {                                                // (the LAST plane whose first tile is not behind wg)
    const int mid = (lo + hi + 1) >> 1;
    if (a.planes[mid].tile_base <= wg) lo = mid; else hi = mid - 1;
  }
  const UnsharpPlane d = a.planes[lo];
  const unsigned ndw = (d.width_bytes + 3u) / 4u;                  // dwords that begin inside the row's samples
  const unsigned tiles_x = (ndw + kTileDwords - 1) / kTileDwords;
  const unsigned t = wg - d.tile_base;
  const unsigned ty = t / tiles_x, tx = t - ty * tiles_x;
  const int dw0 = static_cast<int>(tx) * kTileDwords, row0 = static_cast<int>(ty) * kTileRows;
  if (static_cast<unsigned>(row0) >= d.rows) return;               // (a grid larger than the plan's: nothing of this plane)
  for (int i = static_cast<int>(tid); i < kStageRows * kStageDwords; i += 256) {
    const int r = i / kStageDwords, k = i - r * kStageDwords;
    int y = row0 + r - 1, g = dw0 + k - 1;
    y = y < 0 ? 0 : y > static_cast<int>(d.rows) - 1 ? static_cast<int>(d.rows) - 1 : y;
    g = g < 0 ? 0 : g > static_cast<int>(ndw) - 1 ? static_cast<int>(ndw) - 1 : g;
    stage[r][k] = *((GlobalIn)(d.src + static_cast<size_t>(y) * d.src_stride + 4u * static_cast<unsigned>(g)));
  }
  __syncthreads();
  const int k = static_cast<int>(tid & 63u), r0 = static_cast<int>(tid >> 6) * kLaneRows;
  const unsigned gx = static_cast<unsigned>(dw0 + k), gy0 = static_cast<unsigned>(row0 + r0);
  if (gx >= ndw || gy0 >= d.rows) return;
  if (d.step == 3u) sharpen_column<3>(stage, d, gx, gy0, r0, k); else sharpen_column<1>(stage, d, gx, gy0, r0, k);
}

}  // namespace

namespace sjpeg_internal {

int unsharp_launch(const UnsharpPlane* d_planes, int nplanes, unsigned tiles, hipStream_t st) {
  UnsharpArgs a;
  a.planes = d_planes;
  a.nplanes = nplanes;
  hipLaunchKernelGGL(unsharp_kernel, dim3(tiles), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace sjpeg_internal
