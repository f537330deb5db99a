// pillow_filter.hip -- Pillow's BoxBlur, GaussianBlur and UnsharpMask over the made pictures of a ragged batch on
// gfx950 (sjpeg_hip_filter_ragged_src and the _filtered_ entries; sjpeg_hip.h): pillow_filter_math.h's passes in TWO
// launches behind the launch that made the pictures -- every pass along the rows from the made pictures to a scratch
// buffer of the same layout, every pass along the columns from there to the output -- never one per pass or picture.
//
// Reference: none -- the reference codes the samples it is given.  The contract is on the bytes: Pillow 12.2.0's, by
// the definition in sjpeg_hip.h.  Integers only: the weights r, ww, fw of an axis come from the host.
//
// Shape: each launch a flat grid over the batch's tiles, a workgroup one tile of one picture, found by the binary
// search over the pictures' first tiles that unsharp.hip uses -- so the descriptor, the pixel step, r, ww, fw and the
// pass count are wave-uniform.  A tile is kPillowRowTilePixels pixels x kPillowRowTileRows rows (row launch) or
// kPillowColTileDwords dwords x kPillowColTileRows rows (column launch).  Along the axis the workgroup stages the tile's
// positions [t0, e) and a halo of passes * (r + 1) positions on each side, CUT OFF at the line's ends, as whole aligned
// dwords into LDS.  Pass k of P then runs from one LDS buffer to the other over region k = [max(t0 - (P - k)(r + 1), 0),
// min(e + (P - k)(r + 1), n)): every index a sample reads is clamped into 0 .. n - 1 first, and a clamped index of
// region k lies in region k - 1 -- the replicated edge of an intermediate IS the intermediate at the clamped index, so
// nothing outside the line is ever staged or computed, at a seam the halo holds the neighbour tile's intermediates
// recomputed, and the channel is kept because positions count pixels.  A lane makes a run of kRun consecutive samples
// of one line with a sliding sum: 2 r + 1 LDS reads to start, two a sample after that.  Behind the last pass the tile
// leaves as aligned dwords; the column launch reads the made dword beside the blurred one where the kind is the
// unsharp mask.  A frame of kind 0 and a skipped axis have no passes: staged and stored, a copy by the same code.
//
// A made picture starts at a multiple of 16 with rows whole dwords apart: every global access is an aligned dword
// inside a row's dwords (the last may hold padding, which no sample reads; what lands there is unspecified).  A dword
// that begins at or beyond the row's samples, or a row beyond the picture, is not touched.  No atomics, no lane reads
// what another workgroup writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pillow_filter_math.h"
#include "ragged_aux.h"

namespace {

using sjpeg_internal::PillowFilterAxis;
using sjpeg_internal::PillowFilterPlane;

constexpr int kRowTile = static_cast<int>(sjpeg_internal::kPillowRowTilePixels), kRowRows = static_cast<int>(sjpeg_internal::kPillowRowTileRows);
constexpr int kColDwords = static_cast<int>(sjpeg_internal::kPillowColTileDwords), kColRows = static_cast<int>(sjpeg_internal::kPillowColTileRows);
constexpr int kRowLine = static_cast<int>(sjpeg_internal::kPillowRowLineBytes), kColLine = static_cast<int>(sjpeg_internal::kPillowColLineBytes);
constexpr int kStageDwords = static_cast<int>(sjpeg_internal::kPillowStageBytes / 4);
constexpr int kRun = 8;                                             // samples a lane makes in a row of one pass

struct PillowFilterArgs {
  const PillowFilterPlane* planes;
  int nplanes;
};

// The pictures lie in device memory (reduce.hip says why this is said)
typedef const __attribute__((address_space(1))) uint32_t* GlobalIn;
typedef __attribute__((address_space(1))) uint32_t* GlobalOut;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// One pass over `nlines` lines in LDS, in -> out.  Sample x of line j lies at byte line_at(j) + x * stride - origin.
// Made: positions [a, b); n: the line's samples, indices clamped into it.
template <class LineAt>
__device__ __forceinline__ void box_pass(const uint8_t* in, uint8_t* out, int nlines, LineAt line_at, int stride, int origin, int a, int b, int n,
                                         const PillowFilterAxis& w, int tid) {
  const int r = static_cast<int>(w.r), runs = (b - a + kRun - 1) / kRun;
  for (int it = tid; it < nlines * runs; it += 256) {
    const int run = it / nlines, line = it - run * nlines;
    const int x0 = a + run * kRun, x1 = x0 + kRun < b ? x0 + kRun : b;
    const int at = line_at(line) - origin;
    uint32_t S = 0;
    for (int d = -r; d <= r; ++d) S += in[at + clampi(x0 + d, 0, n - 1) * stride];
    uint32_t lo = in[at + clampi(x0 - r - 1, 0, n - 1) * stride];
    for (int x = x0; x < x1; ++x) {
      const uint32_t hi = in[at + clampi(x + r + 1, 0, n - 1) * stride];
      out[at + x * stride] = static_cast<uint8_t>(sjpeg_internal::pillow_box_sample(w.ww, w.fw, S, lo + hi));
      lo = in[at + clampi(x - r, 0, n - 1) * stride];             // (leaves the sum, and is the next sample's outer one)
      S += hi - lo;
    }
  }
}

// kAxis 0: along the rows, made -> mid.  kAxis 1: along the columns, mid (and made, for the unsharp mask) -> dst.
template <int kAxis>
__global__ __launch_bounds__(256) void pillow_filter_kernel(const PillowFilterArgs a) {
  __shared__ uint32_t stage[2][kStageDwords];
  const unsigned wg = blockIdx.x;
  const int tid = static_cast<int>(threadIdx.x);
  int lo = 0, hi = a.nplanes - 1;
  while (lo < hi) {                                                // (the LAST picture whose first tile is not behind wg)
    const int mid = (lo + hi + 1) >> 1;
    if (a.planes[mid].tile_base[kAxis] <= wg) lo = mid; else hi = mid - 1;
  }
  const PillowFilterPlane d = a.planes[lo];
  const PillowFilterAxis w = d.axis[kAxis];
  const int step = static_cast<int>(d.step), width = static_cast<int>(d.width), rows = static_cast<int>(d.rows);
  const int ndw = (width * step + 3) >> 2;                         // dwords that begin inside a row's samples
  const unsigned t = wg - d.tile_base[kAxis];
  const int P = static_cast<int>(w.passes), reach = static_cast<int>(w.r) + 1;
  const uint8_t* const src = kAxis == 0 ? d.made : d.mid;
  uint8_t* const dst = kAxis == 0 ? d.mid : d.dst;
  auto buf = [&](int i) { return reinterpret_cast<uint8_t*>(stage[i]); };

  if (kAxis == 0) {
    const unsigned tiles_x = (d.width + kRowTile - 1) / kRowTile;
    const unsigned ty = t / tiles_x, tx = t - ty * tiles_x;
    const int t0 = static_cast<int>(tx) * kRowTile, y0 = static_cast<int>(ty) * kRowRows;
    if (y0 >= rows) return;                                        // (a grid larger than the plan's: nothing of this picture)
    const int e = t0 + kRowTile < width ? t0 + kRowTile : width;
    const int nrows = y0 + kRowRows < rows ? kRowRows : rows - y0;
    const int s0 = clampi(t0 - P * reach, 0, width), s1 = clampi(e + P * reach, 0, width);
    const int g0 = (s0 * step) >> 2, g1 = (s1 * step + 3) >> 2;    // the staged dwords of a row: [g0, g1), inside [0, ndw)
    const int per = g1 - g0;
    for (int i = tid; i < nrows * per; i += 256) {
      const int l = i / per, g = g0 + (i - l * per);
      stage[0][l * (kRowLine / 4) + (g - g0)] = *((GlobalIn)(src + static_cast<size_t>(y0 + l) * d.stride + 4u * static_cast<unsigned>(g)));
    }
    __syncthreads();
    const int nlines = nrows * step, origin = 4 * g0;
    auto line_at = [&](int j) { const int l = j / step; return l * kRowLine + (j - l * step); };
    for (int k = 1; k <= P; ++k) {
      box_pass(buf((k - 1) & 1), buf(k & 1), nlines, line_at, step, origin, clampi(t0 - (P - k) * reach, 0, width),
               clampi(e + (P - k) * reach, 0, width), width, w, tid);
      __syncthreads();
    }
    const uint32_t* const done = stage[P & 1];
    const int o0 = (t0 * step) >> 2, o1 = (e * step + 3) >> 2;     // (t0 a multiple of 4: a whole dword)
    const int oper = o1 - o0;
    for (int i = tid; i < nrows * oper; i += 256) {
      const int l = i / oper, g = o0 + (i - l * oper);
      *((GlobalOut)(dst + static_cast<size_t>(y0 + l) * d.stride + 4u * static_cast<unsigned>(g))) = done[l * (kRowLine / 4) + (g - g0)];
    }
  } else {
    const unsigned tiles_x = (static_cast<unsigned>(ndw) + kColDwords - 1) / kColDwords;
    const unsigned ty = t / tiles_x, tx = t - ty * tiles_x;
    const int c0 = static_cast<int>(tx) * kColDwords, t0 = static_cast<int>(ty) * kColRows;
    if (t0 >= rows) return;
    const int e = t0 + kColRows < rows ? t0 + kColRows : rows;
    const int cols = c0 + kColDwords < ndw ? kColDwords : ndw - c0;  // dwords of the tile that begin inside the row
    const int s0 = clampi(t0 - P * reach, 0, rows), s1 = clampi(e + P * reach, 0, rows);
    for (int i = tid; i < (s1 - s0) * kColDwords; i += 256) {
      const int y = s0 + i / kColDwords, c = i % kColDwords;
      if (c < cols) stage[0][(y - s0) * (kColLine / 4) + c] = *((GlobalIn)(src + static_cast<size_t>(y) * d.stride + 4u * static_cast<unsigned>(c0 + c)));
    }
    __syncthreads();
    const int origin = s0 * kColLine;
    auto line_at = [&](int j) { return j; };
    for (int k = 1; k <= P; ++k) {
      box_pass(buf((k - 1) & 1), buf(k & 1), 4 * cols, line_at, kColLine, origin, clampi(t0 - (P - k) * reach, 0, rows),
               clampi(e + (P - k) * reach, 0, rows), rows, w, tid);
      __syncthreads();
    }
    const uint32_t* const done = stage[P & 1];
    const int32_t percent = static_cast<int32_t>(d.percent), threshold = static_cast<int32_t>(d.threshold);
    for (int i = tid; i < (e - t0) * kColDwords; i += 256) {
      const int y = t0 + i / kColDwords, c = i % kColDwords;
      if (c >= cols) continue;
      const size_t at = static_cast<size_t>(y) * d.stride + 4u * static_cast<unsigned>(c0 + c);
      uint32_t v = done[(y - s0) * (kColLine / 4) + c];
      if (d.kind == 3u) {
        const uint32_t p = *((GlobalIn)(d.made + at));
        uint32_t out = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          out |= sjpeg_internal::pillow_unsharp_sample(static_cast<int32_t>((p >> (8 * b)) & 255u), static_cast<int32_t>((v >> (8 * b)) & 255u), percent,
                                                       threshold) << (8 * b);
        }
        v = out;
      }
      *((GlobalOut)(dst + at)) = v;
    }
  }
}

}  // namespace

namespace sjpeg_internal {

int pillow_filter_launch(int launch, const PillowFilterPlane* d_planes, int nplanes, unsigned tiles, hipStream_t st) {
  PillowFilterArgs a;
  a.planes = d_planes;
  a.nplanes = nplanes;
  if (launch == 0) hipLaunchKernelGGL(pillow_filter_kernel<0>, dim3(tiles), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(pillow_filter_kernel<1>, dim3(tiles), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace sjpeg_internal
