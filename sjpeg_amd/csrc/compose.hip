// compose.hip -- the compose stage over the made pictures of a ragged batch on gfx950 (sjpeg_hip_compose_ragged_src and
// the _composed_ entries; sjpeg_hip.h): every picture copied onto its canvas -- Pillow's ImageOps.pad / expand -- and
// the frame's overlays blended over it in list order -- Pillow's paste of an RGBA picture with itself as mask --, by
// ONE launch behind the launches that made the pictures, out of place; never one per picture, overlay or place.
//
// Reference: none -- the reference codes the samples it is given.  The contract is on the bytes: Pillow 12.2.0's, by
// the definition in sjpeg_hip.h and compose_math.h.  Integers only: sizes, places and anchors are resolved on the host.
//
// Shape: a flat grid over the tiles of every canvas, a workgroup one tile of one canvas, found by the binary search
// over the canvases' first tiles that unsharp.hip and pillow_filter.hip use -- so the descriptor and its at most 8
// places are wave-uniform.  A tile is kComposeTileDwords dwords of a canvas row x kComposeTileRows rows; a lane makes
// one dword column of four rows, 64 lanes a row of the tile: 256 contiguous bytes a wave-load and a wave-store.  A
// canvas dword is composed in registers and stored once: its bytes are background or picture byte by byte, then every
// place whose rectangle meets the tile (a uniform branch skips the others) blends the bytes it covers.  The picture's
// bytes for a canvas dword begin at any byte phase -- 3 * px has any --: they are the two aligned dwords around them,
// shifted together; the phase is the frame's, so the branch on it is uniform.  An overlay pixel is one aligned dword.
// A tile wholly in background or wholly in the picture and under no overlay takes the short path: fill or copy.  A
// frame without compose is a canvas of its picture's size: all short path, a copy.
//
// A made picture and a canvas start at a multiple of 4 and 16 with rows whole dwords apart, an overlay at a multiple of
// 4 with a stride of whole dwords: every global access is an aligned dword inside a row's dwords (a canvas row's last
// may hold padding, which no sample reads; what lands there is unspecified).  Nothing is read or written outside the
// canvas rows, the made picture's rows or the overlay's rows.  No atomics, no LDS, no lane reads what another
// workgroup writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compose_math.h"
#include "ragged_aux.h"

// (tests/cxx/compose_kernel_emul.cc sees every access through this: the address and 0 made, 1 canvas, 2 overlay)
#ifndef SJPEG_COMPOSE_ACCESS
#define SJPEG_COMPOSE_ACCESS(p, what) ((void)0)
#endif

namespace {

using sjpeg_internal::ComposeFrame;
using sjpeg_internal::ComposePlace;

constexpr int kTileDwords = static_cast<int>(sjpeg_internal::kComposeTileDwords), kTileRows = static_cast<int>(sjpeg_internal::kComposeTileRows);
constexpr int kLaneRows = kTileRows / 4;                            // rows a lane makes, four rows apart
static_assert(kTileDwords == 64 && kTileRows % 4 == 0, "a wave is one row of the tile, the workgroup four");

struct ComposeArgs {
  const ComposeFrame* frames;
  int nframes;
};

// The pictures lie in device memory (reduce.hip says why this is said)
typedef const __attribute__((address_space(1))) uint32_t* GlobalIn;
typedef __attribute__((address_space(1))) uint32_t* GlobalOut;

__device__ __forceinline__ uint32_t load_dword(const uint8_t* p, int what) {
  SJPEG_COMPOSE_ACCESS(p, what);
  return *((GlobalIn)p);
}
__device__ __forceinline__ void store_dword(uint8_t* p, uint32_t v) {
  SJPEG_COMPOSE_ACCESS(p, 1);
  *((GlobalOut)p) = v;
}

// The four bytes of a made row that begin at byte s of it (s any int; bytes outside the row's ndw dwords read as 0):
// the aligned dwords around them shifted together
__device__ __forceinline__ uint32_t fetch_bytes(const uint8_t* row, int s, int ndw) {
  const int q = s >> 2, ph = s & 3;
  const uint32_t lo = q >= 0 && q < ndw ? load_dword(row + 4 * q, 0) : 0u;
  if (ph == 0) return lo;
  const uint32_t hi = q + 1 >= 0 && q + 1 < ndw ? load_dword(row + 4 * (q + 1), 0) : 0u;
  return (lo >> (8 * ph)) | (hi << (32 - 8 * ph));
}

// the canvas's colour in the dword that begins at byte B of a row
__device__ __forceinline__ uint32_t colour_dword(unsigned B, unsigned step, unsigned colour) {
  if (step == 1u) return (colour & 255u) * 0x01010101u;
  const uint64_t rgb = colour & 0xffffffu, six = rgb | rgb << 24;   // R G B R G B
  return static_cast<uint32_t>(six >> (8u * (B % 3u)));
}

__global__ __launch_bounds__(256) void compose_kernel(const ComposeArgs a) {
  const unsigned wg = blockIdx.x;
  const int tid = static_cast<int>(threadIdx.x);
  int lo = 0, hi = a.nframes - 1;
  while (lo < hi) {                                                // (the LAST canvas whose first tile is not behind wg)
    const int mid = (lo + hi + 1) >> 1;
    if (a.frames[mid].tile_base <= wg) lo = mid; else hi = mid - 1;
  }
  const ComposeFrame* const F = a.frames + lo;
  const int step = static_cast<int>(F->step), cw = static_cast<int>(F->cw), ch = static_cast<int>(F->ch);
  const int py = static_cast<int>(F->py), h = static_cast<int>(F->h);
  const int ndw = static_cast<int>(F->dst_stride >> 2);            // dwords that begin inside a canvas row's samples
  const int src_ndw = (static_cast<int>(F->w) * step + 3) >> 2;    // ... a made row's
  const unsigned src_stride = F->src_stride, dst_stride = F->dst_stride, colour = F->colour;
  const uint8_t* const made = F->made;
  uint8_t* const dst = F->dst;
  const unsigned t = wg - F->tile_base;
  const unsigned tiles_x = (static_cast<unsigned>(ndw) + kTileDwords - 1) / kTileDwords;
  const unsigned ty = t / tiles_x, tx = t - ty * tiles_x;
  const int g0 = static_cast<int>(tx) * kTileDwords, y0 = static_cast<int>(ty) * kTileRows;
  if (y0 >= ch) return;                                            // (a grid larger than the plan's: nothing of this canvas)
  const int g1 = g0 + kTileDwords < ndw ? g0 + kTileDwords : ndw, y1 = y0 + kTileRows < ch ? y0 + kTileRows : ch;
  const int row_bytes = cw * step;
  const int tb0 = 4 * g0, tb1 = 4 * g1 < row_bytes ? 4 * g1 : row_bytes;    // the tile's sample bytes of a row: [tb0, tb1)
  const int pb0 = static_cast<int>(F->px) * step, pb1 = pb0 + static_cast<int>(F->w) * step;   // the picture's: [pb0, pb1)

  // the places that meet the tile, as a bit each
  const int nplaces = static_cast<int>(F->nplaces);
  const int tx0 = tb0 / step, tx1 = (tb1 - 1) / step;              // the tile's first and last pixel of a row
  unsigned meets = 0;
  for (int i = 0; i < nplaces; ++i) {
    const ComposePlace* const p = &F->place[i];
    const int ox = p->ox, oy = p->oy;
    if (ox <= tx1 && ox + static_cast<int>(p->ow) > tx0 && oy < y1 && oy + static_cast<int>(p->oh) > y0) meets |= 1u << i;
  }
  const bool all_background = y1 <= py || y0 >= py + h || tb1 <= pb0 || tb0 >= pb1;
  const bool all_picture = y0 >= py && y1 <= py + h && tb0 >= pb0 && tb1 <= pb1;

  const int g = g0 + (tid & (kTileDwords - 1)), r0 = y0 + (tid >> 6);
  if (g >= g1) return;
  const int B = 4 * g;
  const uint32_t ground = colour_dword(static_cast<unsigned>(B), static_cast<unsigned>(step), colour);

  if (meets == 0u && (all_background || all_picture)) {            // the short path: fill or copy
#pragma unroll
    for (int j = 0; j < kLaneRows; ++j) {
      const int y = r0 + 4 * j;
      if (y >= y1) break;
      const uint32_t v = all_background ? ground : fetch_bytes(made + static_cast<size_t>(y - py) * src_stride, B - pb0, src_ndw);
      store_dword(dst + static_cast<size_t>(y) * dst_stride + static_cast<unsigned>(B), v);
    }
    return;
  }

  // which bytes of this lane's dword are the picture's, in the picture's rows
  uint32_t inside = 0u;
#pragma unroll
  for (int b = 0; b < 4; ++b) if (B + b >= pb0 && B + b < pb1) inside |= 255u << (8 * b);

  uint32_t v[kLaneRows];
#pragma unroll
  for (int j = 0; j < kLaneRows; ++j) {
    const int y = r0 + 4 * j;
    v[j] = ground;
    if (y < y1 && y >= py && y < py + h && inside != 0u) {
      const uint32_t p = fetch_bytes(made + static_cast<size_t>(y - py) * src_stride, B - pb0, src_ndw);
      v[j] = (p & inside) | (ground & ~inside);
    }
  }

  for (int i = 0; i < nplaces; ++i) {
    if ((meets >> i & 1u) == 0u) continue;                         // (uniform)
    const ComposePlace* const p = &F->place[i];
    const int ox = p->ox, oy = p->oy, ow = static_cast<int>(p->ow), oh = static_cast<int>(p->oh);
    const unsigned ostride = p->stride;
    const uint8_t* const rgba = p->rgba;
#pragma unroll
    for (int j = 0; j < kLaneRows; ++j) {
      const int y = r0 + 4 * j;
      if (y >= y1 || y < oy || y >= oy + oh) continue;
      const uint8_t* const orow = rgba + static_cast<size_t>(y - oy) * ostride;
      int have = -1;                                               // the overlay pixel `texel` holds
      uint32_t texel = 0u, out = v[j];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int c = B + b;
        if (c >= row_bytes) continue;
        const int x = step == 3 ? static_cast<int>(static_cast<unsigned>(c) / 3u) : c;
        const int k = step == 3 ? c - 3 * x : 0;
        const int u = x - ox;
        if (u < 0 || u >= ow) continue;
        if (u != have) { texel = load_dword(orow + 4 * u, 2); have = u; }
        const uint32_t src = step == 3 ? (texel >> (8 * k)) & 255u
                                       : sjpeg_internal::compose_luma(texel & 255u, (texel >> 8) & 255u, (texel >> 16) & 255u);
        const uint32_t made_byte = sjpeg_internal::compose_blend((out >> (8 * b)) & 255u, src, texel >> 24);
        out = (out & ~(255u << (8 * b))) | made_byte << (8 * b);
      }
      v[j] = out;
    }
  }

#pragma unroll
  for (int j = 0; j < kLaneRows; ++j) {
    const int y = r0 + 4 * j;
    if (y < y1) store_dword(dst + static_cast<size_t>(y) * dst_stride + static_cast<unsigned>(B), v[j]);
  }
}

}  // namespace

namespace sjpeg_internal {

int compose_launch(const ComposeFrame* d_frames, int nframes, unsigned tiles, hipStream_t st) {
  ComposeArgs a;
  a.frames = d_frames;
  a.nframes = nframes;
  hipLaunchKernelGGL(compose_kernel, dim3(tiles), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace sjpeg_internal
