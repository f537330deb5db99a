// resample.hip -- pictures of a ragged batch resampled with Pillow's filters on gfx950: box, bilinear, Hamming, bicubic
// and Lanczos windows, to a size larger or smaller on either axis, in ONE launch in front of the ragged encodes
// (sjpeg_hip_resample_ragged_src, sjpeg_hip_encode_ragged_resampled_src; sjpeg_hip.h).
//
// Reference: none in the encoder -- the reference codes the picture it is given.  The contract is on the bytes: a
// sample is resample_math.h's accumulate-and-clip of the tables the host built, along x, then along y, with a uint8
// intermediate: Image.resize of Pillow.  The kernel is integers only; a source byte is what the encoder sees there
// (pixel_elem.h for floats, flatten_math.h under a flatten).
//
// Shape: a flat grid over the batch's tiles, a workgroup one tile of tw x 16 samples of one frame's resampled picture,
// found by the binary search over the frames' first tiles that resize.hip and unsharp.hip use -- so the sizes, the
// tables and the format's fields are wave-uniform.  The workgroup walks the source rows that the tile's y-windows cover
// in chunks of R rows.  Per chunk it STAGES each row's segment -- the union of the tile's x-windows -- as bytes in LDS,
// as resize.hip does: packed pixels as they lie in memory, else a run of bytes per channel.  Then the horizontal pass: a
// thread owns one column of the tile (a sample and channel) and every G-th row of the chunk; it reads a coefficient once
// and multiplies it into up to eight rows' sums, which leave clipped as the uint8 INTERMEDIATE in LDS.  Behind a barrier
// the vertical pass: every output sample (up to six a thread) adds the chunk's rows that lie in its y-window, weighted
// -- the chunk's 16 x 16 vertical coefficients lie in LDS, fetched one a thread --, to its int32 sum in a register.
// After the last chunk the sums are clipped into the byte tile and leave as whole dwords.  A pass that is not run has the identity table -- one tap of 2^22, which gives the byte back.  No atomics, no
// scratch; every byte read is one of the picture's.
//
// What the kernel relies on, checked by the plan for every table (resample_plan.cc): |K| < 2^23, so K * b is a 24-bit
// multiply; no partial sum of a sample leaves an int32; every window lies inside its axis and the windows' two ends
// are in order, so a tile's segment is [first sample's xmin, last sample's xmin + n); the segment is at most
// kResampleSegmentMax pixels, so one row always fits the stage.
//
// A frame with an EXIF orientation other than 1 stores its samples byte by byte where orient_math.h puts them in the
// upright picture: the made pictures are small.  An unturned tile leaves as whole dwords: tw is a multiple of 4, the
// last dword of a row may reach into the row's padding (zeros), never past it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "flatten_math.h"
#include "orient_math.h"
#include "pixel_elem.h"
#include "ragged_aux.h"
#include "resample_math.h"
#include "sjpeg_hip.h"
#include "source_layout.h"

namespace {

using sjpeg_internal::ResampleFrame;
using sjpeg_internal::kResampleHalf;
using sjpeg_internal::resample_clip;
using sjpeg_internal::resample_mac;

// how a row's segment is staged
enum { kPacked = 0, kPlanes = 1, kElems = 2 };

constexpr unsigned kStageBytes = sjpeg_internal::kResampleStageBytes;
constexpr int kTileCols = static_cast<int>(sjpeg_internal::kResampleTileCols), kTileRows = static_cast<int>(sjpeg_internal::kResampleTileRows);
constexpr int kTilePitch = kTileCols * 3;                          // bytes a row of the tile and of the intermediate
constexpr int kRowsPerThread = 8;                                  // horizontal pass: rows of a chunk a thread sums
constexpr int kOutPerThread = kTileRows * kTilePitch / 256;        // vertical pass: samples a thread sums
static_assert(kTilePitch * 2 <= 256, "at least two row groups: 2 * kRowsPerThread rows a chunk");
static_assert(kRowsPerThread * 2 >= kTileRows, "a chunk holds at most kTileRows rows");
static_assert(kOutPerThread * 256 == kTileRows * kTilePitch, "the tile's samples divide among the threads");
static_assert(kTileRows * kTileRows == 256, "a thread fetches one vertical coefficient a chunk");
static_assert(sjpeg_internal::kResampleSegmentMax * 4 <= kStageBytes, "a segment of four-byte pixels fits the stage");

struct ResampleArgs {
  const ResampleFrame* frames;
  int nframes;
  int kind;                      // kElem* (pixel_elem.h)
  int pix_step;                  // bytes from a pixel to the next
  int channels;                  // 3, or 1 for the gray formats
  float pscale[3], pbias[3];     // the engine's pixel transform (float formats)
  uint32_t bg[3];                // the flat instantiations: the background, R, G, B
  int premultiplied;
  float ascale, abias;           // the alpha sample's transform (float formats)
};

// The pictures and tables lie in device memory (reduce.hip says why this is said); a source dword is aligned like a byte.
typedef uint32_t __attribute__((aligned(1))) Dword1;
typedef const __attribute__((address_space(1))) Dword1* GlobalDwords;
typedef const __attribute__((address_space(1))) uint8_t* GlobalBytes;
typedef const __attribute__((address_space(1))) int32_t* GlobalInts;
typedef __attribute__((address_space(1))) uint32_t* GlobalOut;
typedef __attribute__((address_space(1))) uint8_t* GlobalOutBytes;

__device__ __forceinline__ unsigned align4(unsigned n) { return (n + 3u) & ~3u; }

// nb bytes of a source row at g into LDS at l (a multiple of 4), by the `lanes` threads of which this is `lane`: whole
// dwords, the last 1..3 bytes one by one -- every byte read is one of the nb
__device__ __forceinline__ void stage_bytes(const uint8_t* g, uint8_t* l, unsigned nb, unsigned lane, unsigned lanes) {
  const unsigned nd = nb >> 2;
  GlobalDwords const gd = (GlobalDwords)(g);
  uint32_t* const ld = reinterpret_cast<uint32_t*>(l);
  for (unsigned i = lane; i < nd; i += lanes) ld[i] = gd[i];
  const unsigned i = (nd << 2) + lane;
  if (i < nb) l[i] = ((GlobalBytes)(g))[i];
}

// kCls: how the format's rows are staged; kFlat: the frames are of an alpha format (four-byte pixels: the packed class;
// float RGBA: the element class) and are flattened as they are staged.  Compile-time, as in resize.hip: an instantiation
// holds its own staging alone, and the arguments the others read are not loaded.
template <int kCls, bool kFlat>
__global__ __launch_bounds__(256) void resample_kernel(const ResampleArgs a) {
  static_assert(!(kFlat && kCls == kPlanes), "a format with alpha is packed pixels or float elements");
  __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
  __shared__ __attribute__((aligned(16))) uint8_t mid[kTileRows * kTilePitch];
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTileRows * kTilePitch];
  __shared__ int32_t wky[kTileRows * kTileRows];                   // a chunk's vertical coefficients, [tile row][chunk row]
  const unsigned wg = blockIdx.x, tid = threadIdx.x;
  int flo = 0, fhi = a.nframes - 1;
  while (flo < fhi) {                                              // (the LAST frame whose first tile is not behind wg)
    const int m = (flo + fhi + 1) >> 1;
    if (a.frames[m].tile_base <= wg) flo = m; else fhi = m - 1;
  }
  const ResampleFrame& d = a.frames[flo];                         // (read where it is used: a copy would live in SGPRs throughout)
  const unsigned t = wg - d.tile_base, tyi = t / d.tiles_x, txi = t - tyi * d.tiles_x;
  const int ox0 = static_cast<int>(txi) * d.tw, oy0 = static_cast<int>(tyi) * kTileRows;
  if (oy0 >= d.h2) return;                                         // (a grid larger than the plan's: nothing of this frame)
  const int tw = min(d.tw, d.w2 - ox0), th = min(kTileRows, d.h2 - oy0);
  const int channels = a.channels, cols = tw * channels;
  GlobalInts const xb = (GlobalInts)(d.xb), xk = (GlobalInts)(d.xk), yb = (GlobalInts)(d.yb), yk = (GlobalInts)(d.yk);
  // the tile's segment of a source row and its source rows: the windows' ends are in order (the plan checked)
  const int xs = xb[2 * ox0], xe = xb[2 * (ox0 + tw - 1)] + xb[2 * (ox0 + tw - 1) + 1];
  const int ys = yb[2 * oy0], ye = yb[2 * (oy0 + th - 1)] + yb[2 * (oy0 + th - 1) + 1];
  // the staged rows: packed pixels as they lie in memory, else a run of bytes per channel
  constexpr bool packed = kCls == kPacked;
  const unsigned lstep = packed ? static_cast<unsigned>(a.pix_step) : 1u;
  const unsigned seg = static_cast<unsigned>(xe - xs);
  const unsigned cpitch = packed ? 0u : align4(seg);
  const unsigned rpitch = packed ? align4(seg * lstep) : cpitch * static_cast<unsigned>(channels);
  const int R = min(kTileRows, static_cast<int>(kStageBytes / rpitch));
  unsigned coff[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) coff[c] = packed ? static_cast<unsigned>(d.off[c]) : static_cast<unsigned>(c) * cpitch;
  // who stages what: a wave a row, or the whole workgroup the one row of a chunk
  const unsigned slanes = R == 1 ? 256u : 64u, slane = tid & (slanes - 1u), srow = tid / slanes, srows = 256u / slanes;

  for (unsigned i = tid; i < kTileRows * kTilePitch / 4u; i += 256u) reinterpret_cast<uint32_t*>(tile)[i] = 0u;   // (the rows' padding)

  // horizontal pass: my column of the tile, my rows of a chunk
  const int G = 256 / cols;                                        // row groups: at least 2
  const int hcol = static_cast<int>(tid) % cols, rg = static_cast<int>(tid) / cols;
  const bool hactive = rg < G;
  const int hj = hcol / channels, hc = hcol - hj * channels;
  const int hxmin = xb[2 * (ox0 + hj)], hn = hactive ? xb[2 * (ox0 + hj) + 1] : 0;
  GlobalInts const hk = xk + static_cast<size_t>(ox0 + hj) * static_cast<size_t>(d.ksx);
  const uint8_t* const hp = stage + static_cast<unsigned>(hxmin - xs) * lstep + (hc == 0 ? coff[0] : hc == 1 ? coff[1] : coff[2]);

  // vertical pass: the coefficient I fetch per chunk -- tile row wr's for the chunk's row wy --
  const int wr = static_cast<int>(tid) >> 4, wy = static_cast<int>(tid) & 15;
  const int wmin = wr < th ? yb[2 * (oy0 + wr)] : 0, wend = wr < th ? wmin + yb[2 * (oy0 + wr) + 1] : 0;
  GlobalInts const wk = yk + static_cast<size_t>(oy0 + (wr < th ? wr : 0)) * static_cast<size_t>(d.ksy) - wmin;
  // ... and my samples of the tile: tile row * 256 + column (-1: none), and their sums
  int vat[kOutPerThread];
  int32_t vacc[kOutPerThread];
#pragma unroll
  for (int i = 0; i < kOutPerThread; ++i) {
    const int o = static_cast<int>(tid) + 256 * i;
    const int r = o / cols;
    vat[i] = r < th ? r * 256 + (o - r * cols) : -1;
    vacc[i] = kResampleHalf;
  }

  for (int y0 = ys; y0 < ye; y0 += R) {
    const int nr = min(R, ye - y0);
    for (unsigned r = srow; r < static_cast<unsigned>(nr); r += srows) {
      const uint8_t* const row = d.src + static_cast<long long>(y0 + static_cast<int>(r)) * d.row_stride;
      uint8_t* const l = stage + r * rpitch;
      if constexpr (kFlat && packed) {
        // four-byte pixels: row + xs * 4 is a pixel boundary and l a multiple of 4; alpha is the last byte.  The colour
        // bytes are replaced, the alpha byte stays (nothing reads it)
        GlobalDwords const gd = (GlobalDwords)(row + static_cast<long long>(xs) * 4);
        uint32_t* const ld = reinterpret_cast<uint32_t*>(l);
        for (unsigned k = slane; k < seg; k += slanes) {
          const uint32_t v = gd[k], al = v >> 24;
          uint32_t o = v & 0xff000000u;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const unsigned sh = coff[c] * 8u;
            o |= sjpeg_internal::flatten_byte(al, (v >> sh) & 255u, a.bg[c], a.premultiplied != 0) << sh;
          }
          ld[k] = o;
        }
      } else if constexpr (packed) {
        stage_bytes(row + static_cast<long long>(xs) * lstep, l, seg * lstep, slane, slanes);
      } else if constexpr (kCls == kPlanes) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (c < channels) stage_bytes(row + d.off[c] + xs, l + c * cpitch, seg, slane, slanes);
        }
      } else {
        // the float formats, a pixel at a time: never an element that is not a used sample of a pixel of the picture
        for (unsigned k = slane; k < seg; k += slanes) {
          const uint8_t* const px = row + static_cast<long long>(xs + static_cast<int>(k)) * a.pix_step;
          uint32_t al = 0u;
          if constexpr (kFlat) al = static_cast<uint32_t>(sjpeg_internal::elem_load_u8(px + 3 * (a.pix_step >> 2), a.kind, a.ascale, a.abias));
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            if (c >= channels) continue;
            uint32_t b = static_cast<uint32_t>(sjpeg_internal::elem_load_u8(px + d.off[c], a.kind, a.pscale[c], a.pbias[c]));
            if constexpr (kFlat) b = sjpeg_internal::flatten_byte(al, b, a.bg[c], a.premultiplied != 0);
            l[c * cpitch + k] = static_cast<uint8_t>(b);
          }
        }
      }
    }
    __syncthreads();
    {
      // the chunk's vertical coefficients: tile row wr's for source row y0 + wy, one a thread (0 outside the window)
      const int y = y0 + wy;
      wky[tid] = y >= wmin && y < wend && wy < nr ? wk[y] : 0;
    }
    {
      int32_t acc[kRowsPerThread];
#pragma unroll
      for (int m = 0; m < kRowsPerThread; ++m) acc[m] = kResampleHalf;
      auto tap = [&](int32_t k, int x) {
        const uint8_t* const p = hp + static_cast<unsigned>(x) * lstep;
#pragma unroll
        for (int m = 0; m < kRowsPerThread; ++m) {
          const int r = rg + G * m;
          if (r < nr) acc[m] = resample_mac(acc[m], k, p[static_cast<unsigned>(r) * rpitch]);
        }
      };
      int x = 0;
      for (; x + 2 <= hn; x += 2) {                                // (two coefficients in flight: the loads are the latency)
        const int32_t k0 = hk[x], k1 = hk[x + 1];
        tap(k0, x); tap(k1, x + 1);
      }
      for (; x < hn; ++x) tap(hk[x], x);
      if (hactive) {
#pragma unroll
        for (int m = 0; m < kRowsPerThread; ++m) {
          const int r = rg + G * m;
          if (r < nr) mid[r * kTilePitch + hcol] = static_cast<uint8_t>(resample_clip(acc[m]));
        }
      }
    }
    __syncthreads();
    // (a coefficient outside a sample's window is 0: every sample walks the whole chunk)
    for (int yy = 0; yy < nr; ++yy) {
#pragma unroll
      for (int i = 0; i < kOutPerThread; ++i) {
        if (vat[i] >= 0) vacc[i] = resample_mac(vacc[i], wky[(vat[i] >> 8) * kTileRows + yy], mid[yy * kTilePitch + (vat[i] & 255)]);
      }
    }
    // (the next chunk's horizontal pass writes `mid` behind the barrier that follows its staging)
  }
#pragma unroll
  for (int i = 0; i < kOutPerThread; ++i) {
    if (vat[i] >= 0) tile[(vat[i] >> 8) * kTilePitch + (vat[i] & 255)] = static_cast<uint8_t>(resample_clip(vacc[i]));
  }
  __syncthreads();
  const int orient = static_cast<int>(d.orient);
  if (orient <= 1) {
    // the tile as whole dwords of the made rows: its first byte is a multiple of 4 (tw is)
    const unsigned ndw = (static_cast<unsigned>(cols) + 3u) >> 2;
    for (unsigned i = tid; i < static_cast<unsigned>(th) * ndw; i += 256u) {
      const unsigned r = i / ndw, k = i - r * ndw;
      uint8_t* const out = d.dst + static_cast<size_t>(oy0 + static_cast<int>(r)) * d.dst_stride + static_cast<size_t>(ox0) * channels;
      ((GlobalOut)(out))[k] = reinterpret_cast<const uint32_t*>(tile + r * kTilePitch)[k];
    }
    return;
  }
  // a turned frame: every sample's bytes where the upright picture has them
  for (unsigned i = tid; i < static_cast<unsigned>(th * cols); i += 256u) {
    const unsigned r = i / static_cast<unsigned>(cols), cb = i - r * static_cast<unsigned>(cols);
    const unsigned j = cb / static_cast<unsigned>(channels), c = cb - j * static_cast<unsigned>(channels);
    uint32_t ux, uy;
    sjpeg_internal::orient_upright(static_cast<uint32_t>(ox0) + j, static_cast<uint32_t>(oy0) + r, static_cast<uint32_t>(d.w2),
                                   static_cast<uint32_t>(d.h2), orient, &ux, &uy);
    ((GlobalOutBytes)(d.dst))[static_cast<size_t>(uy) * d.dst_stride + static_cast<size_t>(ux) * channels + c] = tile[r * kTilePitch + cb];
  }
}

}  // namespace

namespace sjpeg_internal {

int resample_launch(int format, const float* pscale, const float* pbias, const sjpeg_hip_flatten* flatten, const ResampleFrame* d_frames,
                    int nframes, unsigned tiles, hipStream_t st) {
  const SourceLayout& L = *source_layout(format);
  ResampleArgs a;
  memset(&a, 0, sizeof(a));
  a.frames = d_frames;
  a.nframes = nframes;
  a.kind = L.kind;
  a.channels = L.rgb_like ? 3 : 1;
  a.pix_step = L.plane[0].step * L.esz;
  const int cls = L.kind != kElemU8 ? kElems : (L.one_pitch || a.channels == 1) ? kPlanes : kPacked;
  for (int c = 0; c < 3; ++c) { a.pscale[c] = pscale[c]; a.pbias[c] = pbias[c]; }
  if (flatten != nullptr) {
    // (four bytes or four elements a pixel: resample_plan checked it)
    for (int c = 0; c < 3; ++c) a.bg[c] = flatten->background[c];
    a.premultiplied = flatten->premultiplied;
    a.ascale = flatten->alpha_scale;
    a.abias = flatten->alpha_bias;
    if (cls == kElems) {
      hipLaunchKernelGGL((resample_kernel<kElems, true>), dim3(tiles), dim3(256), 0, st, a);
    } else {
      hipLaunchKernelGGL((resample_kernel<kPacked, true>), dim3(tiles), dim3(256), 0, st, a);
    }
  } else if (cls == kElems) {
    hipLaunchKernelGGL((resample_kernel<kElems, false>), dim3(tiles), dim3(256), 0, st, a);
  } else if (cls == kPlanes) {
    hipLaunchKernelGGL((resample_kernel<kPlanes, false>), dim3(tiles), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((resample_kernel<kPacked, false>), dim3(tiles), dim3(256), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace sjpeg_internal
