// resample_box.hip -- resample.hip's kernel over frames that are REDUCED as they are staged: the pictures of
// Image.resize(size, filter, box=, reducing_gap=), Image.thumbnail and ImageOps.fit of Pillow 12.2.0, in ONE launch in
// front of the ragged encodes (sjpeg_hip_resample_box_ragged_src, sjpeg_hip_encode_ragged_resampled_box_src; sjpeg_hip.h).
//
// The contract is on the bytes (resample_math.h): a frame's picture is first Image.reduce((fx, fy), box=safe box) of the
// stored one -- a sample the sum S of its block of n source samples, fx * fy or fewer on the right and bottom edge,
// brought to ((S + n / 2) * m(n)) >> 24 with the multiplier the host divided in float32 -- and that picture is then
// resampled by the tables of its two axes as resample.hip does it, the box inside the tables.  A frame whose factors are
// 1 x 1 has m = 2^24 and is staged as it is.  A call in which no frame is reduced does not come here: its tables satisfy
// what resample.hip's kernel relies on, and it runs that one.
//
// Shape: resample.hip's, the tile, the chunks of source rows, the two passes and the store unchanged -- only that "source"
// means the REDUCED picture.  What differs is the loader.  A wave stages a row of the reduced picture's segment; a lane
// owns a staged pixel and sums its block: fy source rows, of each the run of fx pixels, which is contiguous -- the lane
// reads it as whole dwords from the run's first byte and the last 1..3 bytes one by one, so every byte read is one of the
// block's, and neighbouring lanes read neighbouring runs.  Packed pixels are summed by their byte's place in the pixel,
// planes a run per channel; a flattened or float pixel is transformed and flattened first and summed after, a pixel at a
// time.  The stage holds a run of bytes per channel for every class, so the horizontal pass reads it with step 1.
// Integers only behind the loader, no atomics, no scratch.
//
// What the kernel relies on, checked by the plan (resample_plan.cc): everything resample.hip's does, of the reduced
// picture's tables; the block of every reduced sample inside the safe box, the safe box inside the picture; (255 n +
// n / 2) * m(n) inside a uint32 for the four block sizes of a frame.
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

using sjpeg_internal::ResampleBoxFrame;
using sjpeg_internal::ResampleFrame;
using sjpeg_internal::ResampleStage;
using sjpeg_internal::kResampleHalf;
using sjpeg_internal::resample_clip;
using sjpeg_internal::resample_mac;

// how a row's segment is read
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
static_assert(sjpeg_internal::kResampleSegmentMax * 3 + 12 <= kStageBytes, "a segment of three channels fits the stage");

struct ResampleBoxArgs {
  const ResampleBoxFrame* frames;
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

// the sum of the nb bytes at g: whole dwords from the first byte on, the last 1..3 bytes one by one
__device__ __forceinline__ uint32_t sum_run(const uint8_t* g, unsigned nb) {
  const unsigned nd = nb >> 2;
  GlobalDwords const gd = (GlobalDwords)(g);
  uint32_t s = 0u;
  for (unsigned j = 0; j < nd; ++j) {
    const uint32_t v = gd[j];
    s += (v & 255u) + ((v >> 8) & 255u) + ((v >> 16) & 255u) + (v >> 24);
  }
  for (unsigned i = nd << 2; i < nb; ++i) s += ((GlobalBytes)(g))[i];
  return s;
}

// a byte of a run of packed pixels to the sum of its place in the pixel; c is that place and goes on to the next byte's
__device__ __forceinline__ void add_placed(uint32_t b, unsigned& c, unsigned step, uint32_t& p0, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
  p0 += c == 0u ? b : 0u;
  p1 += c == 1u ? b : 0u;
  p2 += c == 2u ? b : 0u;
  p3 += c == 3u ? b : 0u;
  c = c + 1u == step ? 0u : c + 1u;
}
// the nb bytes at g, a pixel's first byte, to the four sums by place: read as sum_run reads
__device__ __forceinline__ void sum_placed(const uint8_t* g, unsigned nb, unsigned step, uint32_t& p0, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
  const unsigned nd = nb >> 2;
  GlobalDwords const gd = (GlobalDwords)(g);
  unsigned c = 0u;
  for (unsigned j = 0; j < nd; ++j) {
    const uint32_t v = gd[j];
#pragma unroll
    for (int t = 0; t < 4; ++t) add_placed((v >> (8 * t)) & 255u, c, step, p0, p1, p2, p3);
  }
  for (unsigned i = nd << 2; i < nb; ++i) add_placed(((GlobalBytes)(g))[i], c, step, p0, p1, p2, p3);
}
__device__ __forceinline__ uint32_t placed(unsigned at, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
  return at == 0u ? p0 : at == 1u ? p1 : at == 2u ? p2 : p3;
}

// kCls: how the format's rows are read; kFlat: the frames are of an alpha format (four-byte pixels: the packed class;
// float RGBA: the element class) and are flattened before they are summed.  Compile-time, as in resample.hip.
template <int kCls, bool kFlat>
__global__ __launch_bounds__(256) void resample_box_kernel(const ResampleBoxArgs a) {
  static_assert(!(kFlat && kCls == kPlanes), "a format with alpha is packed pixels or float elements");
  __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
  __shared__ __attribute__((aligned(16))) uint8_t mid[kTileRows * kTilePitch];
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTileRows * kTilePitch];
  __shared__ int32_t wky[kTileRows * kTileRows];                   // a chunk's vertical coefficients, [tile row][chunk row]
  const unsigned wg = blockIdx.x, tid = threadIdx.x;
  int flo = 0, fhi = a.nframes - 1;
  while (flo < fhi) {                                              // (the LAST frame whose first tile is not behind wg)
    const int m = (flo + fhi + 1) >> 1;
    if (a.frames[m].r.tile_base <= wg) flo = m; else fhi = m - 1;
  }
  const ResampleFrame& d = a.frames[flo].r;                       // (read where it is used: a copy would live in SGPRs throughout)
  const ResampleStage& sg = a.frames[flo].s;
  const unsigned t = wg - d.tile_base, tyi = t / d.tiles_x, txi = t - tyi * d.tiles_x;
  const int ox0 = static_cast<int>(txi) * d.tw, oy0 = static_cast<int>(tyi) * kTileRows;
  if (oy0 >= d.h2) return;                                         // (a grid larger than the plan's: nothing of this frame)
  const int tw = min(d.tw, d.w2 - ox0), th = min(kTileRows, d.h2 - oy0);
  const int channels = a.channels, cols = tw * channels;
  GlobalInts const xb = (GlobalInts)(d.xb), xk = (GlobalInts)(d.xk), yb = (GlobalInts)(d.yb), yk = (GlobalInts)(d.yk);
  // the tile's segment of a row of the reduced picture and its rows: the windows' ends are in order (the plan checked)
  const int xs = xb[2 * ox0], xe = xb[2 * (ox0 + tw - 1)] + xb[2 * (ox0 + tw - 1) + 1];
  const int ys = yb[2 * oy0], ye = yb[2 * (oy0 + th - 1)] + yb[2 * (oy0 + th - 1) + 1];
  // the staged rows: a run of bytes per channel
  const unsigned seg = static_cast<unsigned>(xe - xs);
  const unsigned cpitch = align4(seg);
  const unsigned rpitch = cpitch * static_cast<unsigned>(channels);
  const int R = min(kTileRows, static_cast<int>(kStageBytes / rpitch));
  // who stages what: a wave a row, or the whole workgroup the one row of a chunk
  const unsigned slanes = R == 1 ? 256u : 64u, slane = tid & (slanes - 1u), srow = tid / slanes, srows = 256u / slanes;
  const int fx = sg.fx, fy = sg.fy, xend = sg.x0 + sg.w, yend = sg.y0 + sg.h;

  for (unsigned i = tid; i < kTileRows * kTilePitch / 4u; i += 256u) reinterpret_cast<uint32_t*>(tile)[i] = 0u;   // (the rows' padding)

  // horizontal pass: my column of the tile, my rows of a chunk
  const int G = 256 / cols;                                        // row groups: at least 2
  const int hcol = static_cast<int>(tid) % cols, rg = static_cast<int>(tid) / cols;
  const bool hactive = rg < G;
  const int hj = hcol / channels, hc = hcol - hj * channels;
  const int hxmin = xb[2 * (ox0 + hj)], hn = hactive ? xb[2 * (ox0 + hj) + 1] : 0;
  GlobalInts const hk = xk + static_cast<size_t>(ox0 + hj) * static_cast<size_t>(d.ksx);
  const uint8_t* const hp = stage + static_cast<unsigned>(hxmin - xs) + static_cast<unsigned>(hc) * cpitch;

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
      // row y0 + r of the reduced picture: the source rows sy0 .. sy0 + ny
      const int sy0 = sg.y0 + (y0 + static_cast<int>(r)) * fy, ny = min(fy, yend - sy0);
      uint8_t* const l = stage + r * rpitch;
      for (unsigned k = slane; k < seg; k += slanes) {
        // ... and its sample xs + k: of each of them the pixels sx0 .. sx0 + nx
        const int sx0 = sg.x0 + (xs + static_cast<int>(k)) * fx, nx = min(fx, xend - sx0);
        uint32_t S[3] = {0u, 0u, 0u};
        for (int yy = 0; yy < ny; ++yy) {
          const uint8_t* const row = d.src + static_cast<long long>(sy0 + yy) * d.row_stride;
          if constexpr (kFlat && kCls == kPacked) {
            // four-byte pixels, alpha the last byte: a dword a pixel
            GlobalDwords const gd = (GlobalDwords)(row + static_cast<long long>(sx0) * 4);
            for (int xx = 0; xx < nx; ++xx) {
              const uint32_t v = gd[xx], al = v >> 24;
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                S[c] += sjpeg_internal::flatten_byte(al, (v >> (static_cast<unsigned>(d.off[c]) * 8u)) & 255u, a.bg[c], a.premultiplied != 0);
              }
            }
          } else if constexpr (kCls == kPacked) {
            const unsigned step = static_cast<unsigned>(a.pix_step);
            uint32_t p0 = 0u, p1 = 0u, p2 = 0u, p3 = 0u;
            sum_placed(row + static_cast<long long>(sx0) * step, static_cast<unsigned>(nx) * step, step, p0, p1, p2, p3);
#pragma unroll
            for (int c = 0; c < 3; ++c) S[c] += placed(static_cast<unsigned>(d.off[c]), p0, p1, p2, p3);
          } else if constexpr (kCls == kPlanes) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              if (c < channels) S[c] += sum_run(row + d.off[c] + sx0, static_cast<unsigned>(nx));
            }
          } else {
            // the float formats, a pixel at a time: never an element that is not a used sample of a pixel of the picture
            for (int xx = 0; xx < nx; ++xx) {
              const uint8_t* const px = row + static_cast<long long>(sx0 + xx) * a.pix_step;
              uint32_t al = 0u;
              if constexpr (kFlat) al = static_cast<uint32_t>(sjpeg_internal::elem_load_u8(px + 3 * (a.pix_step >> 2), a.kind, a.ascale, a.abias));
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                if (c >= channels) continue;
                uint32_t b = static_cast<uint32_t>(sjpeg_internal::elem_load_u8(px + d.off[c], a.kind, a.pscale[c], a.pbias[c]));
                if constexpr (kFlat) b = sjpeg_internal::flatten_byte(al, b, a.bg[c], a.premultiplied != 0);
                S[c] += b;
              }
            }
          }
        }
        const uint32_t n = static_cast<uint32_t>(nx * ny), m = sg.m[(nx < fx ? 1 : 0) + (ny < fy ? 2 : 0)];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (c < channels) l[static_cast<unsigned>(c) * cpitch + k] = static_cast<uint8_t>(sjpeg_internal::resample_reduce_sample(S[c], n, m));
        }
      }
    }
    __syncthreads();
    {
      // the chunk's vertical coefficients: tile row wr's for row y0 + wy, one a thread (0 outside the window)
      const int y = y0 + wy;
      wky[tid] = y >= wmin && y < wend && wy < nr ? wk[y] : 0;
    }
    {
      int32_t acc[kRowsPerThread];
#pragma unroll
      for (int m = 0; m < kRowsPerThread; ++m) acc[m] = kResampleHalf;
      auto tap = [&](int32_t k, int x) {
        const uint8_t* const p = hp + static_cast<unsigned>(x);
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

int resample_box_launch(int format, const float* pscale, const float* pbias, const sjpeg_hip_flatten* flatten, const ResampleBoxFrame* d_frames,
                        int nframes, unsigned tiles, hipStream_t st) {
  const SourceLayout& L = *source_layout(format);
  ResampleBoxArgs a;
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
      hipLaunchKernelGGL((resample_box_kernel<kElems, true>), dim3(tiles), dim3(256), 0, st, a);
    } else {
      hipLaunchKernelGGL((resample_box_kernel<kPacked, true>), dim3(tiles), dim3(256), 0, st, a);
    }
  } else if (cls == kElems) {
    hipLaunchKernelGGL((resample_box_kernel<kElems, false>), dim3(tiles), dim3(256), 0, st, a);
  } else if (cls == kPlanes) {
    hipLaunchKernelGGL((resample_box_kernel<kPlanes, false>), dim3(tiles), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((resample_box_kernel<kPacked, false>), dim3(tiles), dim3(256), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace sjpeg_internal
