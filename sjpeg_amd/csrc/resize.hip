// resize.hip -- pictures of a ragged batch resized to any smaller size on gfx950: thumbnails that fit a box, in ONE
// launch in front of the ragged encodes (sjpeg_hip_resize_ragged_src, sjpeg_hip_encode_ragged_resized_src; sjpeg_hip.h).
//
// Reference: none -- the reference codes the picture it is given (src/enc.cc:391-448).  The contract is on the bytes:
// a sample of frame f's resized picture is the exact area average of the source bytes its cell covers, rounded half up
// (resize_math.h: integers only, one right answer); a source byte is what the encoder sees there today (pixel_elem.h for
// floats).
//
// Shape: a flat grid over the batch's tiles, a workgroup one tile of tw x th resized samples of one frame, found by a
// binary search over the frames' first tiles -- so the sizes, the format's fields and the element kind are
// wave-uniform.  The workgroup walks the source rows its tile covers from the top.  It STAGES the segment of several
// rows that the tile's columns span in LDS -- a wave a row, adjacent lanes adjacent dwords of it (bytes at a row's last
// 1..3 bytes, elements for the floats, which land there as bytes) --, then P = 256 / tw adjacent lanes share a column:
// lane p adds the weighted bytes of every P-th source column of the cell (adjacent lanes read adjacent staged pixels),
// a butterfly of shuffles makes the row's horizontal sum (32 bits: at most 255 W), and lane 0 of the column adds it,
// weighted, to the 64-bit sums of the resized row at hand -- a source row touches at most two.  A finished row is
// rounded into the tile's bytes in LDS; the tile leaves as whole dwords.  tw follows the ratio (P about W / w'), so a
// lane has about one source pixel a row at any ratio; a segment too long for the LDS is staged in chunks, a row at a
// time.  Neighbouring tiles share one source column and row.  No atomics.  DESIGN.md section 4.
//
// A frame with an EXIF orientation other than 1 (sjpeg_hip_orient_ragged_src; orient_math.h) differs in the store
// alone: its finished tile lands mirrored or transposed in the upright picture.  A tile's span of a destination row
// then starts at any byte and may meet its neighbour's inside a dword, so a workgroup stores the bytes of its own
// samples and no other byte, the rows' padding included: whole dwords inside the span, single bytes at its two ends.
//
// The YUV-plane formats (sjpeg_hip_resize_ragged_yuv_src; yuv_resize_plan.cc) run the kernel's second instantiation:
// the flat grid over the tiles of every PLANE of every frame, each plane resized and turned as a gray picture of its
// own.  The UV plane of NV12 / NV21 is a packed picture of two-byte pixels: staged once, summed as two channels, its
// finished tile stored as two planes.
//
// Contact sheets (sjpeg_hip_sheet_ragged_src; sheet_plan.cc): sheet_fill_kernel writes the sheets' background, then the
// kernel's PLACED instantiations store every thumbnail's tiles into its rectangle of a sheet plane.
//
// Alpha flattening (sjpeg_hip_flatten_ragged_src; flatten_math.h): the FLAT instantiations lay every pixel of a BGRA /
// RGBA / float RGBA frame over a background where the segment is staged -- a packed pixel in registers between the
// global load and the LDS store, a float pixel as its four elements become bytes --, so the staged bytes are those of
// the flattened picture and everything behind the stage is as it is for SJPEG_HIP_SRC_RGB.  The sums are over bytes
// b <= 255 as before: the 32-bit and 64-bit bounds above hold unchanged.
//
// Deep video (sjpeg_hip_convert_ragged_yuv16_src; sjpeg_hip.h, "10-bit video"): the DEEP instantiations of the YUV-plane
// kernel read planes of little-endian 16-bit samples -- P010 and its kin, yuv420p10le / 12le.  A row's segment is staged
// as the 16-bit elements it is, whole dwords and at most one trailing element, so the stage holds half as many samples:
// 8192 of a one-channel plane, 4096 pairs of a P010 UV plane, and the chunked path starts at half the width.  The sum
// loop reads uint16 from LDS: adjacent lanes still read adjacent samples, now two halves of one dword where four lanes
// read the four bytes of one, so the 32 lanes the LDS serves together span twice as many banks as with bytes -- at
// most 64 samples (P is the largest power of two in W / w', so 32 lanes' cells span less than 2 x 32 columns), 32
// dwords: each in a bank of its own, as before.  A row's sum is at most 65535 W < 2^32 and a cell's 65535 W H < 2^48:
// h stays 32 bits and acc 64.  A finished row is rounded ONCE, by resize_round_deep with the launch's shift, into the
// byte tile; from there on nothing differs.
//
// Linear light (sjpeg_hip_linear_ragged_src; light_math.h): the LINEAR instantiations of the RGB-like and gray kernel
// average the light the bytes stand for.  The table L[] lies in LDS, 512 bytes, copied once per workgroup.  A byte is
// converted WHERE THE SEGMENT IS STAGED -- behind the flatten, which stays on bytes -- so the stage holds 16-bit linear
// words, always as a run of words per channel whatever the source's layout (a packed pixel is taken apart on the way:
// three byte-pitched words would put 32 lanes' reads on 48 dwords, two to a bank for half of them; a run per channel
// puts them on 16).  The sum loop is then the deep one, sample for sample and bound for bound: a row's sum at most
// 65535 W < 2^32, a cell's 65535 W H < 2^48.  `cap`, for every staging class alike, is the 16 384 bytes over two
// bytes a sample and channel: 2728 pixels of three channels, 8192 of gray; the chunked path starts there.  A finished
// cell goes back to a byte by light_round, the exact inverse, on the lane that rounds today.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "flatten_math.h"
#include "light_math.h"
#include "orient_math.h"
#include "pixel_elem.h"
#include "ragged_aux.h"
#include "reduce_round.h"
#include "resize_math.h"
#include "sjpeg_hip.h"
#include "source_layout.h"

namespace {

using sjpeg_internal::ResizeFrame;
using sjpeg_internal::YuvPlane;
using sjpeg_internal::resize_count;
using sjpeg_internal::resize_first;
using sjpeg_internal::resize_weight;

// how a row's segment is staged
enum { kResizePacked = 0, kResizePlanes = 1, kResizeElems = 2 };

constexpr unsigned kStageBytes = 16384;          // staged source rows
constexpr int kTileRowsMax = 16;                 // th
constexpr unsigned kTileBytes = kTileRowsMax * (256 * 3 + 4);   // (a transposing frame's rows: one dword of pitch more)

struct ResizeArgs {
  const ResizeFrame* frames;
  int nframes;
  int cls;                       // kResize*
  int kind;                      // kElem* (pixel_elem.h)
  int pix_step;                  // bytes from a pixel to the next
  int channels;                  // 3, or 1 for the gray formats
  float pscale[3], pbias[3];     // the engine's pixel transform (float formats)
};

// The pictures lie in device memory (reduce.hip says why this is said); a source dword is aligned like a byte.
typedef uint32_t __attribute__((aligned(1))) Dword1;
typedef const __attribute__((address_space(1))) Dword1* GlobalDwords;
typedef const __attribute__((address_space(1))) uint8_t* GlobalBytes;
typedef const __attribute__((address_space(1))) uint16_t* GlobalWords;
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

// nw 16-bit samples of a source row at g (a multiple of 2) into LDS at l (a multiple of 4): whole dwords, then at most
// one trailing sample -- every byte read is one of the 2 nw, and no dword reaches past the last sample
__device__ __forceinline__ void stage_words(const uint8_t* g, uint8_t* l, unsigned nw, unsigned lane, unsigned lanes) {
  const unsigned nd = nw >> 1;
  GlobalDwords const gd = (GlobalDwords)(g);
  uint32_t* const ld = reinterpret_cast<uint32_t*>(l);
  for (unsigned i = lane; i < nd; i += lanes) ld[i] = gd[i];
  if ((nw & 1u) != 0u && lane == 0u) reinterpret_cast<uint16_t*>(l)[nw - 1u] = ((GlobalWords)(g))[nw - 1u];
}

// a staged sample: a byte, or (deep) a 16-bit word
template <bool kDeep>
__device__ __forceinline__ uint32_t staged_sample(const uint8_t* p) {
  if constexpr (kDeep) return *reinterpret_cast<const uint16_t*>(p);
  else return *p;
}

// The flat instantiations' arguments: the launch's flatten, wave-uniform like the rest
struct FlatResizeArgs : ResizeArgs {
  uint32_t bg[3];                // the background, R, G, B
  int premultiplied;
  float ascale, abias;           // the alpha sample's transform (float formats)
};

// npix four-byte pixels of a source row at g into LDS at l (a multiple of 4), flattened on the way: g is a pixel
// boundary, so every dword is one pixel -- alpha its last byte, R, G and B at the bytes sh[c] / 8 -- and there is no
// tail of single bytes: the count is of pixels.  The colour bytes are replaced, the alpha byte stays (nothing reads it).
__device__ __forceinline__ void stage_pixels_flat(const uint8_t* g, uint8_t* l, unsigned npix, unsigned lane, unsigned lanes,
                                                  const unsigned (&sh)[3], const FlatResizeArgs& a) {
  GlobalDwords const gd = (GlobalDwords)(g);
  uint32_t* const ld = reinterpret_cast<uint32_t*>(l);
  const bool pre = a.premultiplied != 0;
  for (unsigned i = lane; i < npix; i += lanes) {
    const uint32_t v = gd[i], al = v >> 24;
    uint32_t o = v & 0xff000000u;
#pragma unroll
    for (int c = 0; c < 3; ++c) o |= sjpeg_internal::flatten_byte(al, (v >> sh[c]) & 255u, a.bg[c], pre) << sh[c];
    ld[i] = o;
  }
}

// The YUV-plane formats (sjpeg_hip_resize_ragged_yuv_src): the grid runs over the tiles of every PLANE of every frame,
// and what is launch-wide above -- class, channels, pixel step -- is the plane's: Y, and U and V of the planar formats,
// one-channel planes; the UV plane of NV12 / NV21 a packed picture of two-byte pixels.
struct YuvResizeArgs {
  const YuvPlane* planes;
  int nplanes;
};
// ... and the deep instantiations': the launch's depth
struct YuvDeepResizeArgs : YuvResizeArgs {
  uint32_t shift;                // sjpeg_hip_yuv_depth: how many low bits of a word lie below the byte, 0..8
};
template <bool kYuv, bool kFlat = false, bool kDeep = false> struct ResizeArgsOf { typedef ResizeArgs type; };
template <> struct ResizeArgsOf<true, false, false> { typedef YuvResizeArgs type; };
template <> struct ResizeArgsOf<false, true, false> { typedef FlatResizeArgs type; };
template <> struct ResizeArgsOf<true, false, true> { typedef YuvDeepResizeArgs type; };
// a finished cell's sum rounded into its byte (ltab: the linear instantiations' table in LDS)
template <bool kDeep, bool kLinear, class Args>
__device__ __forceinline__ uint32_t round_sample(uint64_t S, uint32_t W, uint32_t H, const Args& a, const uint16_t* ltab) {
  if constexpr (kLinear) return sjpeg_internal::light_round(S, W, H, ltab);
  else if constexpr (kDeep) return sjpeg_internal::resize_round_deep(S, W, H, a.shift);
  else return sjpeg_internal::resize_round(S, W, H);
}

// nb bytes of one channel's run of a source row at g into the words at l (a multiple of 4), each through the table:
// whole dwords, the last 1..3 bytes one by one -- every byte read is one of the nb
__device__ __forceinline__ void stage_bytes_linear(const uint8_t* g, uint16_t* l, unsigned nb, unsigned lane, unsigned lanes,
                                                   const uint16_t* ltab) {
  const unsigned nd = nb >> 2;
  GlobalDwords const gd = (GlobalDwords)(g);
  uint32_t* const ld = reinterpret_cast<uint32_t*>(l);
  for (unsigned i = lane; i < nd; i += lanes) {
    const uint32_t v = gd[i];
    ld[2u * i] = ltab[v & 255u] | (static_cast<uint32_t>(ltab[(v >> 8) & 255u]) << 16);
    ld[2u * i + 1u] = ltab[(v >> 16) & 255u] | (static_cast<uint32_t>(ltab[v >> 24]) << 16);
  }
  const unsigned i = (nd << 2) + lane;
  if (i < nb) l[i] = ltab[((GlobalBytes)(g))[i]];
}

// npix three-byte pixels of a source row at g, taken apart into the three runs of words at l, l + wpitch and
// l + 2 wpitch (8-byte aligned each; channel c's byte lies o[c] = 0..2 bytes into a pixel).  Four pixels a lane: their
// 12 bytes as three dwords, and per channel the four words as ONE 8-byte store -- adjacent lanes adjacent 8 bytes of a
// run --; the last 1..3 pixels byte by byte.  Every byte read is one of the 3 npix.
__device__ __forceinline__ void stage_pixels3_linear(const uint8_t* g, uint16_t* l, unsigned wpitch, unsigned npix, unsigned lane,
                                                     unsigned lanes, unsigned o0, unsigned o1, const uint16_t* ltab) {
  const unsigned ng = npix >> 2, o2 = 3u - o0 - o1;
  GlobalDwords const gd = (GlobalDwords)(g);
  for (unsigned i = lane; i < ng; i += lanes) {
    const uint64_t lo = gd[3u * i] | (static_cast<uint64_t>(gd[3u * i + 1u]) << 32);
    const uint32_t hi = gd[3u * i + 2u];
    auto word = [&](unsigned j) -> uint32_t {                      // the light of byte j = 0..11 of the twelve
      return ltab[j < 8u ? static_cast<uint32_t>(lo >> (8u * j)) & 255u : (hi >> (8u * (j - 8u))) & 255u];
    };
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned o = c == 0 ? o0 : c == 1 ? o1 : o2;
      *reinterpret_cast<uint2*>(l + c * wpitch + 4u * i) =
          make_uint2(word(o) | (word(o + 3u) << 16), word(o + 6u) | (word(o + 9u) << 16));
    }
  }
  const unsigned k = (ng << 2) + lane;
  if (k < npix) {
    GlobalBytes const gb = (GlobalBytes)(g) + 3u * k;
    l[k] = ltab[gb[o0]];
    l[wpitch + k] = ltab[gb[o1]];
    l[2u * wpitch + k] = ltab[gb[o2]];
  }
}
__device__ __forceinline__ int desc_count(const ResizeArgs& a) { return a.nframes; }
__device__ __forceinline__ int desc_count(const YuvResizeArgs& a) { return a.nplanes; }
__device__ __forceinline__ const ResizeFrame& desc_at(const ResizeArgs& a, int i) { return a.frames[i]; }
__device__ __forceinline__ const ResizeFrame& desc_at(const YuvResizeArgs& a, int i) { return a.planes[i].r; }

// kYuv false: the RGB-like and gray formats, a descriptor a frame.  kYuv true: the YUV-plane formats, a descriptor a
// plane; what differs is decided at compile time, so either instantiation holds its own work alone.  A two-channel
// plane is staged ONCE, as the packed pixels it is, summed as two channels and rounded into a tile of pairs; the tile
// leaves as two planes, U to the descriptor's dst and V to its dst2, each by the turned store's rule.
// kPlaced: the descriptors are PLACED ones (ragged_aux.h: contact sheets) -- dst is the picture's first sample inside
// a larger plane, so every tile, an unturned frame's too, leaves by the exact-span store: the whole-dword store
// reaches into what is row padding in a picture of its own and is the next cell or the gutter in a sheet.  A
// compile-time flag: the unplaced instantiations hold what they held before there were sheets.
// kFlat: the frames are of an alpha format (BGRA / RGBA bytes: the packed class; float RGBA: the element class) and
// are flattened as they are staged.  A compile-time flag again, with arguments of its own: the four instantiations
// without it hold what they held before; there is no flat YUV instantiation.
// kDeep: the planes are of 16-bit samples (the YUV-plane formats alone).  A compile-time flag once more: what differs
// is the staged element (esz bytes), the sample the sum loop reads and the rounding; the six instantiations without it
// hold what they held before.
// kLinear: the average is of linear light (the RGB-like and gray formats alone, plain or flat).  A compile-time flag
// like the others: what differs is the table in LDS, the staged sample -- a 16-bit linear word in a run per channel --
// and the rounding; the eight instantiations without it hold what they held before.
template <bool kYuv, bool kPlaced, bool kFlat = false, bool kDeep = false, bool kLinear = false>
__global__ __launch_bounds__(256) void resize_ragged_kernel(const typename ResizeArgsOf<kYuv, kFlat, kDeep>::type a) {
  static_assert(!(kYuv && kFlat), "the YUV-plane formats have no alpha");
  static_assert(kYuv || !kDeep, "16-bit samples: the YUV-plane formats alone");
  static_assert(!(kYuv && kLinear), "linear light: the YUV-plane formats' samples are not RGB light");
  constexpr bool kWide = kDeep || kLinear;                         // the stage holds 16-bit words
  constexpr unsigned esz = kWide ? 2u : 1u;                        // bytes a staged sample
  __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTileBytes];
  __shared__ __attribute__((aligned(16))) uint16_t light[kLinear ? 256 : 1];
  const unsigned wg = blockIdx.x, tid = threadIdx.x;
  const uint16_t* ltab = nullptr;
  if constexpr (kLinear) {
    light[tid] = sjpeg_internal::kLightSrgb[tid];                  // (256 threads, 256 entries; the barrier is below)
    ltab = light;
  }
  int flo = 0, fhi = desc_count(a) - 1;
  while (flo < fhi) {
    const int mid = (flo + fhi + 1) >> 1;
    if (desc_at(a, mid).tile_base <= wg) flo = mid; else fhi = mid - 1;
  }
  const ResizeFrame d = desc_at(a, flo);
  const uint32_t W = d.W, H = d.H, w2 = d.w2, h2 = d.h2;
  const unsigned t = wg - d.tile_base, tyi = t / d.tiles_x, txi = t - tyi * d.tiles_x;
  const uint32_t ox0 = txi * d.tw, oy0 = tyi * d.th;
  const uint32_t tw = min(static_cast<uint32_t>(d.tw), w2 - ox0), th = min(static_cast<uint32_t>(d.th), h2 - oy0);
  const unsigned P = 256u / static_cast<unsigned>(d.tw);          // lanes a column: a power of two, 1..64
  const unsigned j = tid / P, p = tid & (P - 1u);
  const bool col = j < tw;
  unsigned channels;
  int cls, pix_step;
  if constexpr (kYuv) {
    channels = a.planes[flo].channels;
    cls = channels == 2u ? kResizePacked : kResizePlanes;
    pix_step = 2;
  } else {
    channels = a.channels;
    cls = a.cls;
    pix_step = a.pix_step;
  }
  // the channels past the first: all three of an RGB-like picture, U and V of a packed pair
  const bool three = !kYuv && channels == 3u, two = kYuv && channels == 2u;
  // my cell's source columns; the tile's segment of a source row and its source rows
  const uint32_t cx0 = col ? resize_first(ox0 + j, W, w2) : 0u, cx1 = col ? cx0 + resize_count(ox0 + j, W, w2) : 0u;
  const uint32_t xs = resize_first(ox0, W, w2), xe = resize_first(ox0 + tw - 1u, W, w2) + resize_count(ox0 + tw - 1u, W, w2);
  const uint32_t ys = resize_first(oy0, H, h2), ye = resize_first(oy0 + th - 1u, H, h2) + resize_count(oy0 + th - 1u, H, h2);
  // The staged rows: packed pixels as they lie in memory, else a run of bytes per channel; `cap` pixels fit, a longer
  // segment goes in chunks of a single row
  // (linear: a run of words per channel whatever the source's class)
  const bool packed = !kLinear && cls == kResizePacked;
  const unsigned lstep = (packed ? pix_step : 1u) * esz;
  const unsigned cap = packed ? kStageBytes / lstep : (kStageBytes / (channels * esz)) & ~3u;
  const unsigned seg = xe - xs, clen_max = min(seg, cap);
  // (linear: a run starts at a multiple of 8, for the 8-byte stores of four words; cap * 2 is one, so nothing grows)
  const unsigned cpitch = packed ? 0u : kLinear ? (clen_max * esz + 7u) & ~7u : align4(clen_max * esz);
  const unsigned rpitch = packed ? align4(clen_max * lstep) : cpitch * channels;
  const unsigned R = seg > cap ? 1u : kStageBytes / rpitch;
  unsigned coff[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) coff[c] = packed ? static_cast<unsigned>(d.off[c]) * esz : static_cast<unsigned>(c) * cpitch;
  // who stages what: a wave a row, or the whole workgroup the one row of a chunk
  const unsigned slanes = R == 1u ? 256u : 64u, slane = tid & (slanes - 1u), srow = tid / slanes, srows = 256u / slanes;

  // the tile's rows in LDS, whole dwords; a transposing frame reads a destination row down a column of them, so its
  // pitch is an odd number of dwords: the th <= 16 rows of a column lie in th different banks
  const int orient = static_cast<int>(kPlaced ? d.orient & ~sjpeg_internal::kResizePlaced : d.orient);
  const bool transposed = sjpeg_internal::orient_transposes(orient);
  const unsigned tpitch = align4(static_cast<unsigned>(d.tw) * channels) | (transposed ? 4u : 0u);
  for (unsigned i = tid; i < th * tpitch / 4u; i += 256u) reinterpret_cast<uint32_t*>(tile)[i] = 0u;   // (the rows' padding)
  if constexpr (kLinear) __syncthreads();                          // (the table is read while the first rows are staged)

  uint32_t h[3] = {0u, 0u, 0u};
  uint64_t acc[3] = {0ull, 0ull, 0ull};
  uint32_t yo = oy0;                                               // the resized row the sums belong to
  for (uint32_t yb = ys; yb < ye; yb += R) {
    const unsigned nr = min(R, ye - yb);
    for (uint32_t xc = xs; xc < xe; xc += cap) {
      const unsigned clen = min(cap, xe - xc);
      for (unsigned r = srow; r < nr; r += srows) {
        const uint8_t* const row = d.src + static_cast<long long>(yb + r) * d.row_stride;
        uint8_t* const l = stage + r * rpitch;
        if constexpr (kLinear) {
          // the same reads as below, class by class; every byte -- the flattened one of a flat frame -- through the
          // table into its channel's run of words
          uint16_t* const lw = reinterpret_cast<uint16_t*>(l);
          const unsigned wpitch = cpitch >> 1;
          if (cls == kResizePacked && pix_step == 4) {
            // (four-byte pixels: row + xc * 4 is a pixel boundary; alpha is the last byte)
            GlobalDwords const gd = (GlobalDwords)(row + static_cast<long long>(xc) * 4);
            const unsigned sh[3] = {static_cast<unsigned>(d.off[0]) * 8u, static_cast<unsigned>(d.off[1]) * 8u, static_cast<unsigned>(d.off[2]) * 8u};
            for (unsigned k = slane; k < clen; k += slanes) {
              const uint32_t v = gd[k];
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                uint32_t b = (v >> sh[c]) & 255u;
                if constexpr (kFlat) b = sjpeg_internal::flatten_byte(v >> 24, b, a.bg[c], a.premultiplied != 0);
                lw[c * wpitch + k] = ltab[b];
              }
            }
          } else if (cls == kResizePacked) {
            stage_pixels3_linear(row + static_cast<long long>(xc) * 3, lw, wpitch, clen, slane, slanes, static_cast<unsigned>(d.off[0]),
                                 static_cast<unsigned>(d.off[1]), ltab);
          } else if (cls == kResizePlanes) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              if (c < static_cast<int>(channels)) stage_bytes_linear(row + d.off[c] + xc, lw + c * wpitch, clen, slane, slanes, ltab);
            }
          } else {
            // the float formats, a pixel at a time: never an element that is not a used sample of a pixel of the picture
            for (unsigned k = slane; k < clen; k += slanes) {
              const uint8_t* const px = row + static_cast<long long>(xc + k) * a.pix_step;
              uint32_t al = 0u;
              if constexpr (kFlat) {
                al = static_cast<uint32_t>(sjpeg_internal::elem_load_u8(px + 3 * (a.pix_step >> 2), a.kind, a.ascale, a.abias));
              }
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                if (c >= static_cast<int>(channels)) continue;
                uint32_t b = static_cast<uint32_t>(sjpeg_internal::elem_load_u8(px + d.off[c], a.kind, a.pscale[c], a.pbias[c]));
                if constexpr (kFlat) b = sjpeg_internal::flatten_byte(al, b, a.bg[c], a.premultiplied != 0);
                lw[c * wpitch + k] = ltab[b];
              }
            }
          }
        } else if constexpr (kFlat) {
          if (packed) {
            // (four-byte pixels: row + xc * 4 is a pixel boundary and l a multiple of 4)
            const unsigned sh[3] = {coff[0] * 8u, coff[1] * 8u, coff[2] * 8u};
            stage_pixels_flat(row + static_cast<long long>(xc) * 4, l, clen, slane, slanes, sh, a);
          } else {
            // float RGBA, a pixel at a time: its four elements, the colours through the pixel transform as ever and the
            // alpha through the flatten's own, flattened into the three runs of bytes
            const long long esz = a.pix_step >> 2;
            const bool pre = a.premultiplied != 0;
            for (unsigned k = slane; k < clen; k += slanes) {
              const uint8_t* const px = row + static_cast<long long>(xc + k) * a.pix_step;
              const uint32_t al = static_cast<uint32_t>(sjpeg_internal::elem_load_u8(px + 3 * esz, a.kind, a.ascale, a.abias));
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                const uint32_t sc = static_cast<uint32_t>(sjpeg_internal::elem_load_u8(px + d.off[c], a.kind, a.pscale[c], a.pbias[c]));
                l[c * cpitch + k] = static_cast<uint8_t>(sjpeg_internal::flatten_byte(al, sc, a.bg[c], pre));
              }
            }
          }
        } else if (packed) {
          if constexpr (kDeep) {
            stage_words(row + static_cast<long long>(xc) * lstep, l, clen * 2u, slane, slanes);   // (a pair: one dword)
          } else {
            stage_bytes(row + static_cast<long long>(xc) * lstep, l, clen * lstep, slane, slanes);
          }
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            if (c >= static_cast<int>(channels)) continue;
            if (kYuv || cls == kResizePlanes) {
              if constexpr (kDeep) {
                stage_words(row + (d.off[c] + static_cast<long long>(xc)) * 2, l + c * cpitch, clen, slane, slanes);
              } else {
                stage_bytes(row + d.off[c] + xc, l + c * cpitch, clen, slane, slanes);
              }
              continue;
            }
            // the float formats element by element: never an element that is not a used sample of a pixel of the picture
            if constexpr (!kYuv) {
              for (unsigned k = slane; k < clen; k += slanes) {
                l[c * cpitch + k] = static_cast<uint8_t>(sjpeg_internal::elem_load_u8(
                    row + d.off[c] + static_cast<long long>(xc + k) * a.pix_step, a.kind, a.pscale[c], a.pbias[c]));
              }
            }
          }
        }
      }
      __syncthreads();
      const uint32_t lo = max(cx0, xc), hi = min(cx1, xc + clen);
      const bool first = xc == xs, last = xc + clen == xe;
      for (unsigned r = 0; r < nr; ++r) {
        if (first) { h[0] = 0u; h[1] = 0u; h[2] = 0u; }            // (several chunks: nr == 1, h goes from chunk to chunk)
        for (uint32_t x = lo + p; x < hi; x += P) {
          const uint32_t w = resize_weight(ox0 + j, x, W, w2);
          const uint8_t* const px = stage + r * rpitch + (x - xc) * lstep;
          h[0] += w * staged_sample<kWide>(px + coff[0]);
          if (three) { h[1] += w * staged_sample<kWide>(px + coff[1]); h[2] += w * staged_sample<kWide>(px + coff[2]); }
          if (two) h[1] += w * staged_sample<kWide>(px + coff[1]);
        }
        if (!last) continue;
        for (unsigned m = P >> 1; m != 0u; m >>= 1) {
          h[0] += __shfl_xor(h[0], m);
          if (three) { h[1] += __shfl_xor(h[1], m); h[2] += __shfl_xor(h[2], m); }
          if (two) h[1] += __shfl_xor(h[1], m);
        }
        if (col && p == 0u) {
          // source row y into the resized row at hand; the row that ends it may begin the next
          const uint32_t y = yb + r;
          const uint32_t wy = resize_weight(yo, y, H, h2);
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c] += static_cast<uint64_t>(wy) * h[c];
          if ((y + 1u) * h2 >= (yo + 1u) * H) {
            uint8_t* const o = tile + (yo - oy0) * tpitch + j * channels;
            o[0] = static_cast<uint8_t>(round_sample<kDeep, kLinear>(acc[0], W, H, a, ltab));
            if (three) {
              o[1] = static_cast<uint8_t>(round_sample<kDeep, kLinear>(acc[1], W, H, a, ltab));
              o[2] = static_cast<uint8_t>(round_sample<kDeep, kLinear>(acc[2], W, H, a, ltab));
            }
            if (two) o[1] = static_cast<uint8_t>(round_sample<kDeep, kLinear>(acc[1], W, H, a, ltab));
            ++yo;
            const uint32_t wn = yo < oy0 + th ? resize_weight(yo, y, H, h2) : 0u;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = static_cast<uint64_t>(wn) * h[c];
          }
        }
      }
      __syncthreads();
    }
  }
  // the tile as whole dwords of the resized rows: its first byte is a multiple of 4 (tw is), its last dword may reach
  // into the row's padding, never past it
  if (!kPlaced && orient <= 1 && !two) {
    const unsigned ndw = (tw * channels + 3u) >> 2;
    for (unsigned i = tid; i < th * ndw; i += 256u) {
      const unsigned r = i / ndw, k = i - r * ndw;
      uint8_t* const out = d.dst + static_cast<size_t>(oy0 + r) * d.dst_stride + static_cast<size_t>(ox0) * channels;
      ((GlobalOut)(out))[k] = reinterpret_cast<const uint32_t*>(tile + r * tpitch)[k];
    }
    return;
  }
  // A turned frame: the tile is a rectangle of the upright picture too -- nrows rows of nsamp samples from (ux0, uy0),
  // the lower of its two opposite corners' places there.  Adjacent lanes store adjacent bytes or dwords of a destination
  // row and read them along a row of the tile (mirrored or not) or down a column of it; every byte stored is a sample's
  // of this tile.
  uint32_t ax, ay, bx, by;
  sjpeg_internal::orient_upright(ox0, oy0, w2, h2, orient, &ax, &ay);
  sjpeg_internal::orient_upright(ox0 + tw - 1u, oy0 + th - 1u, w2, h2, orient, &bx, &by);
  const uint32_t ux0 = min(ax, bx), uy0 = min(ay, by);
  const bool flipx = ax > bx, flipy = ay > by;
  // (a packed pair's tile leaves as two planes of one-byte samples: `och` bytes a sample where it lands, channel c0 of
  // the tile's `channels` first; else the sample's bytes as they lie in the tile)
  const unsigned och = kYuv ? 1u : channels;
  const unsigned nsamp = transposed ? th : tw, nrows = transposed ? tw : th, span = nsamp * och;
  // Dwords inside the span, bytes at its two ends.  The pictures start at multiples of 16 and their rows are whole
  // dwords apart, so the span's phase is the same in every row: `head` bytes up to the first dword boundary, nd whole
  // dwords -- every byte of them a sample of this tile --, `tail` bytes behind them.  A placed picture starts at any
  // byte of its sheet plane, so its phase is taken from the address the span starts at, the low two bits of
  // dst + ux0 * och; the sheet planes start at multiples of 16 and their rows are whole dwords apart, so the phase is
  // still the same in every row of a tile -- and the same for dst2: V's sheet plane is laid out as U's, 16 bytes a step.
  const unsigned lead = kPlaced ? static_cast<unsigned>(reinterpret_cast<uintptr_t>(d.dst)) & 3u : 0u;
  const unsigned head = min((4u - ((lead + ux0 * och) & 3u)) & 3u, span), nd = (span - head) >> 2, tail = (span - head) & 3u;
  const unsigned units = head + nd + tail;
  for (unsigned c0 = 0; c0 < (kYuv ? channels : 1u); ++c0) {
    // byte k of the tile's span of its destination row q
    auto span_byte = [&](unsigned q, unsigned k) -> uint32_t {
      const unsigned s = och == 3u ? k / 3u : k, c = k - s * och;
      const unsigned along = flipx ? nsamp - 1u - s : s, across = flipy ? nrows - 1u - q : q;
      const unsigned r = transposed ? along : across, jj = transposed ? across : along;
      return tile[r * tpitch + jj * channels + (kYuv ? c0 : c)];
    };
    uint8_t* dst = d.dst;
    if constexpr (kYuv) {
      if (c0 != 0u) dst = a.planes[flo].dst2;
    }
    for (unsigned i = tid; i < nrows * units; i += 256u) {
      const unsigned q = i / units, u = i - q * units;
      uint8_t* const out = dst + static_cast<size_t>(uy0 + q) * d.dst_stride + static_cast<size_t>(ux0) * och;
      if (u >= head && u < head + nd) {
        const unsigned k = head + ((u - head) << 2);
        *((GlobalOut)(out + k)) = span_byte(q, k) | (span_byte(q, k + 1u) << 8) | (span_byte(q, k + 2u) << 16) | (span_byte(q, k + 3u) << 24);
      } else {
        const unsigned k = u < head ? u : head + (nd << 2) + (u - head - nd);
        ((GlobalOutBytes)(out))[k] = static_cast<uint8_t>(span_byte(q, k));
      }
    }
  }
}

// The background of a call's sheets (sjpeg_hip_sheet_ragged_src), launched on the call's stream in front of the placed
// resize: every sample of every sheet plane in whole dwords, row padding included -- a plane's rows are whole dwords
// apart, so its rows * row_dwords dwords lie back to back from its start, a multiple of 16, and end inside the plane.
// Dword k of a row is pattern[k % 3]: an RGB row is a 12-byte pattern whose phase restarts at each row.  A grid-stride
// loop over the dwords of all sheets; adjacent lanes store adjacent dwords.
struct SheetFillArgs {
  uint8_t* base;
  unsigned long long sheet_bytes, per_sheet, total;    // from a sheet to the next; dwords a sheet, and of all sheets
  unsigned long long first[3], off[3];                 // plane c: its first dword among the sheet's, its place in the sheet
  unsigned row_dwords[3];
  uint32_t pattern[3][3];
  int nplanes;
};

__global__ __launch_bounds__(256) void sheet_fill_kernel(const SheetFillArgs a) {
  for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < a.total; i += gridDim.x * 256ull) {
    const unsigned long long s = i / a.per_sheet;
    unsigned long long r = i - s * a.per_sheet;
    const int c = a.nplanes == 3 ? (r >= a.first[2] ? 2 : r >= a.first[1] ? 1 : 0) : 0;
    r -= c == 2 ? a.first[2] : c == 1 ? a.first[1] : 0ull;
    const unsigned rd = c == 2 ? a.row_dwords[2] : c == 1 ? a.row_dwords[1] : a.row_dwords[0];
    const unsigned k = static_cast<unsigned>(r % rd) % 3u;
    const uint32_t p0 = c == 2 ? a.pattern[2][0] : c == 1 ? a.pattern[1][0] : a.pattern[0][0];
    const uint32_t p1 = c == 2 ? a.pattern[2][1] : c == 1 ? a.pattern[1][1] : a.pattern[0][1];
    const uint32_t p2 = c == 2 ? a.pattern[2][2] : c == 1 ? a.pattern[1][2] : a.pattern[0][2];
    uint8_t* const plane = a.base + s * a.sheet_bytes + (c == 2 ? a.off[2] : c == 1 ? a.off[1] : a.off[0]);
    ((GlobalOut)(plane))[r] = k == 2u ? p2 : k == 1u ? p1 : p0;
  }
}

}  // namespace

namespace sjpeg_internal {

static int resize_launch(bool placed, int format, const float* pscale, const float* pbias, const ResizeFrame* d_frames, int nframes,
                         unsigned tiles, hipStream_t st) {
  const SourceLayout& L = *source_layout(format);
  ResizeArgs a;
  memset(&a, 0, sizeof(a));
  a.frames = d_frames;
  a.nframes = nframes;
  a.kind = L.kind;
  a.channels = L.rgb_like ? 3 : 1;
  a.pix_step = L.plane[0].step * L.esz;
  a.cls = L.kind != kElemU8 ? kResizeElems : (L.one_pitch || a.channels == 1) ? kResizePlanes : kResizePacked;
  for (int c = 0; c < 3; ++c) { a.pscale[c] = pscale[c]; a.pbias[c] = pbias[c]; }
  if (placed) {
    hipLaunchKernelGGL((resize_ragged_kernel<false, true>), dim3(tiles), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((resize_ragged_kernel<false, false>), dim3(tiles), dim3(256), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int resize_ragged_flat_launch(bool placed, int format, const float* pscale, const float* pbias, const sjpeg_hip_flatten& flatten,
                              const ResizeFrame* d_frames, int nframes, unsigned tiles, hipStream_t st) {
  const SourceLayout& L = *source_layout(format);
  FlatResizeArgs a;
  memset(&a, 0, sizeof(a));
  a.frames = d_frames;
  a.nframes = nframes;
  a.kind = L.kind;
  a.channels = 3;
  a.pix_step = L.plane[0].step * L.esz;                            // (four bytes or four elements: resize_plan checked it)
  a.cls = L.kind != kElemU8 ? kResizeElems : kResizePacked;
  for (int c = 0; c < 3; ++c) { a.pscale[c] = pscale[c]; a.pbias[c] = pbias[c]; a.bg[c] = flatten.background[c]; }
  a.premultiplied = flatten.premultiplied;
  a.ascale = flatten.alpha_scale;
  a.abias = flatten.alpha_bias;
  if (placed) {
    hipLaunchKernelGGL((resize_ragged_kernel<false, true, true>), dim3(tiles), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((resize_ragged_kernel<false, false, true>), dim3(tiles), dim3(256), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the linear instantiations (sjpeg_hip_linear_ragged_src): the arguments of the plain launch, or of the flat one
int resize_ragged_linear_launch(bool placed, int format, const float* pscale, const float* pbias, const sjpeg_hip_flatten* flatten,
                                const ResizeFrame* d_frames, int nframes, unsigned tiles, hipStream_t st) {
  const SourceLayout& L = *source_layout(format);
  FlatResizeArgs a;
  memset(&a, 0, sizeof(a));
  a.frames = d_frames;
  a.nframes = nframes;
  a.kind = L.kind;
  a.channels = L.rgb_like ? 3 : 1;
  a.pix_step = L.plane[0].step * L.esz;
  a.cls = L.kind != kElemU8 ? kResizeElems : (L.one_pitch || a.channels == 1) ? kResizePlanes : kResizePacked;
  for (int c = 0; c < 3; ++c) { a.pscale[c] = pscale[c]; a.pbias[c] = pbias[c]; }
  if (flatten != nullptr) {
    for (int c = 0; c < 3; ++c) a.bg[c] = flatten->background[c];
    a.premultiplied = flatten->premultiplied;
    a.ascale = flatten->alpha_scale;
    a.abias = flatten->alpha_bias;
    if (placed) {
      hipLaunchKernelGGL((resize_ragged_kernel<false, true, true, false, true>), dim3(tiles), dim3(256), 0, st, a);
    } else {
      hipLaunchKernelGGL((resize_ragged_kernel<false, false, true, false, true>), dim3(tiles), dim3(256), 0, st, a);
    }
  } else {
    const ResizeArgs& plain = a;
    if (placed) {
      hipLaunchKernelGGL((resize_ragged_kernel<false, true, false, false, true>), dim3(tiles), dim3(256), 0, st, plain);
    } else {
      hipLaunchKernelGGL((resize_ragged_kernel<false, false, false, false, true>), dim3(tiles), dim3(256), 0, st, plain);
    }
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int resize_ragged_launch(int format, const float* pscale, const float* pbias, const ResizeFrame* d_frames, int nframes, unsigned tiles,
                         hipStream_t st) {
  return resize_launch(false, format, pscale, pbias, d_frames, nframes, tiles, st);
}
int resize_ragged_placed_launch(int format, const float* pscale, const float* pbias, const ResizeFrame* d_frames, int nframes, unsigned tiles,
                                hipStream_t st) {
  return resize_launch(true, format, pscale, pbias, d_frames, nframes, tiles, st);
}

int yuv_resize_ragged_launch(const YuvPlane* d_planes, int nplanes, unsigned tiles, hipStream_t st) {
  YuvResizeArgs a;
  a.planes = d_planes;
  a.nplanes = nplanes;
  hipLaunchKernelGGL((resize_ragged_kernel<true, false>), dim3(tiles), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int yuv_resize_ragged_placed_launch(const YuvPlane* d_planes, int nplanes, unsigned tiles, hipStream_t st) {
  YuvResizeArgs a;
  a.planes = d_planes;
  a.nplanes = nplanes;
  hipLaunchKernelGGL((resize_ragged_kernel<true, true>), dim3(tiles), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the deep instantiations (16-bit samples, sjpeg_hip_yuv_depth's shift launch-wide), unplaced or placed
int yuv_resize_ragged_deep_launch(bool placed, unsigned shift, const YuvPlane* d_planes, int nplanes, unsigned tiles, hipStream_t st) {
  YuvDeepResizeArgs a;
  a.planes = d_planes;
  a.nplanes = nplanes;
  a.shift = shift;
  if (placed) {
    hipLaunchKernelGGL((resize_ragged_kernel<true, true, false, true>), dim3(tiles), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((resize_ragged_kernel<true, false, false, true>), dim3(tiles), dim3(256), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int sheet_fill_launch(const SheetFill& fill, uint8_t* base, hipStream_t st) {
  SheetFillArgs a;
  a.base = base;
  a.sheet_bytes = fill.sheet_bytes;
  a.nplanes = fill.nplanes;
  unsigned long long at = 0;
  for (int c = 0; c < 3; ++c) {
    a.first[c] = at;
    a.off[c] = fill.off[c];
    a.row_dwords[c] = c < fill.nplanes ? fill.row_dwords[c] : 1u;
    for (int k = 0; k < 3; ++k) a.pattern[c][k] = fill.pattern[c][k];
    if (c < fill.nplanes) at += static_cast<unsigned long long>(fill.rows[c]) * fill.row_dwords[c];
  }
  a.per_sheet = at;
  a.total = at * static_cast<unsigned long long>(fill.nsheets);
  const unsigned long long blocks = (a.total + 255ull) / 256ull;
  hipLaunchKernelGGL(sheet_fill_kernel, dim3(static_cast<unsigned>(blocks < (1ull << 20) ? blocks : (1ull << 20))), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace sjpeg_internal
