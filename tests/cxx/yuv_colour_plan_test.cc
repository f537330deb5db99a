// The host half of the video colour conversion (sjpeg_amd/csrc/yuv_colour_plan.cc) alone, under AddressSanitizer and
// UndefinedBehaviorSanitizer: tests/test_yuv_colour_cxx.py builds this file with it and the three plan files by the host
// compiler.  Every array handed over lies in a heap buffer of exactly its size.  For batches of all four formats, odd
// sizes, every orientation and a colour per frame -- and the same batches placed into sheets -- the descriptors are
// held to the planes they describe; then the kernel's rule of what a lane touches (yuv_colour.hip, restated here) is
// walked over a heap buffer of exactly the bytes the planes take: every touched byte lies inside it, every sample of a
// converting frame is touched by exactly one lane, no sample of an identity frame and no byte outside a placed
// rectangle is touched, and what else is touched is row padding.  Bad colours come back as SJPEG_HIP_EINVAL.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../sjpeg_amd/csrc/ragged_aux.h"
#include "sjpeg_hip.h"

static std::string g_error;
namespace sjpeg_internal {
int set_error(int code, const std::string& msg) { g_error = msg; return code; }
}  // namespace sjpeg_internal

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #c, g_error.c_str()); return 1; } } while (0)

using sjpeg_internal::YuvColourFrame;
using sjpeg_internal::YuvColourPlan;

// marks[b]: 0 untouched, else how many lanes touched byte b
struct Marks {
  std::unique_ptr<uint8_t[]> m;
  size_t bytes;
  bool ok = true;
  void touch(size_t at, size_t n) {
    for (size_t i = 0; i < n; ++i) {
      if (at + i >= bytes) { ok = false; return; }
      ++m[at + i];
    }
  }
};

// the four bytes of a row from sample p on, by the kernel's rule (row: the row's offset in the buffer)
static void touch4(Marks* mk, bool placed, size_t row, int p, int n, unsigned stride) {
  if (!placed) {
    if (static_cast<unsigned>(p) < stride) mk->touch(row + p, 4);
    return;
  }
  if (p >= 0 && p + 4 <= n && ((row + p) & 3u) == 0) { mk->touch(row + p, 4); return; }
  for (int b = 0; b < 4; ++b) if (p + b >= 0 && p + b < n) mk->touch(row + p + b, 1);
}

static int walk(const YuvColourPlan& plan, Marks* mk) {
  for (size_t f = 0; f < plan.frames.size(); ++f) {
    const YuvColourFrame& d = plan.frames[f];
    const unsigned next = f + 1 < plan.frames.size() ? plan.frames[f + 1].tile_base : plan.tiles;
    const unsigned long long lanes = static_cast<unsigned long long>(d.groups) * d.ch;
    if (next == d.tile_base) continue;                           // identity: no tiles
    CHECK((lanes + 255) / 256 == next - d.tile_base);
    for (unsigned long long lane = 0; lane < static_cast<unsigned long long>(next - d.tile_base) * 256; ++lane) {
      const unsigned j = static_cast<unsigned>(lane / d.groups), g = static_cast<unsigned>(lane % d.groups);
      if (j >= static_cast<unsigned>(d.ch)) continue;
      const int p = 4 * static_cast<int>(g) - (plan.placed ? d.lead : 0);
      touch4(mk, plan.placed, reinterpret_cast<uintptr_t>(d.u) + static_cast<size_t>(j) * d.c_stride, p, d.cw, d.c_stride);
      touch4(mk, plan.placed, reinterpret_cast<uintptr_t>(d.v) + static_cast<size_t>(j) * d.c_stride, p, d.cw, d.c_stride);
      for (int r = 0; r < d.s; ++r) {
        const unsigned row = d.s * j + r;
        if (row >= static_cast<unsigned>(d.uh)) continue;
        for (int k = 0; k < d.s; ++k) {
          touch4(mk, plan.placed, reinterpret_cast<uintptr_t>(d.y) + static_cast<size_t>(row) * d.y_stride, d.s * p + 4 * k, d.uw, d.y_stride);
        }
      }
    }
    CHECK(mk->ok);
  }
  return 0;
}

// every sample of plane (at, w x h, stride) has mark `want`; counted off so that what is left can be looked at
static int settle(Marks* mk, size_t at, int w, int h, unsigned stride, int want) {
  for (int y = 0; y < h; ++y) {
    for (int x = 0; x < w; ++x) {
      uint8_t& m = mk->m[at + static_cast<size_t>(y) * stride + x];
      if (m != want) { printf("sample (%d, %d) of a %dx%d plane touched %d times, not %d\n", x, y, w, h, m, want); return 1; }
      m = 0;
    }
  }
  return 0;
}

static int chroma_dim(int format, int v) { return format == SJPEG_HIP_SRC_YUV444 ? v : (v + 1) / 2; }

static int one_batch(int format, int nframes, bool sheet, uint32_t* seed, long* plans) {
  auto next = [&]() { *seed = *seed * 1664525u + 1013904223u; return *seed >> 8; };
  const int nplanes = format == SJPEG_HIP_SRC_NV12 || format == SJPEG_HIP_SRC_NV21 ? 2 : 3;
  const bool half = format != SJPEG_HIP_SRC_YUV444;
  std::unique_ptr<sjpeg_hip_ragged_frame[]> frames(new sjpeg_hip_ragged_frame[nframes]);
  std::unique_ptr<int32_t[][2]> sizes(new int32_t[nframes][2]);
  std::unique_ptr<uint8_t[]> orients(new uint8_t[nframes]);
  std::unique_ptr<sjpeg_hip_yuv_colour[]> colours(new sjpeg_hip_yuv_colour[nframes]);
  std::unique_ptr<sjpeg_hip_sheet> sh(new sjpeg_hip_sheet);
  memset(sh.get(), 0, sizeof(*sh));
  sh->cols = 3; sh->rows = 2;
  sh->cell_width = half ? 38 : 37; sh->cell_height = half ? 26 : 23;
  sh->gutter = half ? 2 : 1; sh->margin = half ? 6 : 3;
  for (int f = 0; f < nframes; ++f) {
    memset(&frames[f], 0, sizeof(frames[f]));
    frames[f].width = 1 + static_cast<int>(next() % 90);
    frames[f].height = 1 + static_cast<int>(next() % 60);
    for (int i = 0; i < nplanes; ++i) {
      frames[f].plane[i] = reinterpret_cast<void*>(static_cast<uintptr_t>(0x10000000u + 0x1000000u * i));
      frames[f].row_stride[i] = 1 << 12;
    }
    orients[f] = static_cast<uint8_t>(1 + next() % 8);
    // (sizes are in the stored orientation; a sheet's thumbnail must fit its cell upright)
    const int bw = sheet ? (orients[f] >= 5 ? 23 : 37) : 90, bh = sheet ? (orients[f] >= 5 ? 37 : 23) : 60;
    const int mw = frames[f].width < bw ? frames[f].width : bw, mh = frames[f].height < bh ? frames[f].height : bh;
    sizes[f][0] = next() % 4 == 0 ? mw : 1 + static_cast<int>(next() % mw);
    sizes[f][1] = next() % 4 == 0 ? mh : 1 + static_cast<int>(next() % mh);
    memset(&colours[f], 0, sizeof(colours[f]));
    colours[f].matrix = next() % 2;
    colours[f].range = next() % 2;
  }
  for (int variant = 0; variant < 3; ++variant) {               // a colour per frame, one for all, none
    const sjpeg_hip_yuv_colour* col = variant == 2 ? nullptr : colours.get();
    const int per_frame = variant == 0;
    sjpeg_internal::YuvResizePlan own;
    sjpeg_internal::SheetPlan placed;
    if (sheet) {
      CHECK(sjpeg_internal::sheet_plan("test", format, nframes, frames.get(), sh.get(), sizes.get(), orients.get(), &placed) == 0);
      CHECK(placed.yuv);
    } else {
      CHECK(sjpeg_internal::yuv_resize_plan("test", format, nframes, frames.get(), sizes.get(), orients.get(), &own) == 0);
    }
    const sjpeg_internal::YuvResizePlan& planes = sheet ? placed.planes : own;
    const size_t bytes = sheet ? placed.bytes : own.bytes;
    YuvColourPlan plan;
    CHECK(sjpeg_internal::yuv_colour_plan("test", planes, col, per_frame, &plan) == 0);
    ++*plans;
    CHECK(plan.frames.size() == static_cast<size_t>(nframes) && plan.placed == sheet);
    CHECK(sjpeg_internal::yuv_colour_all_identity(nframes, col, per_frame) == (plan.tiles == 0));
    Marks mk;
    mk.bytes = bytes;
    mk.m.reset(new uint8_t[bytes]);
    memset(mk.m.get(), 0, bytes);
    if (walk(plan, &mk) != 0) return 1;
    unsigned tiles = 0;
    std::unique_ptr<sjpeg_hip_ragged_frame[]> out(new sjpeg_hip_ragged_frame[nframes]);
    uint8_t* const base = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(0x40000000u));
    if (!sheet) sjpeg_internal::yuv_resize_plan_frames(own, frames.get(), base, out.get());
    for (int f = 0; f < nframes; ++f) {
      const YuvColourFrame& d = plan.frames[f];
      const int o = orients[f];
      const int w2 = sizes[f][0], h2 = sizes[f][1], c2w = chroma_dim(format, w2), c2h = chroma_dim(format, h2);
      CHECK(d.uw == (o >= 5 ? h2 : w2) && d.uh == (o >= 5 ? w2 : h2));
      CHECK(d.cw == (o >= 5 ? c2h : c2w) && d.ch == (o >= 5 ? c2w : c2h));
      CHECK(d.cw == chroma_dim(format, d.uw) && d.ch == chroma_dim(format, d.uh));      // the size the upright luma's implies
      CHECK(d.s == (half ? 2 : 1));
      const sjpeg_hip_yuv_colour c = col == nullptr ? sjpeg_hip_yuv_colour{0, 0, {0, 0}} : col[per_frame ? f : 0];
      const sjpeg_internal::YuvColourTable t = sjpeg_internal::yuv_colour_table(c.matrix, c.range);
      CHECK(memcmp(&d.table, &t, sizeof(t)) == 0);
      const bool ident = c.matrix == 0 && c.range == 0;
      CHECK(d.tile_base == tiles);
      if (!ident) tiles += (d.groups * static_cast<unsigned>(d.ch) + 255u) / 256u;
      const size_t yat = reinterpret_cast<uintptr_t>(d.y), uat = reinterpret_cast<uintptr_t>(d.u), vat = reinterpret_cast<uintptr_t>(d.v);
      if (sheet) {
        const sjpeg_internal::SheetPlace& pl = placed.places[f];
        const size_t sheet_at = static_cast<size_t>(pl.sheet) * placed.fill.sheet_bytes;
        const int cx = half ? pl.x0 / 2 : pl.x0, cy = half ? pl.y0 / 2 : pl.y0;
        CHECK(d.y_stride == placed.fill.row_dwords[0] * 4 && d.c_stride == placed.fill.row_dwords[1] * 4);
        CHECK(yat == sheet_at + placed.fill.off[0] + static_cast<size_t>(pl.y0) * d.y_stride + pl.x0);
        CHECK(uat == sheet_at + placed.fill.off[1] + static_cast<size_t>(cy) * d.c_stride + cx);
        CHECK(vat == sheet_at + placed.fill.off[2] + static_cast<size_t>(cy) * d.c_stride + cx);
        CHECK(d.lead == (cx & 3) && d.groups == static_cast<unsigned>(d.lead + d.cw + 3) / 4u);
      } else {
        CHECK(base + yat == out[f].plane[0] && base + uat == out[f].plane[1] && base + vat == out[f].plane[2]);
        CHECK(d.y_stride == static_cast<unsigned>(out[f].row_stride[0]) && d.c_stride == static_cast<unsigned>(out[f].row_stride[1]));
        CHECK(yat % 16 == 0 && uat % 16 == 0 && vat % 16 == 0 && d.y_stride % 4 == 0 && d.c_stride % 4 == 0);
        CHECK(d.lead == 0 && d.groups == static_cast<unsigned>(d.cw + 3) / 4u);
      }
      // every sample once, or not at all
      if (settle(&mk, yat, d.uw, d.uh, d.y_stride, ident ? 0 : 1) != 0 || settle(&mk, uat, d.cw, d.ch, d.c_stride, ident ? 0 : 1) != 0 ||
          settle(&mk, vat, d.cw, d.ch, d.c_stride, ident ? 0 : 1) != 0) {
        printf("FAILED: format %d frame %d of %d, %dx%d upright, orientation %d, %s\n", format, f, nframes, d.uw, d.uh, o, sheet ? "placed" : "own");
        return 1;
      }
      if (!sheet) {
        // what is left of the frame's planes is row padding: in a row of the plane, behind its samples
        const size_t at[3] = {yat, uat, vat};
        for (int c = 0; c < 3; ++c) {
          const int w = c == 0 ? d.uw : d.cw, h = c == 0 ? d.uh : d.ch;
          const unsigned stride = c == 0 ? d.y_stride : d.c_stride;
          for (int y = 0; y < h; ++y) for (unsigned x = w; x < stride; ++x) mk.m[at[c] + static_cast<size_t>(y) * stride + x] = 0;
        }
      }
    }
    CHECK(tiles == plan.tiles);
    for (size_t b = 0; b < bytes; ++b) {
      if (mk.m[b] != 0) { printf("FAILED: byte %zu of %zu, no sample and no row padding of a frame's, was touched (%s)\n", b, bytes, sheet ? "placed" : "own"); return 1; }
    }
  }
  return 0;
}

static int refusals() {
  std::unique_ptr<sjpeg_hip_ragged_frame[]> frames(new sjpeg_hip_ragged_frame[2]);
  std::unique_ptr<sjpeg_hip_yuv_colour[]> colours(new sjpeg_hip_yuv_colour[2]);
  for (int f = 0; f < 2; ++f) {
    memset(&frames[f], 0, sizeof(frames[f]));
    frames[f].width = 16; frames[f].height = 8;
    memset(&colours[f], 0, sizeof(colours[f]));
  }
  sjpeg_internal::YuvResizePlan planes;
  CHECK(sjpeg_internal::yuv_resize_plan("t", SJPEG_HIP_SRC_NV12, 2, frames.get(), nullptr, nullptr, &planes) == 0);
  YuvColourPlan plan;
  colours[1].matrix = 2;
  CHECK(sjpeg_internal::yuv_colour_plan("t", planes, colours.get(), 1, &plan) == SJPEG_HIP_EINVAL);
  CHECK(g_error == "t: frame 1: colour: matrix 2 is not one of 0..1 (SJPEG_HIP_MATRIX_BT601, _BT709)");
  CHECK(plan.frames.empty() && plan.tiles == 0);                  // a refused batch leaves no plan
  CHECK(sjpeg_internal::yuv_colour_plan("t", planes, colours.get(), 0, &plan) == 0 && plan.tiles == 0);       // ([0] alone is read)
  colours[1].matrix = 1; colours[1].range = 7;
  CHECK(sjpeg_internal::yuv_colour_check("t", 2, colours.get(), 1) == SJPEG_HIP_EINVAL);
  CHECK(g_error == "t: frame 1: colour: range 7 is not one of 0..1 (SJPEG_HIP_RANGE_FULL, _LIMITED)");
  colours[1].range = 1; colours[0].reserved[1] = 1;
  CHECK(sjpeg_internal::yuv_colour_check("t", 2, colours.get(), 0) == SJPEG_HIP_EINVAL && g_error == "t: colour: reserved must be 0");
  CHECK(!sjpeg_internal::yuv_colour_all_identity(2, colours.get(), 0));          // (not in order: no identity)
  colours[0].reserved[1] = 0;
  CHECK(sjpeg_internal::yuv_colour_check("t", 2, colours.get(), 1) == 0 && sjpeg_internal::yuv_colour_check("t", 2, nullptr, 1) == 0);
  CHECK(sjpeg_internal::yuv_colour_all_identity(2, colours.get(), 0) && !sjpeg_internal::yuv_colour_all_identity(2, colours.get(), 1));
  CHECK(sjpeg_internal::yuv_colour_all_identity(2, nullptr, 1));
  // the host formula on samples in heap buffers of exactly their size
  std::unique_ptr<uint8_t[][3]> in(new uint8_t[3][3]), outp(new uint8_t[3][3]);
  const uint8_t src[3][3] = {{16, 128, 128}, {235, 128, 128}, {81, 90, 240}};
  memcpy(in.get(), src, sizeof(src));
  CHECK(sjpeg_hip_yuv_colour_samples(&colours[1], 3, in.get(), outp.get()) == 0);
  CHECK(outp[0][0] == 0 && outp[0][1] == 128 && outp[1][0] == 255 && outp[1][2] == 128);
  CHECK(sjpeg_hip_yuv_colour_samples(&colours[0], 3, in.get(), outp.get()) == 0 && memcmp(in.get(), outp.get(), 9) == 0);
  CHECK(sjpeg_hip_yuv_colour_samples(nullptr, 3, in.get(), outp.get()) == SJPEG_HIP_EINVAL);
  CHECK(sjpeg_hip_yuv_colour_samples(&colours[1], 3, nullptr, outp.get()) == SJPEG_HIP_EINVAL);
  return 0;
}

int main() {
  const int formats[4] = {SJPEG_HIP_SRC_YUV444, SJPEG_HIP_SRC_YUV420, SJPEG_HIP_SRC_NV12, SJPEG_HIP_SRC_NV21};
  uint32_t seed = 20261;
  long plans = 0;
  for (int round = 0; round < 30; ++round) {
    for (int format : formats) {
      if (one_batch(format, 1 + round % 9, false, &seed, &plans) != 0) return 1;
      if (one_batch(format, 1 + round % 9, true, &seed, &plans) != 0) return 1;
    }
  }
  if (refusals() != 0) return 1;
  printf("yuv colour plan ok: %ld plans\n", plans);
  return 0;
}
