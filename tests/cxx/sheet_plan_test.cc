// The host half of the contact sheets (sjpeg_amd/csrc/sheet_plan.cc) with the two plans it reuses (resize_plan.cc,
// yuv_resize_plan.cc), under AddressSanitizer and UndefinedBehaviorSanitizer: tests/test_sheet_plan_cxx.py builds this
// file with them by the host compiler.  Every array handed over lies in a heap buffer of exactly its size.  For
// batches of RGB-like, gray and all four YUV-plane formats, given and fitted sizes, every orientation, the plan is
// held to the header's words: every thumbnail rectangle inside its cell, the cells disjoint and inside the sheet,
// chroma places half the luma's, `places` agreeing with the descriptors, `bytes` the documented layout.
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

static size_t align4(size_t n) { return (n + 3) & ~static_cast<size_t>(3); }
static size_t align16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }
static bool is_yuv(int format) {
  return format == SJPEG_HIP_SRC_YUV444 || format == SJPEG_HIP_SRC_YUV420 || format == SJPEG_HIP_SRC_NV12 || format == SJPEG_HIP_SRC_NV21;
}
static bool is_gray(int format) {
  return format == SJPEG_HIP_SRC_GRAY || format == SJPEG_HIP_SRC_GRAY_F32 || format == SJPEG_HIP_SRC_GRAY_F16 || format == SJPEG_HIP_SRC_GRAY_BF16;
}

struct Rect { long long x, y, w, h; };
static bool inside(const Rect& a, const Rect& b) { return a.x >= b.x && a.y >= b.y && a.x + a.w <= b.x + b.w && a.y + a.h <= b.y + b.h; }
static bool disjoint(const Rect& a, const Rect& b) { return a.x + a.w <= b.x || b.x + b.w <= a.x || a.y + a.h <= b.y || b.y + b.h <= a.y; }

static int one_batch(int format, int nframes, uint32_t* seed, long* plans) {
  auto next = [&]() { *seed = *seed * 1664525u + 1013904223u; return *seed >> 8; };
  const bool yuv = is_yuv(format), half = yuv && format != SJPEG_HIP_SRC_YUV444;
  const int nplanes = !yuv ? 1 : format == SJPEG_HIP_SRC_NV12 || format == SJPEG_HIP_SRC_NV21 ? 2 : 3;
  const int channels = yuv || is_gray(format) ? 1 : 3;
  std::unique_ptr<sjpeg_hip_sheet> sheet(new sjpeg_hip_sheet);
  memset(sheet.get(), 0, sizeof(sjpeg_hip_sheet));
  const int even = half ? 2 : 1;
  sheet->cols = 1 + static_cast<int>(next() % 4); sheet->rows = 1 + static_cast<int>(next() % 3);
  sheet->cell_width = even * (1 + static_cast<int>(next() % 40)); sheet->cell_height = even * (1 + static_cast<int>(next() % 30));
  sheet->gutter = even * static_cast<int>(next() % 4); sheet->margin = even * static_cast<int>(next() % 4);
  sheet->background[0] = 0x11; sheet->background[1] = 0x7E; sheet->background[2] = 0xEF;
  std::unique_ptr<sjpeg_hip_ragged_frame[]> frames(new sjpeg_hip_ragged_frame[nframes]);
  std::unique_ptr<int32_t[][2]> sizes(new int32_t[nframes][2]);
  std::unique_ptr<uint8_t[]> orients(new uint8_t[nframes]);
  for (int f = 0; f < nframes; ++f) {
    memset(&frames[f], 0, sizeof(frames[f]));
    orients[f] = static_cast<uint8_t>(1 + next() % 8);
    const bool t = orients[f] >= 5;
    // a given size whose upright form fits the cell; a source at least that large
    const int bw = t ? sheet->cell_height : sheet->cell_width, bh = t ? sheet->cell_width : sheet->cell_height;
    sizes[f][0] = 1 + static_cast<int>(next() % bw); sizes[f][1] = 1 + static_cast<int>(next() % bh);
    const int big = next() % 16 == 0;
    frames[f].width = sizes[f][0] + static_cast<int>(next() % (big ? 65536 - sizes[f][0] : 700));
    frames[f].height = sizes[f][1] + static_cast<int>(next() % (big ? 65536 - sizes[f][1] : 90));
    for (int i = 0; i < 3; ++i) {
      frames[f].plane[i] = reinterpret_cast<void*>(static_cast<uintptr_t>(0x10000000u + 0x1000000u * i));
      frames[f].row_stride[i] = 1 << 20;
    }
  }
  int SW = 0, SH = 0;
  CHECK(sjpeg_hip_sheet_size(sheet.get(), format, &SW, &SH) == 0);
  CHECK(SW == 2 * sheet->margin + sheet->cols * sheet->cell_width + (sheet->cols - 1) * sheet->gutter);
  CHECK(SH == 2 * sheet->margin + sheet->rows * sheet->cell_height + (sheet->rows - 1) * sheet->gutter);
  const int per = sheet->cols * sheet->rows, nsheets = (nframes + per - 1) / per;
  // the documented layout of a sheet
  size_t off[3] = {0, 0, 0}, stride[3] = {0, 0, 0}, sheet_bytes = 0;
  int pw[3], ph[3];
  for (int c = 0; c < (yuv ? 3 : 1); ++c) {
    pw[c] = c > 0 && half ? SW / 2 : SW; ph[c] = c > 0 && half ? SH / 2 : SH;
    off[c] = sheet_bytes; stride[c] = align4(static_cast<size_t>(pw[c]) * channels);
    sheet_bytes += align16(stride[c] * ph[c]);
  }
  for (int variant = 0; variant < 4; ++variant) {
    const int32_t (*sz)[2] = variant & 1 ? nullptr : sizes.get();
    const uint8_t* orr = variant & 2 ? nullptr : orients.get();
    if (sz != nullptr && orr == nullptr) {
      // (the given sizes fit the cell turned as `orients` say: without the orientations they need not)
      bool fits = true;
      for (int f = 0; f < nframes; ++f) fits = fits && sizes[f][0] <= sheet->cell_width && sizes[f][1] <= sheet->cell_height;
      if (!fits) continue;
    }
    sjpeg_internal::SheetPlan plan;
    CHECK(sjpeg_internal::sheet_plan("test", format, nframes, frames.get(), sheet.get(), sz, orr, &plan) == 0);
    ++*plans;
    CHECK(plan.nframes == nframes && plan.nsheets == nsheets && plan.width == SW && plan.height == SH && plan.yuv == yuv);
    CHECK(plan.out_format == (!yuv ? (channels == 3 ? SJPEG_HIP_SRC_RGB : SJPEG_HIP_SRC_GRAY)
                                   : format == SJPEG_HIP_SRC_YUV444 ? SJPEG_HIP_SRC_YUV444 : SJPEG_HIP_SRC_YUV420));
    CHECK(plan.bytes == sheet_bytes * nsheets && plan.fill.sheet_bytes == sheet_bytes && plan.fill.nsheets == nsheets);
    CHECK(sjpeg_hip_sheet_ragged_bytes(format, nframes, frames.get(), sheet.get(), sz, orr) == plan.bytes);
    CHECK(plan.fill.nplanes == (yuv ? 3 : 1));
    for (int c = 0; c < plan.fill.nplanes; ++c) {
      CHECK(plan.fill.off[c] == off[c] && off[c] % 16 == 0 && plan.fill.rows[c] == static_cast<unsigned>(ph[c]));
      CHECK(plan.fill.row_dwords[c] * 4u == stride[c]);
      // the fill stays inside its plane, and its pattern is the background's bytes from a row's start
      CHECK(off[c] + static_cast<size_t>(plan.fill.rows[c]) * plan.fill.row_dwords[c] * 4 <= (c + 1 < plan.fill.nplanes ? off[c + 1] : sheet_bytes));
      for (int b = 0; b < 12; ++b) {
        const uint8_t got = static_cast<uint8_t>(plan.fill.pattern[c][b / 4] >> (8 * (b % 4)));
        CHECK(got == sheet->background[channels == 3 ? b % 3 : c]);
      }
    }
    std::unique_ptr<sjpeg_hip_ragged_frame[]> out(new sjpeg_hip_ragged_frame[nsheets]);
    uint8_t* const base = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(0x40000000u));
    sjpeg_internal::sheet_plan_frames(plan, base, out.get());
    for (int s = 0; s < nsheets; ++s) {
      CHECK(out[s].width == SW && out[s].height == SH);
      for (int c = 0; c < plan.fill.nplanes; ++c) {
        CHECK(out[s].plane[c] == base + s * sheet_bytes + off[c] && out[s].row_stride[c] == static_cast<int64_t>(stride[c]));
      }
    }
    std::unique_ptr<int32_t[][5]> places(new int32_t[nframes][5]);
    CHECK(sjpeg_hip_sheet_places(format, nframes, frames.get(), sheet.get(), sz, orr, places.get()) == 0);
    std::vector<Rect> cells(static_cast<size_t>(nframes));
    size_t k = 0;
    unsigned long long tiles = 0;
    for (int f = 0; f < nframes; ++f) {
      const int o = orr != nullptr ? orr[f] : 1;
      int w2, h2;
      if (sz != nullptr) {
        w2 = sz[f][0]; h2 = sz[f][1];
      } else {
        CHECK(sjpeg_hip_fit_size(frames[f].width, frames[f].height, o >= 5 ? sheet->cell_height : sheet->cell_width,
                                 o >= 5 ? sheet->cell_width : sheet->cell_height, &w2, &h2) == 0);
      }
      const int uw = o >= 5 ? h2 : w2, uh = o >= 5 ? w2 : h2;
      const sjpeg_internal::SheetPlace& p = plan.places[f];
      CHECK(places[f][0] == p.sheet && places[f][1] == p.x0 && places[f][2] == p.y0 && places[f][3] == p.uw && places[f][4] == p.uh);
      CHECK(p.sheet == f / per && p.uw == uw && p.uh == uh);
      const int cell = f % per, i = cell % sheet->cols, j = cell / sheet->cols;
      const Rect c = {sheet->margin + 1ll * i * (sheet->cell_width + sheet->gutter), sheet->margin + 1ll * j * (sheet->cell_height + sheet->gutter),
                      sheet->cell_width, sheet->cell_height};
      cells[f] = c;
      const Rect sheet_rect = {0, 0, SW, SH}, thumb = {p.x0, p.y0, uw, uh};
      CHECK(inside(c, sheet_rect) && inside(thumb, c));
      int ex = (sheet->cell_width - uw) / 2, ey = (sheet->cell_height - uh) / 2;
      if (half) { ex &= ~1; ey &= ~1; }
      CHECK(p.x0 == c.x + ex && p.y0 == c.y + ey);            // centred: the spare sample on the right and at the bottom
      if (half) {
        CHECK(p.x0 % 2 == 0 && p.y0 % 2 == 0 && c.x % 2 == 0 && c.y % 2 == 0);
        const Rect chroma = {p.x0 / 2, p.y0 / 2, (uw + 1) / 2, (uh + 1) / 2}, half_cell = {c.x / 2, c.y / 2, c.w / 2, c.h / 2};
        CHECK(inside(chroma, half_cell));                     // the chroma planes fit their half cell
      }
      for (int g = f - (f % per); g < f; ++g) CHECK(disjoint(cells[g], c));
      // the descriptors: where the kernel stores is where `places` say
      for (int n = 0; n < nplanes; ++n, ++k) {
        const sjpeg_internal::ResizeFrame& d = yuv ? plan.planes.planes[k].r : plan.rgb.frames[k];
        CHECK((d.orient & sjpeg_internal::kResizePlaced) != 0 && (d.orient & 0xffu) == static_cast<unsigned>(o));
        CHECK(d.tile_base == tiles);
        CHECK(d.tw >= 4 && d.tw <= 256 && (d.tw & (d.tw - 1)) == 0 && d.th >= 1 && d.th <= 16);
        tiles += static_cast<unsigned long long>(d.tiles_x) * ((d.h2 + d.th - 1) / d.th);
        const int c0 = n;                                      // (the plane the descriptor's dst lies in: Y, U)
        const bool ch = half && c0 > 0;
        const size_t want = p.sheet * sheet_bytes + off[c0] + static_cast<size_t>(ch ? p.y0 / 2 : p.y0) * stride[c0] +
                            static_cast<size_t>(ch ? p.x0 / 2 : p.x0) * channels;
        CHECK(reinterpret_cast<uintptr_t>(d.dst) == want && d.dst_stride == stride[c0]);
        const int dw = c0 > 0 && half ? (w2 + 1) / 2 : w2, dh = c0 > 0 && half ? (h2 + 1) / 2 : h2;
        CHECK(d.w2 == dw && d.h2 == dh);
        // the last byte the descriptor's picture holds lies inside its sheet plane
        const int duw = o >= 5 ? dh : dw, duh = o >= 5 ? dw : dh;
        const size_t last = want + static_cast<size_t>(duh - 1) * stride[c0] + static_cast<size_t>(duw) * channels;
        CHECK(last <= p.sheet * sheet_bytes + off[c0] + stride[c0] * ph[c0]);
        if (yuv && plan.planes.planes[k].channels == 2) {
          const uintptr_t v = reinterpret_cast<uintptr_t>(plan.planes.planes[k].dst2);
          CHECK(v == want - off[1] + off[2] && (v - want) % 16 == 0);   // V's plane laid out as U's: the same phase
        }
        if (yuv) CHECK(plan.planes.planes[k].frame == f);
      }
    }
    CHECK(tiles == (yuv ? plan.planes.tiles : plan.rgb.tiles));
    CHECK(k == (yuv ? plan.planes.planes.size() : plan.rgb.frames.size()));
  }
  return 0;
}

static int refusals() {
  std::unique_ptr<sjpeg_hip_sheet> sheet(new sjpeg_hip_sheet);
  std::unique_ptr<sjpeg_hip_ragged_frame[]> frames(new sjpeg_hip_ragged_frame[3]);
  std::unique_ptr<int32_t[][2]> sizes(new int32_t[3][2]);
  std::unique_ptr<uint8_t[]> orients(new uint8_t[3]);
  auto reset = [&]() {
    memset(sheet.get(), 0, sizeof(sjpeg_hip_sheet));
    sheet->cols = 2; sheet->rows = 1; sheet->cell_width = 16; sheet->cell_height = 10; sheet->gutter = 2; sheet->margin = 2;
    for (int f = 0; f < 3; ++f) {
      memset(&frames[f], 0, sizeof(frames[f]));
      frames[f].width = 64; frames[f].height = 40;
      sizes[f][0] = 16; sizes[f][1] = 10;
      orients[f] = 1;
    }
  };
  sjpeg_internal::SheetPlan plan;
  const int rgb = SJPEG_HIP_SRC_RGB, nv = SJPEG_HIP_SRC_NV12;
  int w = 0, h = 0;
  reset();
  CHECK(sjpeg_internal::sheet_plan("t", rgb, 3, frames.get(), sheet.get(), sizes.get(), orients.get(), &plan) == 0 && plan.nsheets == 2);
  orients[1] = 6;                                             // 16 x 10 stored is 10 x 16 upright: above the cell's 16 x 10
  CHECK(sjpeg_internal::sheet_plan("t", rgb, 3, frames.get(), sheet.get(), sizes.get(), orients.get(), &plan) == SJPEG_HIP_EINVAL);
  CHECK(g_error.find("frame 1") != std::string::npos && g_error.find("16x10") != std::string::npos && g_error.find("10x16") != std::string::npos &&
        g_error.find("orientation 6") != std::string::npos);
  CHECK(plan.places.empty() && plan.bytes == 0);              // a refused batch leaves no plan
  CHECK(sjpeg_internal::sheet_plan("t", rgb, 3, frames.get(), sheet.get(), nullptr, orients.get(), &plan) == 0);   // fitted: 6 x 10 upright
  CHECK(plan.places[1].uw == 6 && plan.places[1].uh == 10);
  reset(); sizes[2][0] = 65;
  CHECK(sjpeg_internal::sheet_plan("t", rgb, 3, frames.get(), sheet.get(), sizes.get(), nullptr, &plan) == SJPEG_HIP_EINVAL);
  CHECK(g_error.find("frame 2") != std::string::npos && g_error.find("above the source's 64x40") != std::string::npos);
  reset(); orients[0] = 9;
  CHECK(sjpeg_internal::sheet_plan("t", nv, 3, frames.get(), sheet.get(), nullptr, orients.get(), &plan) == SJPEG_HIP_EINVAL);
  CHECK(g_error.find("frame 0") != std::string::npos && g_error.find("orientation 9") != std::string::npos);
  reset(); frames[1].width = 0;
  CHECK(sjpeg_internal::sheet_plan("t", nv, 3, frames.get(), sheet.get(), nullptr, nullptr, &plan) == SJPEG_HIP_EINVAL);
  CHECK(g_error.find("frame 1") != std::string::npos && g_error.find("bad dimensions") != std::string::npos);
  reset(); sheet->cell_width = 15;
  CHECK(sjpeg_hip_sheet_size(sheet.get(), nv, &w, &h) == SJPEG_HIP_EINVAL && g_error.find("cell_width 15 is odd") != std::string::npos);
  CHECK(sjpeg_hip_sheet_size(sheet.get(), SJPEG_HIP_SRC_YUV444, &w, &h) == 0 && w == 2 * 2 + 2 * 15 + 2 && h == 14);
  reset(); sheet->gutter = 1;
  CHECK(sjpeg_hip_sheet_size(sheet.get(), nv, &w, &h) == SJPEG_HIP_EINVAL && g_error.find("gutter 1 is odd") != std::string::npos);
  reset(); sheet->reserved = 1;
  CHECK(sjpeg_hip_sheet_size(sheet.get(), rgb, &w, &h) == SJPEG_HIP_EINVAL && g_error.find("reserved") != std::string::npos);
  reset(); sheet->cols = 0;
  CHECK(sjpeg_hip_sheet_size(sheet.get(), rgb, &w, &h) == SJPEG_HIP_EINVAL && g_error.find("cols 0") != std::string::npos);
  reset(); sheet->cols = 4096; sheet->cell_width = 16;
  CHECK(sjpeg_hip_sheet_size(sheet.get(), rgb, &w, &h) == SJPEG_HIP_EINVAL && g_error.find("above 65535") != std::string::npos);
  reset(); sheet->cols = 65535; sheet->cell_width = 65535; sheet->gutter = 65535;       // (no overflow on the way)
  CHECK(sjpeg_hip_sheet_size(sheet.get(), rgb, &w, &h) == SJPEG_HIP_EINVAL && g_error.find("above 65535") != std::string::npos);
  reset();
  CHECK(sjpeg_hip_sheet_size(sheet.get(), 99, &w, &h) == SJPEG_HIP_EINVAL && sjpeg_hip_sheet_size(nullptr, rgb, &w, &h) == SJPEG_HIP_EINVAL);
  CHECK(sjpeg_hip_sheet_ragged_bytes(rgb, 3, nullptr, sheet.get(), nullptr, nullptr) == 0 && g_error.find("frames == NULL") != std::string::npos);
  CHECK(sjpeg_hip_sheet_ragged_bytes(rgb, 0, frames.get(), sheet.get(), nullptr, nullptr) == 0);
  return 0;
}

int main() {
  const int formats[8] = {SJPEG_HIP_SRC_RGB, SJPEG_HIP_SRC_BGRA, SJPEG_HIP_SRC_GRAY, SJPEG_HIP_SRC_RGB_PLANAR_F16,
                          SJPEG_HIP_SRC_YUV444, SJPEG_HIP_SRC_YUV420, SJPEG_HIP_SRC_NV12, SJPEG_HIP_SRC_NV21};
  uint32_t seed = 20251;
  long plans = 0;
  for (int round = 0; round < 16; ++round) {
    for (int format : formats) {
      if (one_batch(format, 1 + (round * 5) % 23, &seed, &plans) != 0) return 1;
    }
  }
  if (refusals() != 0) return 1;
  if (plans < 300) { printf("FAILED: only %ld plans\n", plans); return 1; }
  printf("sheet plan ok: %ld plans\n", plans);
  return 0;
}
