// The host half of resampling with Pillow's filters (sjpeg_amd/csrc/resample_plan.cc) alone, under AddressSanitizer and
// UndefinedBehaviorSanitizer: tests/test_resample_cxx.py builds this file with it by the host compiler.  Sources of
// interleaved RGB and of gray lie in heap buffers of exactly their bytes; the plan's descriptors, sizes, layout and bytes
// are held to them, the tables are shared per (filter, in, out), and then the kernel's rule (resample.hip, restated
// here: the tile, the segment staged row by row in chunks, the horizontal pass into the uint8 intermediate, the vertical
// pass over the chunk's coefficients, the store, turned or not) is walked workgroup by workgroup over those buffers:
// every load and store lies inside its buffer, every sample is stored exactly once, and the bytes equal the two passes
// written here from resample_math.h's sample.  The refusals come back as SJPEG_HIP_EINVAL with their words.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../sjpeg_amd/csrc/orient_math.h"
#include "../../sjpeg_amd/csrc/ragged_aux.h"
#include "../../sjpeg_amd/csrc/resample_math.h"
#include "sjpeg_hip.h"

static std::string g_error;
namespace sjpeg_internal {
int set_error(int code, const std::string& msg) { g_error = msg; return code; }
}  // namespace sjpeg_internal

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #c, g_error.c_str()); return 1; } } while (0)

using namespace sjpeg_internal;

struct Case { int w, h, w2, h2, filter, orient; };

static bool said(const char* words) { return g_error.find(words) != std::string::npos; }

// a source of `channels` interleaved bytes a pixel in a heap buffer of exactly its bytes (no row padding)
struct Source {
  std::unique_ptr<uint8_t[]> buf;
  sjpeg_hip_ragged_frame frame;
};
static Source make_source(int w, int h, int channels, unsigned seed) {
  Source s;
  const size_t n = static_cast<size_t>(w) * h * channels;
  s.buf.reset(new uint8_t[n]);
  for (size_t i = 0; i < n; ++i) { seed = seed * 1664525u + 1013904223u; s.buf[i] = (seed >> 28) == 0 ? 0 : (seed >> 28) == 1 ? 255 : static_cast<uint8_t>(seed >> 16); }
  memset(&s.frame, 0, sizeof(s.frame));
  s.frame.width = w; s.frame.height = h;
  s.frame.plane[0] = s.buf.get();
  s.frame.row_stride[0] = static_cast<int64_t>(w) * channels;
  return s;
}

// the two passes, from resample_math.h's tables and sample: [h2][w2][channels]
static std::vector<uint8_t> expect(const Source& s, int channels, int w2, int h2, int filter) {
  const int w = s.frame.width, h = s.frame.height;
  std::vector<int32_t> xb, xk, yb, yk;
  int ksx = 1, ksy = 1;
  if (w2 != w) { resample_table(filter, w, w2, &xb, &xk); ksx = static_cast<int>(resample_ksize(filter, w, w2)); } else resample_identity_table(w, &xb, &xk);
  if (h2 != h) { resample_table(filter, h, h2, &yb, &yk); ksy = static_cast<int>(resample_ksize(filter, h, h2)); } else resample_identity_table(h, &yb, &yk);
  std::vector<uint8_t> mid(static_cast<size_t>(h) * w2 * channels), out(static_cast<size_t>(h2) * w2 * channels);
  for (int y = 0; y < h; ++y) for (int x = 0; x < w2; ++x) for (int c = 0; c < channels; ++c) {
    mid[(static_cast<size_t>(y) * w2 + x) * channels + c] = static_cast<uint8_t>(resample_sample(
        &xk[static_cast<size_t>(x) * ksx], s.buf.get() + (static_cast<size_t>(y) * w + xb[2 * x]) * channels + c, xb[2 * x + 1], channels));
  }
  for (int y = 0; y < h2; ++y) for (int x = 0; x < w2; ++x) for (int c = 0; c < channels; ++c) {
    out[(static_cast<size_t>(y) * w2 + x) * channels + c] = static_cast<uint8_t>(resample_sample(
        &yk[static_cast<size_t>(y) * ksy], &mid[(static_cast<size_t>(yb[2 * y]) * w2 + x) * channels + c], yb[2 * y + 1], static_cast<long long>(w2) * channels));
  }
  return out;
}

// resample.hip's kernel, workgroup `wg`, restated: the same tile, segment, chunks, passes and stores, on heap memory
static int walk(const ResamplePlan& plan, int channels, unsigned wg, uint8_t* dst_base, std::vector<uint8_t>* stored, long long* samples) {
  int lo = 0, hi = static_cast<int>(plan.frames.size()) - 1;
  while (lo < hi) { const int m = (lo + hi + 1) >> 1; if (plan.frames[m].tile_base <= wg) lo = m; else hi = m - 1; }
  const ResampleFrame& d = plan.frames[lo];
  const int32_t* const T = plan.tables.data();
  const int32_t *xb = T + reinterpret_cast<uintptr_t>(d.xb) / 4, *xk = T + reinterpret_cast<uintptr_t>(d.xk) / 4;
  const int32_t *yb = T + reinterpret_cast<uintptr_t>(d.yb) / 4, *yk = T + reinterpret_cast<uintptr_t>(d.yk) / 4;
  const unsigned t = wg - d.tile_base, tyi = t / d.tiles_x, txi = t - tyi * d.tiles_x;
  const int ox0 = static_cast<int>(txi) * d.tw, oy0 = static_cast<int>(tyi) * static_cast<int>(kResampleTileRows);
  CHECK(d.tw == 4 || d.tw == 8 || d.tw == 16 || d.tw == 32);
  CHECK(ox0 < d.w2 && oy0 < d.h2);
  const int tw = std::min(d.tw, d.w2 - ox0), th = std::min(static_cast<int>(kResampleTileRows), d.h2 - oy0), cols = tw * channels;
  const int xs = xb[2 * ox0], xe = xb[2 * (ox0 + tw - 1)] + xb[2 * (ox0 + tw - 1) + 1];
  const int ys = yb[2 * oy0], ye = yb[2 * (oy0 + th - 1)] + yb[2 * (oy0 + th - 1) + 1];
  CHECK(xs >= 0 && xs < xe && xe <= d.W && ys >= 0 && ys < ye && ye <= d.H);
  const unsigned seg = static_cast<unsigned>(xe - xs), lstep = static_cast<unsigned>(channels);   // (packed pixels, or gray)
  CHECK(seg <= kResampleSegmentMax);
  const unsigned rpitch = (seg * lstep + 3u) & ~3u;
  const int R = std::min(static_cast<int>(kResampleTileRows), static_cast<int>(kResampleStageBytes / rpitch));
  CHECK(R >= 1);
  std::unique_ptr<uint8_t[]> stage(new uint8_t[static_cast<size_t>(R) * rpitch]);
  std::unique_ptr<uint8_t[]> mid(new uint8_t[kResampleTileRows * kResampleTileCols * 3]);
  std::vector<int32_t> vacc(static_cast<size_t>(th) * cols, kResampleHalf);
  const int G = 256 / cols;
  CHECK(G >= 2 && 8 * G >= R);
  for (int y0 = ys; y0 < ye; y0 += R) {
    const int nr = std::min(R, ye - y0);
    for (int r = 0; r < nr; ++r) {
      memcpy(stage.get() + static_cast<size_t>(r) * rpitch, d.src + static_cast<long long>(y0 + r) * d.row_stride + static_cast<long long>(xs) * lstep,
             static_cast<size_t>(seg) * lstep);
    }
    for (int tid = 0; tid < 256; ++tid) {
      const int hcol = tid % cols, rg = tid / cols;
      if (rg >= G) continue;
      const int hj = hcol / channels, hc = hcol - hj * channels;
      const int hxmin = xb[2 * (ox0 + hj)], hn = xb[2 * (ox0 + hj) + 1];
      CHECK(hxmin >= xs && hxmin + hn <= xe && hn <= d.ksx);
      for (int m = 0; m < 8; ++m) {
        const int r = rg + G * m;
        if (r >= nr) continue;
        mid[r * kResampleTileCols * 3 + hcol] = static_cast<uint8_t>(resample_sample(
            xk + static_cast<size_t>(ox0 + hj) * d.ksx, stage.get() + static_cast<size_t>(r) * rpitch + static_cast<unsigned>(hxmin - xs) * lstep + hc,
            hn, lstep));
      }
    }
    for (int r = 0; r < th; ++r) {
      const int wmin = yb[2 * (oy0 + r)], wend = wmin + yb[2 * (oy0 + r) + 1];
      CHECK(wend - wmin <= d.ksy && wmin >= ys && wend <= ye);
      for (int yy = 0; yy < nr; ++yy) {
        const int y = y0 + yy;
        const int32_t k = y >= wmin && y < wend ? yk[static_cast<size_t>(oy0 + r) * d.ksy + (y - wmin)] : 0;
        for (int cb = 0; cb < cols; ++cb) vacc[static_cast<size_t>(r) * cols + cb] = resample_mac(vacc[static_cast<size_t>(r) * cols + cb], k, mid[yy * kResampleTileCols * 3 + cb]);
      }
    }
  }
  uint32_t uw, uh;
  oriented_size(static_cast<uint32_t>(d.w2), static_cast<uint32_t>(d.h2), static_cast<int>(d.orient), &uw, &uh);
  uint8_t* const dst = dst_base + reinterpret_cast<uintptr_t>(d.dst);
  for (int r = 0; r < th; ++r) for (int cb = 0; cb < cols; ++cb) {
    const int j = cb / channels, c = cb - j * channels;
    uint32_t ux, uy;
    orient_upright(static_cast<uint32_t>(ox0 + j), static_cast<uint32_t>(oy0 + r), static_cast<uint32_t>(d.w2), static_cast<uint32_t>(d.h2),
                   static_cast<int>(d.orient), &ux, &uy);
    CHECK(ux < uw && uy < uh);
    const size_t at = static_cast<size_t>(dst - dst_base) + static_cast<size_t>(uy) * d.dst_stride + static_cast<size_t>(ux) * channels + c;
    CHECK((*stored)[at] == 0);
    (*stored)[at] = 1;
    dst_base[at] = static_cast<uint8_t>(resample_clip(vacc[static_cast<size_t>(r) * cols + cb]));
    ++*samples;
  }
  if (d.orient <= 1) {
    // the unturned tile leaves as whole dwords: the last one ends inside the row's stride
    CHECK((static_cast<size_t>(ox0) * channels) % 4 == 0 && static_cast<size_t>(ox0) * channels + ((cols + 3) & ~3) <= d.dst_stride);
  }
  return 0;
}

static int run_batch(int format, const std::vector<Case>& cases, long long* samples) {
  const int channels = format == SJPEG_HIP_SRC_RGB ? 3 : 1;
  std::vector<Source> srcs;
  std::vector<sjpeg_hip_ragged_frame> frames;
  std::vector<int32_t> sizes;
  std::vector<uint8_t> orients;
  std::vector<sjpeg_hip_resample> rs;
  for (size_t k = 0; k < cases.size(); ++k) {
    srcs.push_back(make_source(cases[k].w, cases[k].h, channels, 77u + static_cast<unsigned>(k)));
    frames.push_back(srcs.back().frame);
    sizes.push_back(cases[k].w2); sizes.push_back(cases[k].h2);
    orients.push_back(static_cast<uint8_t>(cases[k].orient));
    rs.push_back(sjpeg_hip_resample{static_cast<uint8_t>(cases[k].filter), {0, 0, 0}});
  }
  const int n = static_cast<int>(cases.size());
  const int32_t (*sz)[2] = reinterpret_cast<const int32_t (*)[2]>(sizes.data());
  ResamplePlan plan;
  CHECK(resample_plan("t", format, n, frames.data(), sz, orients.data(), rs.data(), 1, nullptr, &plan) == 0);
  CHECK(plan.resized_format == (channels == 3 ? SJPEG_HIP_SRC_RGB : SJPEG_HIP_SRC_GRAY));
  CHECK(plan.bytes == sjpeg_hip_resample_ragged_bytes(format, n, frames.data(), sz, orients.data()) && plan.bytes > 0);
  std::unique_ptr<uint8_t[]> dst(new uint8_t[plan.bytes]);
  memset(dst.get(), 0xcd, plan.bytes);
  std::vector<uint8_t> stored(plan.bytes, 0);
  // layout: every picture at a multiple of 16, rows whole dwords apart, the upright size reported
  std::vector<sjpeg_hip_ragged_frame> made(n);
  resample_plan_frames(plan, frames.data(), dst.get(), made.data());
  size_t at = 0;
  unsigned tiles = 0;
  for (int f = 0; f < n; ++f) {
    const Case& c = cases[f];
    const ResampleFrame& d = plan.frames[f];
    const int uw = c.orient >= 5 ? c.h2 : c.w2, uh = c.orient >= 5 ? c.w2 : c.h2;
    CHECK(made[f].width == uw && made[f].height == uh && made[f].plane[0] == dst.get() + at);
    CHECK(made[f].row_stride[0] == ((uw * channels + 3) & ~3) && at % 16 == 0);
    at += (static_cast<size_t>(made[f].row_stride[0]) * uh + 15) & ~static_cast<size_t>(15);
    CHECK(d.tile_base == tiles && d.W == c.w && d.H == c.h && d.w2 == c.w2 && d.h2 == c.h2);
    CHECK(d.ksx == (c.w == c.w2 ? 1 : sjpeg_hip_resample_ksize(c.filter, c.w, c.w2)));
    CHECK(d.ksy == (c.h == c.h2 ? 1 : sjpeg_hip_resample_ksize(c.filter, c.h, c.h2)));
    tiles += d.tiles_x * ((static_cast<unsigned>(c.h2) + kResampleTileRows - 1) / kResampleTileRows);
  }
  CHECK(at == plan.bytes && tiles == plan.tiles);
  for (unsigned wg = 0; wg < plan.tiles; ++wg) {
    if (walk(plan, channels, wg, dst.get(), &stored, samples) != 0) { printf("  (workgroup %u)\n", wg); return 1; }
  }
  for (int f = 0; f < n; ++f) {
    const Case& c = cases[f];
    const std::vector<uint8_t> want = expect(srcs[f], channels, c.w2, c.h2, c.filter);
    const uint8_t* const p = static_cast<const uint8_t*>(made[f].plane[0]);
    for (int y = 0; y < c.h2; ++y) for (int x = 0; x < c.w2; ++x) {
      uint32_t ux, uy;
      orient_upright(static_cast<uint32_t>(x), static_cast<uint32_t>(y), static_cast<uint32_t>(c.w2), static_cast<uint32_t>(c.h2), c.orient, &ux, &uy);
      for (int ch = 0; ch < channels; ++ch) {
        const size_t o = static_cast<size_t>(uy) * made[f].row_stride[0] + static_cast<size_t>(ux) * channels + ch;
        CHECK(stored[static_cast<size_t>(p - dst.get()) + o] == 1);
        CHECK(p[o] == want[(static_cast<size_t>(y) * c.w2 + x) * channels + ch]);
      }
    }
  }
  return 0;
}

int main() {
  // ---- the kernel's rule over the plan: tile edges, tiny pictures, each axis alone, enlarging, a strip, the cap, turns
  std::vector<Case> cases;
  const int widths[] = {31, 32, 33, 34, 63, 64, 65}, heights[] = {15, 16, 17, 18, 31, 32, 33};
  for (int k = 0; k < 7; ++k) cases.push_back({48, 24, widths[k], heights[k], k % 5, 1});
  const Case more[] = {{1, 1, 1, 1, 4, 1}, {1, 1, 3, 3, 3, 1}, {2, 1, 1, 2, 2, 1}, {1, 2, 2, 1, 1, 1}, {3, 3, 1, 1, 0, 1}, {3, 3, 3, 3, 4, 5},
                       {50, 40, 50, 17, 4, 1}, {50, 40, 23, 40, 3, 1}, {50, 40, 75, 13, 2, 1}, {50, 40, 20, 90, 1, 1}, {20, 12, 30, 18, 0, 1},
                       {9, 7, 63, 49, 4, 1}, {100, 60, 37, 23, 3, 1}, {700, 5, 3, 2, 0, 1}, {192, 192, 3, 3, 4, 1}, {384, 4, 1, 4, 0, 1},
                       {1500, 3, 5, 3, 0, 1}, {12000, 2, 32, 2, 0, 1}, {12000, 2, 33, 40, 0, 3}};
  for (const Case& c : more) cases.push_back(c);
  for (int o = 1; o <= 8; ++o) cases.push_back({40, 23, 57, 11, o % 5, o});
  long long samples = 0;
  if (run_batch(SJPEG_HIP_SRC_RGB, cases, &samples) != 0) return 1;
  if (run_batch(SJPEG_HIP_SRC_GRAY, cases, &samples) != 0) return 1;

  // ---- tables are shared per (filter, in, out): 100 frames of 1920 x 1080 to 320 x 180 upload two
  {
    std::unique_ptr<uint8_t[]> one(new uint8_t[1920 * 1080 * 3]());
    std::vector<sjpeg_hip_ragged_frame> frames(100);
    std::vector<int32_t> sizes;
    for (auto& f : frames) { memset(&f, 0, sizeof(f)); f.width = 1920; f.height = 1080; f.plane[0] = one.get(); f.row_stride[0] = 1920 * 3; sizes.push_back(320); sizes.push_back(180); }
    const sjpeg_hip_resample lanczos = {SJPEG_HIP_RESAMPLE_LANCZOS, {0, 0, 0}};
    ResamplePlan plan;
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 100, frames.data(), reinterpret_cast<const int32_t (*)[2]>(sizes.data()), nullptr, &lanczos, 0, nullptr, &plan) == 0);
    CHECK(plan.ntables == 2 && plan.tables.size() == 320u * (2 + 37) + 180u * (2 + 37));
    CHECK(plan.frames[0].ksx == 37 && plan.frames[0].ksy == 37 && plan.frames[0].tw == 32 && plan.tiles == 100u * 10 * 12);
    for (int f = 1; f < 100; ++f) CHECK(plan.frames[f].xk == plan.frames[0].xk && plan.frames[f].yb == plan.frames[0].yb);
    // two filters, the same sizes: four; a square frame shares one table between its axes; own size: one identity table
    std::vector<sjpeg_hip_resample> mixed(100, lanczos);
    for (int f = 0; f < 100; f += 2) mixed[f].filter = SJPEG_HIP_RESAMPLE_BICUBIC;
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 100, frames.data(), reinterpret_cast<const int32_t (*)[2]>(sizes.data()), nullptr, mixed.data(), 1, nullptr, &plan) == 0);
    CHECK(plan.ntables == 4);
    frames[0].width = frames[0].height = 64;
    const int32_t sq[1][2] = {{20, 20}}, own[1][2] = {{64, 64}};
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, frames.data(), sq, nullptr, &lanczos, 0, nullptr, &plan) == 0 && plan.ntables == 1);
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, frames.data(), own, nullptr, &lanczos, 0, nullptr, &plan) == 0 && plan.ntables == 1);
    CHECK(plan.frames[0].ksx == 1 && plan.tables.size() == 64u * 3);
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, frames.data(), nullptr, nullptr, &lanczos, 0, nullptr, &plan) == 0 && plan.ntables == 1);
  }

  // ---- the refusals
  {
    Source s = make_source(400, 200, 3, 5);
    const sjpeg_hip_resample lanczos = {SJPEG_HIP_RESAMPLE_LANCZOS, {0, 0, 0}}, box = {SJPEG_HIP_RESAMPLE_BOX, {0, 0, 0}};
    ResamplePlan plan;
    const int32_t ok[1][2] = {{100, 50}};
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, ok, nullptr, nullptr, 0, nullptr, &plan) == SJPEG_HIP_EINVAL && said("resample == NULL"));
    sjpeg_hip_resample bad = {5, {0, 0, 0}};
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, ok, nullptr, &bad, 1, nullptr, &plan) == SJPEG_HIP_EINVAL && said("frame 0: resample: filter 5 is not one of"));
    bad = {4, {0, 0, 1}};
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, ok, nullptr, &bad, 0, nullptr, &plan) == SJPEG_HIP_EINVAL && said("t: resample: reserved must be 0"));
    const int32_t zero[1][2] = {{0, 50}}, huge[1][2] = {{100, 65536}}, top[1][2] = {{65535, 1}};
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, zero, nullptr, &box, 0, nullptr, &plan) == SJPEG_HIP_EINVAL && said("frame 0: size 0x50 is below 1x1"));
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, huge, nullptr, &box, 0, nullptr, &plan) == SJPEG_HIP_EINVAL && said("size 100x65536 is above 65535x65535"));
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, top, nullptr, &box, 0, nullptr, &plan) == 0 && plan.frames[0].w2 == 65535);
    // the cap: Lanczos 400 -> 6 is 2 * ceil(3 * 400 / 6) + 1 = 401 samples; 400 -> 7 is 345
    const int32_t over[1][2] = {{6, 200}}, under[1][2] = {{7, 200}}, overy[1][2] = {{400, 3}};
    CHECK(sjpeg_hip_resample_ksize(SJPEG_HIP_RESAMPLE_LANCZOS, 400, 6) == 401 && sjpeg_hip_resample_ksize(SJPEG_HIP_RESAMPLE_LANCZOS, 400, 7) == 345);
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, over, nullptr, &lanczos, 0, nullptr, &plan) == SJPEG_HIP_EINVAL);
    CHECK(said("frame 0: the x axis, 400 to 6 samples with SJPEG_HIP_RESAMPLE_LANCZOS, takes a window of 401 samples, above the cap of 385"));
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, overy, nullptr, &lanczos, 0, nullptr, &plan) == SJPEG_HIP_EINVAL && said("the y axis, 200 to 3 samples"));
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, under, nullptr, &lanczos, 0, nullptr, &plan) == 0);
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, over, nullptr, &box, 0, nullptr, &plan) == 0);    // (box: 69 samples)
    CHECK(sjpeg_hip_resample_ragged_bytes(SJPEG_HIP_SRC_RGB, 1, &s.frame, zero, nullptr) == 0);
    for (int format : {SJPEG_HIP_SRC_NV12, SJPEG_HIP_SRC_NV21, SJPEG_HIP_SRC_YUV420, SJPEG_HIP_SRC_YUV444}) {
      CHECK(resample_plan("t", format, 1, &s.frame, ok, nullptr, &lanczos, 0, nullptr, &plan) == SJPEG_HIP_EINVAL && said("pictures are not resampled"));
    }
    CHECK(said("SJPEG_HIP_SRC_YUV444"));
    const uint8_t nine = 9;
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, ok, &nine, &lanczos, 0, nullptr, &plan) == SJPEG_HIP_EINVAL && said("orientation 9"));
    const sjpeg_hip_flatten fl = {{1, 2, 3}, 0, 255.0f, 0.0f};
    CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, ok, nullptr, &lanczos, 0, &fl, &plan) == SJPEG_HIP_EINVAL && said("has no alpha channel"));
    // the host entries
    int32_t b[4][2], K[4 * 7];
    CHECK(sjpeg_hip_resample_ksize(7, 2, 4) == 0 && said("filter 7"));
    CHECK(sjpeg_hip_resample_ksize(0, 0, 4) == 0 && sjpeg_hip_resample_ksize(0, 4, 65536) == 0);
    CHECK(sjpeg_hip_resample_table(SJPEG_HIP_RESAMPLE_LANCZOS, 2, 4, b, K, 27) == SJPEG_HIP_EINVAL && said("K_capacity 27 is below the 28"));
    CHECK(sjpeg_hip_resample_table(SJPEG_HIP_RESAMPLE_LANCZOS, 2, 4, nullptr, K, 28) == SJPEG_HIP_EINVAL);
    CHECK(sjpeg_hip_resample_table(SJPEG_HIP_RESAMPLE_LANCZOS, 2, 4, b, K, 28) == 0 && b[0][0] == 0 && b[3][0] + b[3][1] == 2);
  }
  printf("resample plan ok: %lld samples\n", samples);
  return 0;
}
