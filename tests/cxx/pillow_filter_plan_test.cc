// The host half of Pillow's filters (sjpeg_amd/csrc/pillow_filter_plan.cc) alone, under AddressSanitizer and
// UndefinedBehaviorSanitizer: tests/test_pillow_filter_cxx.py builds this file with it by the host compiler.  Every
// refusal comes back as SJPEG_HIP_EINVAL with its words and the frame's number; the plan's descriptors -- offsets,
// sizes, the weights of both axes, percent and threshold of an unsharp mask alone -- and the tile counts of the two
// launches are held to made pictures laid out as the resample plans lay them out.  pillow_filter_kernel_emul.cc includes
// this file for its pictures and its expectation: the closed form of sjpeg_hip.h, written here with clamped indices.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "../../sjpeg_amd/csrc/pillow_filter_math.h"
#include "../../sjpeg_amd/csrc/ragged_aux.h"
#include "sjpeg_hip.h"

static std::string g_error;
namespace sjpeg_internal {
int set_error(int code, const std::string& msg) { g_error = msg; return code; }
}  // namespace sjpeg_internal

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #c, g_error.c_str()); return 1; } } while (0)

using namespace sjpeg_internal;

struct Picture { int w, h; };
static size_t align_up(size_t n, size_t a) { return (n + a - 1) / a * a; }

// made pictures of `format` (RGB or gray) in one heap buffer of exactly their bytes: each at a multiple of 16, rows whole
// dwords apart
struct Batch {
  std::unique_ptr<uint8_t[]> buf;
  size_t bytes = 0;
  std::vector<sjpeg_hip_ragged_frame> frames;
};
static Batch make_batch(int format, const std::vector<Picture>& pics, unsigned seed) {
  Batch b;
  const int step = format == SJPEG_HIP_SRC_RGB ? 3 : 1;
  std::vector<size_t> offs;
  for (const Picture& p : pics) { offs.push_back(b.bytes); b.bytes += align_up(align_up((size_t)p.w * step, 4) * p.h, 16); }
  b.buf.reset(new uint8_t[b.bytes]);
  for (size_t i = 0; i < b.bytes; ++i) { seed = seed * 1664525u + 1013904223u; b.buf[i] = (uint8_t)(seed >> 24); }
  for (size_t k = 0; k < pics.size(); ++k) {
    sjpeg_hip_ragged_frame f;
    memset(&f, 0, sizeof(f));
    f.width = pics[k].w; f.height = pics[k].h;
    f.plane[0] = b.buf.get() + offs[k];
    f.row_stride[0] = (int64_t)align_up((size_t)pics[k].w * step, 4);
    b.frames.push_back(f);
  }
  return b;
}

static sjpeg_hip_pillow_filter filter_of(int kind, float rx, float ry, int percent = 0, int threshold = 0) {
  sjpeg_hip_pillow_filter f;
  memset(&f, 0, sizeof(f));
  f.kind = (uint8_t)kind; f.radius_x = rx; f.radius_y = ry; f.percent = (uint16_t)percent; f.threshold = (uint8_t)threshold;
  return f;
}

// ---- the expectation: one pass along an axis by the closed form, indices clamped
static void expect_pass(std::vector<uint8_t>* pic, int w, int h, int c, int axis, const PillowFilterAxis& a) {
  std::vector<uint8_t> out(pic->size());
  const int n = axis == 0 ? w : h, r = (int)a.r;
  auto at = [&](int x, int y, int ch) -> uint32_t { return (*pic)[((size_t)y * w + x) * c + ch]; };
  auto cl = [&](int i) { return i < 0 ? 0 : i > n - 1 ? n - 1 : i; };
  for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) for (int ch = 0; ch < c; ++ch) {
    const int i = axis == 0 ? x : y;
    uint64_t S = 0;
    for (int d = -r; d <= r; ++d) S += axis == 0 ? at(cl(i + d), y, ch) : at(x, cl(i + d), ch);
    const uint64_t edge = axis == 0 ? at(cl(i - r - 1), y, ch) + at(cl(i + r + 1), y, ch) : at(x, cl(i - r - 1), ch) + at(x, cl(i + r + 1), ch);
    const uint64_t v = (uint64_t)a.ww * S + (uint64_t)a.fw * edge + (1u << 23);
    if (v >> 32) { printf("a sample leaves uint32\n"); abort(); }
    out[((size_t)y * w + x) * c + ch] = (uint8_t)(v >> 24);
  }
  pic->swap(out);
}
static std::vector<uint8_t> expect_filter(const std::vector<uint8_t>& pic, int w, int h, int c, const sjpeg_hip_pillow_filter& f) {
  std::vector<uint8_t> b = pic;
  if (f.kind == 0) return b;
  const float radius[2] = {f.radius_x, f.radius_y};
  for (int axis = 0; axis < 2; ++axis) {
    const PillowFilterAxis a = pillow_filter_axis(f.kind, radius[axis]);
    for (uint32_t k = 0; k < a.passes; ++k) expect_pass(&b, w, h, c, axis, a);
  }
  if (f.kind != 3) return b;
  for (size_t i = 0; i < b.size(); ++i) {
    const int p = pic[i], d = p - b[i];
    int v = p;
    if (std::abs(d) > (int)f.threshold) { v = p + d * (int)f.percent / 100; v = v < 0 ? 0 : v > 255 ? 255 : v; }
    b[i] = (uint8_t)v;
  }
  return b;
}

static bool refused(int rc, const char* words) {
  if (rc != SJPEG_HIP_EINVAL || g_error.find(words) == std::string::npos) { printf("wanted a refusal with \"%s\", got %d: %s\n", words, rc, g_error.c_str()); return false; }
  return true;
}

static int plan_tests() {
  const std::vector<Picture> pics = {{1, 1}, {5, 7}, {70, 37}, {300, 160}, {300, 20}, {20, 300}, {129, 5}, {128, 65}};
  const size_t n = pics.size();
  for (int format : {SJPEG_HIP_SRC_RGB, SJPEG_HIP_SRC_GRAY}) {
    Batch b = make_batch(format, pics, 5);
    const unsigned step = format == SJPEG_HIP_SRC_RGB ? 3 : 1;
    std::vector<sjpeg_hip_pillow_filter> fs(n, filter_of(2, 2.0f, 2.0f));
    fs[0] = filter_of(0, 0, 0); fs[1] = filter_of(1, 5.0f, 0.0f); fs[2] = filter_of(3, 2.0f, 2.0f, 150, 3); fs[4] = filter_of(1, 63.9f, 63.0f);
    PillowFilterPlan plan;
    CHECK(pillow_filter_plan("t", format, (int)n, b.frames.data(), b.buf.get(), fs.data(), 1, &plan) == 0);
    CHECK(plan.planes.size() == n);
    unsigned long long t0 = 0, t1 = 0;
    for (size_t k = 0; k < n; ++k) {
      const PillowFilterPlane& d = plan.planes[k];
      const uintptr_t off = (uintptr_t)((const uint8_t*)b.frames[k].plane[0] - b.buf.get());
      CHECK((uintptr_t)d.made == off && (uintptr_t)d.mid == off && (uintptr_t)d.dst == off);
      CHECK(d.width == (unsigned)pics[k].w && d.rows == (unsigned)pics[k].h && d.step == step && d.stride == (unsigned)b.frames[k].row_stride[0]);
      CHECK(d.kind == fs[k].kind && d.percent == (fs[k].kind == 3 ? 150u : 0u) && d.threshold == (fs[k].kind == 3 ? 3u : 0u));
      CHECK(d.tile_base[0] == t0 && d.tile_base[1] == t1);
      const unsigned ndw = (pics[k].w * step + 3) / 4;
      t0 += (unsigned long long)((pics[k].w + 127) / 128) * ((pics[k].h + 3) / 4);
      t1 += (unsigned long long)((ndw + 3) / 4) * ((pics[k].h + 63) / 64);
      for (int a = 0; a < 2; ++a) {
        const PillowFilterAxis want = pillow_filter_axis(fs[k].kind, a == 0 ? fs[k].radius_x : fs[k].radius_y);
        CHECK(memcmp(&d.axis[a], &want, sizeof(want)) == 0);
      }
    }
    CHECK(plan.tiles[0] == t0 && plan.tiles[1] == t1);
    CHECK(plan.planes[0].axis[0].passes == 0 && plan.planes[1].axis[0].passes == 1 && plan.planes[1].axis[1].passes == 0);
    CHECK(plan.planes[2].axis[1].passes == 3 && plan.planes[2].axis[0].r == 1 && plan.planes[4].axis[0].r == 63 && plan.planes[4].axis[1].r == 63);
    // one filter for the call; none at all: every frame of kind 0, the same tiles
    CHECK(pillow_filter_plan("t", format, (int)n, b.frames.data(), b.buf.get(), &fs[2], 0, &plan) == 0 && plan.planes[7].kind == 3 && plan.tiles[0] == t0);
    CHECK(pillow_filter_plan("t", format, (int)n, b.frames.data(), b.buf.get(), nullptr, 0, &plan) == 0 && plan.planes[3].kind == 0 && plan.tiles[1] == t1);
  }
  // the tile counts said outright: 300 x 160 RGB is 3 x 40 row tiles and 57 x 3 column tiles
  CHECK(pillow_row_tiles(300, 160) == 120 && pillow_col_tiles(225, 160) == 171 && pillow_row_tiles(1, 1) == 1 && pillow_col_tiles(1, 1) == 1);
  CHECK(pillow_row_tiles(128, 4) == 1 && pillow_row_tiles(129, 5) == 4 && pillow_col_tiles(4, 64) == 1 && pillow_col_tiles(5, 65) == 4);

  // ---- the refusals
  Batch b = make_batch(SJPEG_HIP_SRC_RGB, {{9, 9}, {8, 8}, {7, 7}}, 9);
  PillowFilterPlan plan;
  auto plan_with = [&](sjpeg_hip_pillow_filter f, int per_frame = 1) {
    std::vector<sjpeg_hip_pillow_filter> fs(3, filter_of(2, 1.0f, 1.0f));
    fs[per_frame ? 2 : 0] = f;
    const int rc = pillow_filter_plan("who", SJPEG_HIP_SRC_RGB, 3, b.frames.data(), b.buf.get(), fs.data(), per_frame, &plan);
    const int rc2 = pillow_filter_check("who", 3, fs.data(), per_frame);
    if (rc != rc2 || (rc != 0) != plan.planes.empty()) return -1;       // (a refused plan is left empty)
    return rc;
  };
  CHECK(refused(plan_with(filter_of(4, 1, 1)), "who: frame 2: filter: kind 4 is not one of 0..3"));
  CHECK(refused(plan_with(filter_of(1, -0.5f, 1)), "who: frame 2: filter: radius_x is not a finite number of 0 or more"));
  CHECK(refused(plan_with(filter_of(2, 1, NAN)), "who: frame 2: filter: radius_y is not a finite number"));
  CHECK(refused(plan_with(filter_of(2, INFINITY, 1)), "who: frame 2: filter: radius_x is not a finite number"));
  CHECK(refused(plan_with(filter_of(1, 64.0f, 1)), "who: frame 2: filter: radius_x gives a box radius above 63 (Pillow has no such limit"));
  CHECK(refused(plan_with(filter_of(2, 1, 66.0f)), "who: frame 2: filter: radius_y gives a box radius above 63"));
  CHECK(refused(plan_with(filter_of(1, 3.0e9f, 1)), "radius_x gives a box radius above 63"));
  // sigmas whose radius formula cancels or overflows in float32 (-inf, NaN) are refused, not taken for a skipped axis
  for (float sigma : {1.0e6f, 1.4e15f, 1.0e16f, 2.0e19f, 1.0e30f, 3.4e38f}) {
    CHECK(refused(plan_with(filter_of(2, sigma, 1)), "who: frame 2: filter: radius_x gives a box radius above 63"));
    CHECK(refused(plan_with(filter_of(3, sigma, sigma, 150, 3)), "who: frame 2: filter: radius_x gives a box radius above 63"));
  }
  for (float sigma = 66.0f; sigma < 3.0e38f; sigma *= 1.37f) CHECK(refused(plan_with(filter_of(2, 1, sigma)), "radius_y gives a box radius above 63"));
  CHECK(refused(plan_with(filter_of(3, 2.0f, 2.5f, 150, 3)), "who: frame 2: filter: an unsharp mask has one radius (radius_x must equal radius_y)"));
  sjpeg_hip_pillow_filter res = filter_of(0, 0, 0); res.reserved[3] = 1;
  CHECK(refused(plan_with(res), "who: frame 2: filter: reserved must be 0"));
  CHECK(refused(plan_with(filter_of(7, 1, 1), 0), "who: filter: kind 7"));                    // (one for the call: no frame to name)
  CHECK(plan_with(filter_of(1, 63.99f, 63.0f)) == 0 && plan_with(filter_of(2, 63.0f, 0.0f)) == 0 && plan_with(filter_of(3, 0.0f, 0.0f, 65535, 255)) == 0);
  const sjpeg_hip_pillow_filter ok = filter_of(2, 1, 1);
  CHECK(refused(pillow_filter_plan("who", SJPEG_HIP_SRC_YUV420, 3, b.frames.data(), b.buf.get(), &ok, 0, &plan), "who: filter: made pictures of format"));
  CHECK(refused(pillow_filter_plan("who", SJPEG_HIP_SRC_RGBA, 3, b.frames.data(), b.buf.get(), &ok, 0, &plan), "are not filtered (RGB and gray ones are)"));
  std::vector<sjpeg_hip_ragged_frame> bad = b.frames;
  bad[1].row_stride[0] = 26;
  CHECK(refused(pillow_filter_plan("who", SJPEG_HIP_SRC_RGB, 3, bad.data(), b.buf.get(), &ok, 0, &plan), "who: frame 1: filter: the made picture is not rows of whole dwords"));
  bad = b.frames; bad[0].plane[0] = (const uint8_t*)bad[0].plane[0] + 2;
  CHECK(refused(pillow_filter_plan("who", SJPEG_HIP_SRC_RGB, 3, bad.data(), b.buf.get(), &ok, 0, &plan), "who: frame 0: filter: the made picture is not rows"));
  // all-none: NULL, kind 0 everywhere; a reserved byte makes a filter something to refuse, not nothing
  std::vector<sjpeg_hip_pillow_filter> none(3, filter_of(0, 5, 5));
  CHECK(pillow_filter_all_none(3, nullptr, 0) && pillow_filter_all_none(3, none.data(), 1) && pillow_filter_all_none(3, none.data(), 0));
  none[2] = ok; CHECK(!pillow_filter_all_none(3, none.data(), 1) && pillow_filter_all_none(3, none.data(), 0));
  none[2] = res; CHECK(!pillow_filter_all_none(3, none.data(), 1));
  // the host entry
  uint32_t r, ww, fw, passes;
  CHECK(sjpeg_hip_pillow_filter_weights(2, 2.0f, &r, &ww, &fw, &passes) == 0 && r == 1 && passes == 3 && ww == (uint32_t)(16777216.0f / 3.75f));
  CHECK(refused(sjpeg_hip_pillow_filter_weights(1, 64.0f, &r, &ww, &fw, &passes), "sjpeg_hip_pillow_filter_weights: radius gives a box radius above 63"));
  CHECK(refused(sjpeg_hip_pillow_filter_weights(0, 1.0f, &r, &ww, &fw, &passes), "kind 0 is not one of 1..3"));
  CHECK(refused(sjpeg_hip_pillow_filter_weights(1, 1.0f, nullptr, &ww, &fw, &passes), "== NULL"));
  return 0;
}

#ifndef PILLOW_FILTER_NO_MAIN
int main() {
  if (plan_tests() != 0) return 1;
  printf("pillow filter plan ok\n");
  return 0;
}
#endif
