// The host half of the compose stage (sjpeg_amd/csrc/compose_plan.cc) alone, under AddressSanitizer and
// UndefinedBehaviorSanitizer: tests/test_compose_cxx.py builds this file with it by the host compiler.  Every refusal
// comes back as SJPEG_HIP_EINVAL with its words and the number of the frame, overlay or place; the plan's descriptors --
// the canvases' layout, the places resolved from their anchors, places wholly outside dropped -- and the tile counts
// are held to made pictures laid out as the resample plans lay them out.  compose_kernel_emul.cc includes this file for
// its pictures and its expectation: the definition of sjpeg_hip.h, written here sample by sample.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "../../sjpeg_amd/csrc/compose_math.h"
#include "../../sjpeg_amd/csrc/ragged_aux.h"
#include "sjpeg_hip.h"

static std::string g_error;
namespace sjpeg_internal {
int set_error(int code, const std::string& msg) { g_error = msg; return code; }
}  // namespace sjpeg_internal

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #c, g_error.c_str()); return 1; } } while (0)
#define REFUSED(call, words) do { g_error.clear(); CHECK((call) == SJPEG_HIP_EINVAL); CHECK(g_error.find(words) != std::string::npos); } while (0)

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

// an overlay of w x h pixels in a heap buffer of exactly its rows, `extra` bytes of stride beyond 4 * w; alpha: 0 all
// 0, 1 all 255, else random
struct OverlayBuf {
  std::unique_ptr<uint32_t[]> buf;
  sjpeg_hip_overlay o;
};
static OverlayBuf make_overlay(int w, int h, int extra, int alpha, unsigned seed) {
  OverlayBuf v;
  const size_t stride = (size_t)4 * w + extra, bytes = stride * (h - 1) + (size_t)4 * w;
  v.buf.reset(new uint32_t[bytes / 4]);
  uint8_t* p = reinterpret_cast<uint8_t*>(v.buf.get());
  for (size_t i = 0; i < bytes; ++i) { seed = seed * 1664525u + 1013904223u; p[i] = (uint8_t)(seed >> 24); }
  for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) {
    if (alpha == 0) p[y * stride + 4 * x + 3] = 0;
    if (alpha == 1) p[y * stride + 4 * x + 3] = 255;
  }
  v.o.rgba = p; v.o.width = w; v.o.height = h; v.o.stride = (int64_t)stride;
  return v;
}

static sjpeg_hip_compose compose_at(int cw, int ch, int px, int py, int first = 0, int n = 0, int r = 10, int g = 200, int b = 90) {
  sjpeg_hip_compose c;
  memset(&c, 0, sizeof(c));
  c.canvas_width = cw; c.canvas_height = ch; c.px = px; c.py = py; c.first_place = first; c.nplaces = n;
  c.colour[0] = (uint8_t)r; c.colour[1] = (uint8_t)g; c.colour[2] = (uint8_t)b;
  return c;
}
static sjpeg_hip_compose compose_centred(int cw, int ch, double cx, double cy, int first = 0, int n = 0) {
  sjpeg_hip_compose c = compose_at(cw, ch, 0, 0, first, n);
  c.mode = 1; c.cx = cx; c.cy = cy;
  return c;
}
static sjpeg_hip_overlay_place place_of(int overlay, int x, int y, int anchor) {
  sjpeg_hip_overlay_place p;
  memset(&p, 0, sizeof(p));
  p.overlay = overlay; p.x = x; p.y = y; p.anchor = (uint8_t)anchor;
  return p;
}

// ---- the expectation: the canvas of one frame, sample by sample, by sjpeg_hip.h's words (c bytes a pixel, tight rows)
static std::vector<uint8_t> expect_compose(const uint8_t* pic, size_t pic_stride, int w, int h, int c, const sjpeg_hip_compose& s,
                                           const sjpeg_hip_overlay* overlays, const sjpeg_hip_overlay_place* places, int* cw_out, int* ch_out) {
  const bool own = s.canvas_width == 0 && s.canvas_height == 0;
  const int cw = own ? w : s.canvas_width, ch = own ? h : s.canvas_height;
  long long px = s.px, py = s.py;
  if (s.mode == 1) { px = compose_pad_offset(cw, w, s.cx); py = compose_pad_offset(ch, h, s.cy); }
  std::vector<uint8_t> out((size_t)cw * ch * c);
  for (int y = 0; y < ch; ++y) for (int x = 0; x < cw; ++x) for (int k = 0; k < c; ++k) {
    const bool in = x >= px && x < px + w && y >= py && y < py + h;
    out[((size_t)y * cw + x) * c + k] = in ? pic[(size_t)(y - py) * pic_stride + (size_t)(x - px) * c + k] : s.colour[c == 3 ? k : 0];
  }
  for (int i = 0; i < s.nplaces; ++i) {
    const sjpeg_hip_overlay_place& p = places[s.first_place + i];
    const sjpeg_hip_overlay& v = overlays[p.overlay];
    long long ox, oy;
    compose_anchor(p.anchor, cw, ch, v.width, v.height, p.x, p.y, &ox, &oy);
    for (int y = 0; y < v.height; ++y) for (int x = 0; x < v.width; ++x) {
      const long long X = ox + x, Y = oy + y;
      if (X < 0 || Y < 0 || X >= cw || Y >= ch) continue;
      const uint8_t* t = static_cast<const uint8_t*>(v.rgba) + (size_t)y * v.stride + 4 * (size_t)x;
      for (int k = 0; k < c; ++k) {
        uint8_t& d = out[((size_t)Y * cw + X) * c + k];
        const uint32_t src = c == 3 ? t[k] : compose_luma(t[0], t[1], t[2]);
        d = (uint8_t)((d * (255 - t[3]) + src * t[3] + 127) / 255);       // (the other statement of the blend)
      }
    }
  }
  *cw_out = cw; *ch_out = ch;
  return out;
}

static int plan_tests() {
  // ---- layout, places and tiles
  const std::vector<Picture> pics = {{5, 3}, {1, 1}, {300, 20}, {7, 7}};
  Batch made = make_batch(SJPEG_HIP_SRC_RGB, pics, 7u);
  OverlayBuf a = make_overlay(4, 2, 0, 2, 3u), b = make_overlay(3, 5, 8, 2, 4u);
  const sjpeg_hip_overlay overlays[2] = {a.o, b.o};
  const sjpeg_hip_overlay_place places[] = {place_of(0, 1, 1, 0), place_of(0, 1, 1, 1), place_of(1, 1, 1, 2), place_of(1, 2, 1, 3), place_of(0, 1, -1, 4),
                                            place_of(0, 100, 0, 0), place_of(1, -3, 0, 1)};
  const sjpeg_hip_compose compose[4] = {compose_at(9, 7, 2, 3, 0, 5), compose_at(0, 0, 0, 0), compose_centred(301, 40, 0.5, 0.5, 5, 2),
                                        compose_at(7, 7, 0, 0)};
  ComposePlan plan;
  CHECK(compose_plan("t", SJPEG_HIP_SRC_RGB, 4, made.frames.data(), made.buf.get(), compose, 1, overlays, 2, places, 7, &plan) == 0);
  CHECK(plan.frames.size() == 4 && !plan.identity);
  const ComposeFrame& f0 = plan.frames[0];
  CHECK(f0.cw == 9 && f0.ch == 7 && f0.w == 5 && f0.h == 3 && f0.px == 2 && f0.py == 3 && f0.step == 3 && f0.dst_stride == 28 && f0.src_stride == 16);
  CHECK(f0.colour == (10u | 200u << 8 | 90u << 16) && f0.nplaces == 5 && f0.tile_base == 0 && f0.dst == nullptr);
  CHECK(f0.place[0].ox == 1 && f0.place[0].oy == 1 && f0.place[0].ow == 4 && f0.place[0].oh == 2 && f0.place[0].stride == 16);
  CHECK(f0.place[1].ox == 9 - 4 - 1 && f0.place[1].oy == 1);
  CHECK(f0.place[2].ox == 1 && f0.place[2].oy == 7 - 5 - 1 && f0.place[2].stride == 20 && f0.place[2].rgba == b.o.rgba);
  CHECK(f0.place[3].ox == 9 - 3 - 2 && f0.place[3].oy == 7 - 5 - 1);
  CHECK(f0.place[4].ox == (9 - 4) / 2 + 1 && f0.place[4].oy == (7 - 2) / 2 - 1);
  const ComposeFrame& f1 = plan.frames[1];
  CHECK(f1.cw == 1 && f1.ch == 1 && f1.px == 0 && f1.py == 0 && f1.nplaces == 0 && f1.tile_base == 1);
  CHECK(reinterpret_cast<uintptr_t>(f1.dst) == 28 * 7 + 12 && reinterpret_cast<uintptr_t>(f1.made) == 48);
  const ComposeFrame& f2 = plan.frames[2];
  // (301 - 300) * 0.5 = 0.5 rounds to 0, 20 * 0.5 = 10; the place at x = 100 stays, the one 3 beyond the right edge is outside
  CHECK(f2.cw == 301 && f2.ch == 40 && f2.px == 0 && f2.py == 10 && f2.nplaces == 1 && f2.place[0].ox == 100 && f2.tile_base == 2);
  CHECK(f2.dst_stride == 904 && reinterpret_cast<uintptr_t>(f2.dst) == 28 * 7 + 12 + 16);
  // 904 / 4 = 226 dwords: 4 tiles across, 40 rows: 3 down
  CHECK(plan.frames[3].tile_base == 2 + 12 && plan.tiles == 15);
  CHECK(plan.bytes == (size_t)(28 * 7 + 12) + 16 + 904 * 40 + (size_t)align_up(24 * 7, 16));
  std::vector<sjpeg_hip_ragged_frame> out(4);
  std::vector<sjpeg_hip_ragged_frame> src = made.frames;
  src[2].out_offset = 77; src[2].out_capacity = 99;
  compose_plan_frames(plan, src.data(), reinterpret_cast<uint8_t*>(uintptr_t(4096)), out.data());
  CHECK(out[2].width == 301 && out[2].height == 40 && out[2].row_stride[0] == 904 && out[2].out_offset == 77 && out[2].out_capacity == 99);
  CHECK(reinterpret_cast<uintptr_t>(out[2].plane[0]) == 4096 + 28 * 7 + 12 + 16);
  // one struct for the call; identities
  const sjpeg_hip_compose one = compose_centred(400, 400, 0.5, 0.5, 3, 1);
  CHECK(compose_plan("t", SJPEG_HIP_SRC_RGB, 4, made.frames.data(), made.buf.get(), &one, 0, overlays, 2, places, 7, &plan) == 0);
  CHECK(plan.frames[0].px == 198 && plan.frames[0].py == 198 && plan.frames[2].px == 50 && plan.frames[2].py == 190);   // 197.5 -> 198 (even)
  CHECK(plan.frames[3].place[0].ox == 400 - 3 - 2 && plan.frames[3].place[0].oy == 400 - 5 - 1);
  CHECK(compose_plan("t", SJPEG_HIP_SRC_RGB, 4, made.frames.data(), made.buf.get(), nullptr, 0, nullptr, 0, nullptr, 0, &plan) == 0 && plan.identity);
  const sjpeg_hip_compose same = compose_at(7, 7, 0, 0);
  CHECK(compose_plan("t", SJPEG_HIP_SRC_RGB, 1, &made.frames[3], made.buf.get(), &same, 0, nullptr, 0, nullptr, 0, &plan) == 0 && plan.identity);
  CHECK(compose_all_none(4, nullptr, 0) && !compose_all_none(1, &same, 0));
  const sjpeg_hip_compose zero = compose_at(0, 0, 0, 0);
  CHECK(compose_all_none(3, &zero, 0));
  Batch gray = make_batch(SJPEG_HIP_SRC_GRAY, pics, 9u);
  CHECK(compose_plan("t", SJPEG_HIP_SRC_GRAY, 4, gray.frames.data(), gray.buf.get(), compose, 1, overlays, 2, places, 7, &plan) == 0);
  CHECK(plan.frames[0].step == 1 && plan.frames[0].dst_stride == 12 && plan.frames[2].dst_stride == 304);

  // ---- the refusals
#define PLAN(c, per, ov, nov, pl, npl) compose_plan("t", SJPEG_HIP_SRC_RGB, 4, made.frames.data(), made.buf.get(), c, per, ov, nov, pl, npl, &plan)
  sjpeg_hip_compose c = compose_at(0, 5, 0, 0);
  REFUSED(PLAN(&c, 0, nullptr, 0, nullptr, 0), "t: compose: canvas 0x5 is not 0x0");
  c = compose_at(65536, 5, 0, 0);
  REFUSED(PLAN(&c, 0, nullptr, 0, nullptr, 0), "canvas 65536x5");
  c = compose_at(-1, -1, 0, 0);
  REFUSED(PLAN(&c, 0, nullptr, 0, nullptr, 0), "1..65535 a side");
  sjpeg_hip_compose four[4] = {zero, zero, compose_at(300, 20, 1, 0), zero};
  REFUSED(PLAN(four, 1, nullptr, 0, nullptr, 0), "t: frame 2: compose: the 300x20 picture at (1, 0) is not wholly inside the 300x20 canvas");
  four[2] = compose_at(400, 400, 0, -1);
  REFUSED(PLAN(four, 1, nullptr, 0, nullptr, 0), "frame 2: compose: the 300x20 picture at (0, -1)");
  four[2] = compose_centred(299, 400, 0.5, 0.5);
  REFUSED(PLAN(four, 1, nullptr, 0, nullptr, 0), "frame 2: compose: the 300x20 picture is not wholly inside the 299x400 canvas");
  four[2] = zero; four[1] = compose_at(0, 0, 1, 0);
  REFUSED(PLAN(four, 1, nullptr, 0, nullptr, 0), "frame 1: compose: the 1x1 picture at (1, 0) is not wholly inside the 1x1 canvas");
  four[1] = compose_centred(9, 9, NAN, 0.5);
  REFUSED(PLAN(four, 1, nullptr, 0, nullptr, 0), "t: frame 1: compose: the centering is not finite");
  four[1] = compose_centred(9, 9, 0.5, INFINITY);
  REFUSED(PLAN(four, 1, nullptr, 0, nullptr, 0), "the centering is not finite");
  four[1] = zero; four[1].mode = 2;
  REFUSED(PLAN(four, 1, nullptr, 0, nullptr, 0), "frame 1: compose: mode 2 is not 0 (at px, py) or 1 (by the centering)");
  four[1] = zero; four[1].reserved[3] = 1;
  REFUSED(PLAN(four, 1, nullptr, 0, nullptr, 0), "frame 1: compose: reserved must be 0");
  four[1] = compose_at(0, 0, 0, 0, 5, 3);
  REFUSED(PLAN(four, 1, overlays, 2, places, 7), "frame 1: compose: places 5 .. 8 are not within the call's 7 places");
  four[1] = compose_at(0, 0, 0, 0, -1, 1);
  REFUSED(PLAN(four, 1, overlays, 2, places, 7), "are not within the call's 7 places");
  four[1] = zero;
  {
    std::vector<sjpeg_hip_overlay_place> many(9, place_of(0, 0, 0, 0));
    four[3] = compose_at(0, 0, 0, 0, 0, 9);
    REFUSED(PLAN(four, 1, overlays, 2, many.data(), 9), "frame 3: compose: 9 places are more than 8");
    four[3] = compose_at(0, 0, 0, 0, 1, 8);
    CHECK(PLAN(four, 1, overlays, 2, many.data(), 9) == 0 && plan.frames[3].nplaces == 8);
    four[3] = zero;
    many[4].overlay = 2;
    REFUSED(PLAN(four, 1, overlays, 2, many.data(), 9), "t: place 4: overlay 2 is not one of the call's 2 overlays");
    many[4].overlay = -1;
    REFUSED(PLAN(four, 1, overlays, 2, many.data(), 9), "place 4: overlay -1");
    many[4] = place_of(0, 0, 0, 5);
    REFUSED(PLAN(four, 1, overlays, 2, many.data(), 9), "place 4: anchor 5 is not one of 0..4");
    many[4] = place_of(0, 0, 0, 0); many[4].reserved[1] = 7;
    REFUSED(PLAN(four, 1, overlays, 2, many.data(), 9), "place 4: reserved must be 0");
  }
  REFUSED(PLAN(four, 1, nullptr, 2, places, 7), "overlays == NULL");
  REFUSED(PLAN(four, 1, overlays, 2, nullptr, 7), "places == NULL");
  sjpeg_hip_overlay bad[2] = {a.o, b.o};
  bad[1].rgba = nullptr;
  REFUSED(PLAN(four, 1, bad, 2, places, 7), "t: overlay 1: rgba == NULL");
  bad[1].rgba = static_cast<const uint8_t*>(b.o.rgba) + 2;
  REFUSED(PLAN(four, 1, bad, 2, places, 7), "overlay 1: rgba must be a multiple of 4");
  bad[1] = b.o; bad[1].width = 0;
  REFUSED(PLAN(four, 1, bad, 2, places, 7), "overlay 1: width 0 or height 5 is not one of 1..65535");
  bad[1] = b.o; bad[1].height = 65536;
  REFUSED(PLAN(four, 1, bad, 2, places, 7), "height 65536");
  bad[1] = b.o; bad[1].stride = 8;
  REFUSED(PLAN(four, 1, bad, 2, places, 7), "overlay 1: stride 8 is below 4 * width or not a multiple of 4");
  bad[1] = b.o; bad[1].stride = 22;
  REFUSED(PLAN(four, 1, bad, 2, places, 7), "stride 22");
  REFUSED(compose_plan("t", SJPEG_HIP_SRC_YUV420, 4, made.frames.data(), made.buf.get(), compose, 1, overlays, 2, places, 7, &plan),
          "t: compose: made pictures of format " + std::to_string(SJPEG_HIP_SRC_YUV420) + " are not composed (RGB and gray ones are)");
  CHECK(plan.frames.empty() && plan.tiles == 0);
  std::vector<sjpeg_hip_ragged_frame> odd = made.frames;
  odd[1].row_stride[0] = 3;
  REFUSED(compose_plan("t", SJPEG_HIP_SRC_RGB, 4, odd.data(), made.buf.get(), compose, 1, overlays, 2, places, 7, &plan),
          "frame 1: compose: the made picture is not rows of whole dwords");
#undef PLAN

  // ---- the helpers
  int32_t o[2];
  CHECK(sjpeg_hip_contain_size(3, 2, 5, 5, o) == 0 && o[0] == 5 && o[1] == 3);
  CHECK(sjpeg_hip_contain_size(2, 3, 6, 5, o) == 0 && o[0] == 3 && o[1] == 5);
  CHECK(sjpeg_hip_contain_size(5, 5, 6, 1, o) == 0 && o[0] == 1 && o[1] == 1);
  CHECK(sjpeg_hip_contain_size(1920, 1080, 256, 256, o) == 0 && o[0] == 256 && o[1] == 144);
  CHECK(sjpeg_hip_contain_size(4, 2, 8, 4, o) == 0 && o[0] == 8 && o[1] == 4);
  REFUSED(sjpeg_hip_contain_size(1000, 1, 10, 10, o), "has a side of 0");
  REFUSED(sjpeg_hip_contain_size(0, 1, 10, 10, o), "not one of 1..65535");
  REFUSED(sjpeg_hip_contain_size(1, 1, 10, 10, nullptr), "out == NULL");
  CHECK(sjpeg_hip_pad_place(5, 3, 5, 5, 0.5, 0.5, o) == 0 && o[0] == 0 && o[1] == 1);
  CHECK(sjpeg_hip_pad_place(3, 5, 6, 5, 0.5, 0.5, o) == 0 && o[0] == 2 && o[1] == 0);     // 1.5 rounds to 2
  CHECK(sjpeg_hip_pad_place(1, 1, 6, 1, 0.5, 0.5, o) == 0 && o[0] == 2 && o[1] == 0);     // 2.5 rounds to 2
  CHECK(sjpeg_hip_pad_place(256, 144, 256, 256, 0.5, 0.5, o) == 0 && o[0] == 0 && o[1] == 56);
  CHECK(sjpeg_hip_pad_place(1, 1, 11, 11, -3.0, 7.0, o) == 0 && o[0] == 0 && o[1] == 10);  // clamped into 0..1
  REFUSED(sjpeg_hip_pad_place(6, 1, 5, 5, 0.5, 0.5, o), "is not wholly inside");
  REFUSED(sjpeg_hip_pad_place(1, 1, 5, 5, NAN, 0.5, o), "not finite");
  CHECK(sjpeg_hip_compose_sample(0, 255, 0, 0, 128, 0) == 128 && sjpeg_hip_compose_sample(128, 0, 0, 0, 128, 0) == 64);
  CHECK(sjpeg_hip_compose_sample(0, 0, 0, 0, 128, 0) == 0 && sjpeg_hip_compose_sample(0, 255, 255, 255, 255, 1) == 255);
  return 0;
}

#ifndef COMPOSE_NO_MAIN
int main() {
  if (plan_tests() != 0) return 1;
  printf("compose plan ok\n");
  return 0;
}
#endif
