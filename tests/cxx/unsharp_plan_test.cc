// The host half of the unsharp mask (sjpeg_amd/csrc/unsharp_plan.cc) alone, under AddressSanitizer and
// UndefinedBehaviorSanitizer: tests/test_unsharp_cxx.py builds this file with it by the host compiler.  Made pictures of
// the four made formats -- RGB, gray, 4:2:0 with odd sizes, 4:4:4 -- lie in heap buffers of exactly their bytes, laid out
// as the resize plans lay them out; the plan's descriptors are held to them (U and V carry amount 0), and then the
// kernel's rule (unsharp.hip, restated here: the tile, the clamped staging, the window of three dwords, the store) is
// walked workgroup by workgroup over those buffers: every load and store lies inside its buffer, every dword that begins
// inside a row's samples is stored exactly once, nothing else is, and the bytes equal a picture filter written here.
// Bad parameters, formats and layouts come back as SJPEG_HIP_EINVAL.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../sjpeg_amd/csrc/ragged_aux.h"
#include "../../sjpeg_amd/csrc/unsharp_math.h"
#include "sjpeg_hip.h"

static std::string g_error;
namespace sjpeg_internal {
int set_error(int code, const std::string& msg) { g_error = msg; return code; }
}  // namespace sjpeg_internal

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #c, g_error.c_str()); return 1; } } while (0)

using sjpeg_internal::UnsharpPlan;
using sjpeg_internal::UnsharpPlane;
using sjpeg_internal::kUnsharpTileDwords;
using sjpeg_internal::kUnsharpTileRows;

struct Picture { int w, h; };

static size_t align_up(size_t n, size_t a) { return (n + a - 1) / a * a; }

// the made pictures of `format` in one heap buffer of exactly their bytes: every plane at a multiple of 16, rows whole
// dwords apart; frames[] as a plan kind's frames() reports them
struct Batch {
  std::unique_ptr<uint8_t[]> buf;
  size_t bytes = 0;
  std::vector<sjpeg_hip_ragged_frame> frames;
};
static void plane_dims(int format, int w, int h, int c, int* pw, int* ph) {
  const bool half = c > 0 && format == SJPEG_HIP_SRC_YUV420;
  *pw = half ? (w + 1) / 2 : w;
  *ph = half ? (h + 1) / 2 : h;
}
static Batch make_batch(int format, const std::vector<Picture>& pics, unsigned seed) {
  Batch b;
  const int nplanes = format == SJPEG_HIP_SRC_YUV420 || format == SJPEG_HIP_SRC_YUV444 ? 3 : 1;
  const int step = format == SJPEG_HIP_SRC_RGB ? 3 : 1;
  std::vector<size_t> offs;
  for (const Picture& p : pics) for (int c = 0; c < nplanes; ++c) {
    int pw, ph;
    plane_dims(format, p.w, p.h, c, &pw, &ph);
    offs.push_back(b.bytes);
    b.bytes += align_up(align_up(static_cast<size_t>(pw) * step, 4) * ph, 16);
  }
  b.buf.reset(new uint8_t[b.bytes]);
  for (size_t i = 0; i < b.bytes; ++i) { seed = seed * 1664525u + 1013904223u; b.buf[i] = static_cast<uint8_t>(seed >> 24); }
  size_t k = 0;
  for (const Picture& p : pics) {
    sjpeg_hip_ragged_frame f;
    memset(&f, 0, sizeof(f));
    f.width = p.w; f.height = p.h;
    for (int c = 0; c < nplanes; ++c, ++k) {
      int pw, ph;
      plane_dims(format, p.w, p.h, c, &pw, &ph);
      f.plane[c] = b.buf.get() + offs[k];
      f.row_stride[c] = static_cast<int64_t>(align_up(static_cast<size_t>(pw) * step, 4));
    }
    b.frames.push_back(f);
  }
  return b;
}

// the filter on a plane of rows of bytes with a channel step, the edge replicated per channel
static uint8_t filtered(const uint8_t* src, unsigned stride, int wbytes, int rows, int step, int x, int y, int amount, int threshold) {
  uint8_t n[9];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
    int yy = y + i - 1, xx = x + (j - 1) * step;
    yy = yy < 0 ? 0 : yy > rows - 1 ? rows - 1 : yy;
    if (xx < 0 || xx >= wbytes) xx = x;                            // (the nearest sample of the channel inside: this one)
    n[3 * i + j] = src[static_cast<size_t>(yy) * stride + xx];
  }
  return static_cast<uint8_t>(sjpeg_internal::unsharp_sample(n, amount, threshold));
}

struct Walk {
  const uint8_t* src; size_t src_bytes;
  uint8_t* dst; size_t dst_bytes;
  std::vector<uint8_t> stored;                                     // per dst byte: how often
  bool ok = true;
  uint32_t load(size_t at) {
    if (at + 4 > src_bytes || (at & 3) != 0) { ok = false; return 0; }
    uint32_t v; memcpy(&v, src + at, 4); return v;
  }
  void store(size_t at, uint32_t v) {
    if (at + 4 > dst_bytes || (at & 3) != 0) { ok = false; return; }
    memcpy(dst + at, &v, 4);
    for (int b = 0; b < 4; ++b) ++stored[at + b];
  }
};

static int byte_at(const uint32_t w[3], int i) { return static_cast<int>((w[i >> 2] >> (8 * (i & 3))) & 255u); }

// one workgroup of unsharp.hip, lane by lane
static void workgroup(Walk* wk, const std::vector<UnsharpPlane>& planes, unsigned wg) {
  int lo = 0, hi = static_cast<int>(planes.size()) - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (planes[mid].tile_base <= wg) lo = mid; else hi = mid - 1;
  }
  const UnsharpPlane& d = planes[lo];
  const size_t src0 = reinterpret_cast<uintptr_t>(d.src), dst0 = reinterpret_cast<uintptr_t>(d.dst);
  const int TD = static_cast<int>(kUnsharpTileDwords), TR = static_cast<int>(kUnsharpTileRows);
  const unsigned ndw = (d.width_bytes + 3u) / 4u, tiles_x = (ndw + TD - 1) / TD;
  const unsigned t = wg - d.tile_base, ty = t / tiles_x, tx = t - ty * tiles_x;
  const int dw0 = static_cast<int>(tx) * TD, row0 = static_cast<int>(ty) * TR;
  if (static_cast<unsigned>(row0) >= d.rows) { wk->ok = false; return; }      // (the plan's grid has no such workgroup)
  std::vector<uint32_t> stage(static_cast<size_t>(TR + 2) * (TD + 2));
  for (int i = 0; i < (TR + 2) * (TD + 2); ++i) {
    const int r = i / (TD + 2), k = i - r * (TD + 2);
    int y = row0 + r - 1, g = dw0 + k - 1;
    y = y < 0 ? 0 : y > static_cast<int>(d.rows) - 1 ? static_cast<int>(d.rows) - 1 : y;
    g = g < 0 ? 0 : g > static_cast<int>(ndw) - 1 ? static_cast<int>(ndw) - 1 : g;
    stage[i] = wk->load(src0 + static_cast<size_t>(y) * d.src_stride + 4u * g);
  }
  const int step = static_cast<int>(d.step);
  for (int tid = 0; tid < 256; ++tid) {
    const int k = tid & 63, r0 = (tid >> 6) * (TR / 4);
    const unsigned gx = dw0 + k, gy0 = row0 + r0;
    if (gx >= ndw || gy0 >= d.rows) continue;
    for (int j = 0; j < TR / 4 && gy0 + j < d.rows; ++j) {
      uint32_t out = 0;
      for (int b = 0; b < 4; ++b) {
        const unsigned x = 4 * gx + b;
        int h[3], p = 0;
        for (int r = 0; r < 3; ++r) {
          const uint32_t* w = &stage[static_cast<size_t>(r0 + j + r) * (TD + 2) + k];
          const int at = byte_at(w, 4 + b);
          const int left = x >= static_cast<unsigned>(step) ? byte_at(w, 4 + b - step) : at;
          const int right = x + step < d.width_bytes ? byte_at(w, 4 + b + step) : at;
          h[r] = left + 2 * at + right;
          if (r == 1) p = at;
        }
        out |= static_cast<uint32_t>(sjpeg_internal::unsharp_apply(p, sjpeg_internal::unsharp_blur16(h[0], h[1], h[2]), d.amount, d.threshold)) << (8 * b);
      }
      wk->store(dst0 + static_cast<size_t>(gy0 + j) * d.dst_stride + 4u * gx, out);
    }
  }
}

static int check_batch(int format, const std::vector<Picture>& pics, const std::vector<sjpeg_hip_unsharp>& us, int per_frame, long* samples) {
  const Batch b = make_batch(format, pics, 12345u + static_cast<unsigned>(format));
  const int n = static_cast<int>(pics.size());
  const int nplanes = format == SJPEG_HIP_SRC_YUV420 || format == SJPEG_HIP_SRC_YUV444 ? 3 : 1;
  const int step = format == SJPEG_HIP_SRC_RGB ? 3 : 1;
  UnsharpPlan plan;
  CHECK(sjpeg_internal::unsharp_plan("t", format, n, b.frames.data(), b.buf.get(), us.data(), per_frame, &plan) == 0);
  CHECK(plan.planes.size() == static_cast<size_t>(n) * nplanes);
  // ---- the descriptors
  unsigned tiles = 0;
  for (int f = 0; f < n; ++f) for (int c = 0; c < nplanes; ++c) {
    const UnsharpPlane& d = plan.planes[static_cast<size_t>(f) * nplanes + c];
    int pw, ph;
    plane_dims(format, pics[f].w, pics[f].h, c, &pw, &ph);
    const sjpeg_hip_unsharp& u = us[per_frame ? f : 0];
    CHECK(reinterpret_cast<uintptr_t>(d.src) == static_cast<size_t>(static_cast<const uint8_t*>(b.frames[f].plane[c]) - b.buf.get()));
    CHECK(reinterpret_cast<uintptr_t>(d.dst) == reinterpret_cast<uintptr_t>(d.src) && (reinterpret_cast<uintptr_t>(d.src) & 15u) == 0);
    CHECK(d.width_bytes == static_cast<unsigned>(pw * step) && d.rows == static_cast<unsigned>(ph) && d.step == static_cast<unsigned>(step));
    CHECK(d.src_stride == static_cast<unsigned>(b.frames[f].row_stride[c]) && d.dst_stride == d.src_stride);
    CHECK(d.amount == (c == 0 ? u.amount : 0u) && d.threshold == (c == 0 ? u.threshold : 0u));
    CHECK(d.tile_base == tiles);
    tiles += ((d.width_bytes + 3) / 4 + kUnsharpTileDwords - 1) / kUnsharpTileDwords * ((d.rows + kUnsharpTileRows - 1) / kUnsharpTileRows);
  }
  CHECK(plan.tiles == tiles && tiles >= static_cast<unsigned>(n * nplanes));
  // ---- the kernel's rule over heap buffers of exactly the pictures' bytes
  std::unique_ptr<uint8_t[]> out(new uint8_t[b.bytes]);
  memset(out.get(), 0xA5, b.bytes);
  Walk wk{b.buf.get(), b.bytes, out.get(), b.bytes, std::vector<uint8_t>(b.bytes, 0)};
  for (unsigned wg = 0; wg < plan.tiles; ++wg) workgroup(&wk, plan.planes, wg);
  CHECK(wk.ok);
  std::vector<uint8_t> want(b.bytes, 0);                           // per byte: stored once (1) or never (0)
  for (const UnsharpPlane& d : plan.planes) {
    const size_t at = reinterpret_cast<uintptr_t>(d.src);
    for (unsigned y = 0; y < d.rows; ++y) {
      for (unsigned x = 0; x < ((d.width_bytes + 3) & ~3u); ++x) want[at + static_cast<size_t>(y) * d.dst_stride + x] = 1;
      for (unsigned x = 0; x < d.width_bytes; ++x) {
        const uint8_t w = filtered(b.buf.get() + at, d.src_stride, static_cast<int>(d.width_bytes), static_cast<int>(d.rows), static_cast<int>(d.step),
                                   static_cast<int>(x), static_cast<int>(y), static_cast<int>(d.amount), static_cast<int>(d.threshold));
        CHECK(out[at + static_cast<size_t>(y) * d.dst_stride + x] == w);
        if (d.amount == 0) CHECK(w == b.buf[at + static_cast<size_t>(y) * d.src_stride + x]);
        ++*samples;
      }
    }
  }
  CHECK(wk.stored == want);
  for (size_t i = 0; i < b.bytes; ++i) if (want[i] == 0) CHECK(out[i] == 0xA5);
  return 0;
}

int main() {
  long samples = 0;
  // sizes one under, at and one over the tile each way (64 dwords: 256 gray bytes, 85.33 RGB pixels; 16 rows), the
  // smallest ones, and row lengths of every residue mod 4
  const std::vector<Picture> gray = {{1, 1}, {2, 1}, {1, 2}, {3, 3}, {5, 7}, {255, 15}, {256, 16}, {257, 17}, {513, 33}, {7, 3}},
                             rgb = {{1, 1}, {2, 1}, {1, 2}, {3, 3}, {5, 7}, {85, 15}, {86, 16}, {171, 17}, {172, 33}, {7, 3}},
                             yuv = {{1, 1}, {5, 7}, {2, 1}, {513, 33}, {511, 31}, {64, 17}};
  auto params = [](size_t n) {
    std::vector<sjpeg_hip_unsharp> us;
    for (size_t k = 0; k < n; ++k) us.push_back(sjpeg_hip_unsharp{static_cast<uint8_t>(k % 3 == 2 ? 255 : 32 * (k % 5)), static_cast<uint8_t>(k % 4 == 3 ? 9 : 0), {0, 0}});
    return us;
  };
  if (check_batch(SJPEG_HIP_SRC_GRAY, gray, params(gray.size()), 1, &samples)) return 1;
  if (check_batch(SJPEG_HIP_SRC_RGB, rgb, params(rgb.size()), 1, &samples)) return 1;
  if (check_batch(SJPEG_HIP_SRC_YUV420, yuv, params(yuv.size()), 1, &samples)) return 1;
  if (check_batch(SJPEG_HIP_SRC_YUV444, yuv, params(yuv.size()), 1, &samples)) return 1;
  if (check_batch(SJPEG_HIP_SRC_RGB, rgb, {sjpeg_hip_unsharp{64, 3, {0, 0}}}, 0, &samples)) return 1;
  if (check_batch(SJPEG_HIP_SRC_YUV420, yuv, {sjpeg_hip_unsharp{255, 0, {0, 0}}}, 0, &samples)) return 1;
  // ---- refusals
  {
    const Batch b = make_batch(SJPEG_HIP_SRC_GRAY, {{5, 7}, {9, 2}}, 3u);
    UnsharpPlan plan;
    sjpeg_hip_unsharp us[2] = {{32, 0, {0, 0}}, {32, 0, {0, 1}}};
    CHECK(sjpeg_internal::unsharp_plan("who", SJPEG_HIP_SRC_GRAY, 2, b.frames.data(), b.buf.get(), us, 1, &plan) == SJPEG_HIP_EINVAL);
    CHECK(g_error == "who: frame 1: unsharp: reserved must be 0" && plan.planes.empty() && plan.tiles == 0);
    CHECK(sjpeg_internal::unsharp_plan("who", SJPEG_HIP_SRC_GRAY, 2, b.frames.data(), b.buf.get(), us + 1, 0, &plan) == SJPEG_HIP_EINVAL);
    CHECK(g_error == "who: unsharp: reserved must be 0");
    CHECK(sjpeg_internal::unsharp_plan("who", SJPEG_HIP_SRC_GRAY, 2, b.frames.data(), b.buf.get(), us, 0, &plan) == 0 && plan.planes.size() == 2);
    CHECK(sjpeg_internal::unsharp_plan("who", SJPEG_HIP_SRC_GRAY, 2, b.frames.data(), b.buf.get(), nullptr, 0, &plan) == 0 && plan.planes[0].amount == 0);
    CHECK(sjpeg_internal::unsharp_plan("who", SJPEG_HIP_SRC_NV12, 2, b.frames.data(), b.buf.get(), us, 0, &plan) == SJPEG_HIP_EINVAL);
    CHECK(sjpeg_internal::unsharp_plan("who", SJPEG_HIP_SRC_BGRA, 2, b.frames.data(), b.buf.get(), us, 0, &plan) == SJPEG_HIP_EINVAL);
    std::vector<sjpeg_hip_ragged_frame> bad = b.frames;
    bad[1].row_stride[0] = 8;                                      // (9 samples a row)
    CHECK(sjpeg_internal::unsharp_plan("who", SJPEG_HIP_SRC_GRAY, 2, bad.data(), b.buf.get(), us, 0, &plan) == SJPEG_HIP_EINVAL);
    CHECK(g_error.find("who: frame 1: unsharp: plane 0") == 0);
    bad = b.frames;
    bad[0].plane[0] = b.buf.get() + 2;
    CHECK(sjpeg_internal::unsharp_plan("who", SJPEG_HIP_SRC_GRAY, 2, bad.data(), b.buf.get(), us, 0, &plan) == SJPEG_HIP_EINVAL);
    CHECK(sjpeg_internal::unsharp_all_zero(2, nullptr, 1) && !sjpeg_internal::unsharp_all_zero(2, us, 1));
    sjpeg_hip_unsharp zero[2] = {{0, 7, {0, 0}}, {0, 0, {0, 0}}};
    CHECK(sjpeg_internal::unsharp_all_zero(2, zero, 1) && sjpeg_internal::unsharp_all_zero(2, zero, 0));
    zero[1].amount = 1;
    CHECK(!sjpeg_internal::unsharp_all_zero(2, zero, 1) && sjpeg_internal::unsharp_all_zero(2, zero, 0));
    uint32_t byte = 9;
    const uint8_t n9[9] = {10, 10, 10, 10, 11, 10, 10, 10, 10};
    CHECK(sjpeg_hip_unsharp_sample(22, 0, n9, &byte) == 0 && byte == 12);
    CHECK(sjpeg_hip_unsharp_sample(256, 0, n9, &byte) == SJPEG_HIP_EINVAL && sjpeg_hip_unsharp_sample(1, -1, n9, &byte) == SJPEG_HIP_EINVAL);
    CHECK(sjpeg_hip_unsharp_sample(1, 1, nullptr, &byte) == SJPEG_HIP_EINVAL && sjpeg_hip_unsharp_sample(1, 1, n9, nullptr) == SJPEG_HIP_EINVAL && byte == 12);
  }
  printf("unsharp plan ok: %ld samples\n", samples);
  return 0;
}
