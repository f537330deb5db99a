// The arithmetic of the unsharp mask (sjpeg_amd/csrc/unsharp_math.h) on the host, under UndefinedBehaviorSanitizer:
// tests/test_unsharp_cxx.py builds this file by the host compiler.  The header's formula is held to a restatement in
// 64-bit integers with a true floor division, for every p and S at a set of amounts and thresholds; amount 0 is the
// identity for every p, S and threshold; the clamp at both ends; the threshold's edge; and the issue's known answers
// on whole pictures, through a picture filter written here with the edge replicated.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../sjpeg_amd/csrc/unsharp_math.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

using sjpeg_internal::unsharp_apply;
using sjpeg_internal::unsharp_sample;

static int64_t floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0 && (a < 0) != (b < 0)) ? 1 : 0); }

static int model(int p, int S, int amount, int threshold) {
  const int64_t D = 16ll * p - S;
  if ((D < 0 ? -D : D) < 16ll * threshold) return p;
  const int64_t v = floor_div(512ll * p + static_cast<int64_t>(amount) * D + 256, 512);
  return static_cast<int>(v < 0 ? 0 : v > 255 ? 255 : v);
}

// a picture of `step` interleaved channels, w pixels x h rows, tightly packed; the edge replicated per channel
static std::vector<uint8_t> filter(const std::vector<uint8_t>& im, int w, int h, int step, int amount, int threshold) {
  std::vector<uint8_t> out(im.size());
  auto at = [&](int x, int y, int c) {
    x = x < 0 ? 0 : x > w - 1 ? w - 1 : x;
    y = y < 0 ? 0 : y > h - 1 ? h - 1 : y;
    return im[(static_cast<size_t>(y) * w + x) * step + c];
  };
  for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) for (int c = 0; c < step; ++c) {
    uint8_t n[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) n[3 * i + j] = at(x + j - 1, y + i - 1, c);
    out[(static_cast<size_t>(y) * w + x) * step + c] = static_cast<uint8_t>(unsharp_sample(n, amount, threshold));
  }
  return out;
}

int main() {
  // ---- the formula against the restatement: every p and S the weights allow (S holds 4 p), and every S at all
  const int amounts[] = {0, 1, 31, 32, 33, 64, 128, 254, 255}, thresholds[] = {0, 1, 25, 26, 100, 254, 255};
  long checked = 0;
  for (int amount : amounts) for (int threshold : thresholds) for (int p = 0; p < 256; ++p) for (int S = 0; S <= 4080; ++S) {
    CHECK(unsharp_apply(p, S, amount, threshold) == model(p, S, amount, threshold));
    ++checked;
  }
  // ---- amount 0 is the identity, exhaustively
  for (int threshold = 0; threshold < 256; ++threshold) for (int p = 0; p < 256; ++p) for (int S = 0; S <= 4080; ++S) {
    CHECK(unsharp_apply(p, S, 0, threshold) == p);
    ++checked;
  }
  // ---- threshold 255 is the identity for every neighbourhood sum that holds 4 p
  for (int amount = 0; amount < 256; ++amount) for (int p = 0; p < 256; ++p) for (int S = 4 * p; S <= 4 * p + 12 * 255; ++S) {
    CHECK(unsharp_apply(p, S, amount, 255) == p);
  }
  // ---- the clamp at both ends, amount 255: p = 0 among 255s, p = 255 among 0s, and the unclamped values beside them
  {
    uint8_t lo[9] = {255, 255, 255, 255, 0, 255, 255, 255, 255}, hi[9] = {0, 0, 0, 0, 255, 0, 0, 0, 0};
    CHECK(unsharp_sample(lo, 255, 0) == 0 && unsharp_sample(hi, 255, 0) == 255);
    CHECK(model(0, 12 * 255, 255, 0) == 0 && model(255, 4 * 255, 255, 0) == 255);
    CHECK(floor_div(512 * 0 + 255 * (0 - 3060) + 256, 512) == -1524 && floor_div(512 * 255 + 255 * 3060 + 256, 512) == 1779);
    uint8_t flat[9] = {7, 7, 7, 7, 7, 7, 7, 7, 7};
    CHECK(unsharp_sample(flat, 255, 0) == 7);
    // (one level of contrast: 512 p + amount D + 256 crosses a multiple of 512 exactly where it should)
    uint8_t one[9] = {10, 10, 10, 10, 11, 10, 10, 10, 10};          // D = 12
    CHECK(unsharp_sample(one, 32, 0) == 12 && unsharp_sample(one, 255, 0) == 17 && unsharp_sample(one, 21, 0) == 11 &&
          unsharp_sample(one, 22, 0) == 12);                        // (22 * 12 + 256 = 520 >= 512)
  }
  // ---- |D| == 16 * threshold is sharpened, one below is not
  for (int threshold = 1; threshold < 192; ++threshold) {
    const int p = 200, D = 16 * threshold;
    if (16 * p - D < 4 * p) break;
    CHECK(unsharp_apply(p, 16 * p - D, 32, threshold) == model(p, 16 * p - D, 32, 0));
    CHECK(unsharp_apply(p, 16 * p - D, 32, threshold) != p || (32 * D + 256) / 512 == 0);
    CHECK(unsharp_apply(p, 16 * p - D + 1, 32, threshold) == p);
    CHECK(unsharp_apply(55, 16 * 55 + D, 32, threshold) == model(55, 16 * 55 + D, 32, 0) && unsharp_apply(55, 16 * 55 + D - 1, 32, threshold) == 55);
  }
  // ---- the known answers
  {
    std::vector<uint8_t> rows;
    for (int y = 0; y < 5; ++y) for (int x = 0; x < 8; ++x) rows.push_back(x < 4 ? 100 : 200);
    const uint8_t want32[8] = {100, 100, 100, 75, 225, 200, 200, 200}, want64[8] = {100, 100, 100, 50, 250, 200, 200, 200};
    const std::vector<uint8_t> a = filter(rows, 8, 5, 1, 32, 0), b = filter(rows, 8, 5, 1, 64, 0);
    for (int y = 0; y < 5; ++y) for (int x = 0; x < 8; ++x) CHECK(a[y * 8 + x] == want32[x] && b[y * 8 + x] == want64[x]);
    CHECK(filter(rows, 8, 5, 1, 32, 26) == rows && filter(rows, 8, 5, 1, 32, 25) == a);
    CHECK(filter({10, 12}, 2, 1, 1, 32, 0) == (std::vector<uint8_t>{10, 13}));
    std::vector<uint8_t> board;
    for (int y = 0; y < 4; ++y) for (int x = 0; x < 4; ++x) board.push_back((x + y) % 2 == 0 ? 100 : 200);
    const std::vector<uint8_t> c = filter(board, 4, 4, 1, 32, 0);
    CHECK(c[0] == 63 && c[1] == 250 && c[2] == 50 && c[3] == 238);
    // a constant picture and a 1 x 1 picture come back unchanged; three interleaved channels filter each on its own
    CHECK(filter(std::vector<uint8_t>(35, 91), 7, 5, 1, 255, 0) == std::vector<uint8_t>(35, 91));
    CHECK(filter({201}, 1, 1, 1, 255, 0) == std::vector<uint8_t>{201} && filter({1, 2, 3}, 1, 1, 3, 255, 0) == (std::vector<uint8_t>{1, 2, 3}));
    std::vector<uint8_t> rgb;
    for (int y = 0; y < 5; ++y) for (int x = 0; x < 8; ++x) { rgb.push_back(x < 4 ? 100 : 200); rgb.push_back(77); rgb.push_back(x < 4 ? 200 : 100); }
    const std::vector<uint8_t> d = filter(rgb, 8, 5, 3, 32, 0);
    for (int x = 0; x < 8; ++x) CHECK(d[3 * x] == want32[x] && d[3 * x + 1] == 77 && d[3 * x + 2] == 300 - want32[x]);
  }
  printf("unsharp math ok: %ld samples\n", checked);
  return 0;
}
