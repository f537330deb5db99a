// The arithmetic of resampling with Pillow's filters (sjpeg_amd/csrc/resample_math.h) and the host entries over it,
// under AddressSanitizer and UndefinedBehaviorSanitizer: tests/test_resample_cxx.py builds this file by the host compiler
// and hands it the tables recorded in tests/golden/resample_pillow.npz as a file of int32 (argv[1]: per table filter,
// in, out, ksize, then out * 2 bounds and out * ksize coefficients).  sjpeg_hip_resample_table must equal every one of
// them; the two bounds the kernel relies on must hold over the grid sjpeg_hip.h names, with the maxima it states; the
// known answers of the header, the identity table and both clips are walked.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../sjpeg_amd/csrc/resample_math.h"
#include "sjpeg_hip.h"

static std::string g_error;
namespace sjpeg_internal {
int set_error(int code, const std::string& msg) { g_error = msg; return code; }
}  // namespace sjpeg_internal

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #c, g_error.c_str()); return 1; } } while (0)

using namespace sjpeg_internal;

static std::vector<uint8_t> axis(const std::vector<uint8_t>& row, int out, int filter) {
  std::vector<int32_t> b, K;
  const int in = static_cast<int>(row.size());
  resample_table(filter, in, out, &b, &K);
  const size_t ks = static_cast<size_t>(resample_ksize(filter, in, out));
  std::vector<uint8_t> o(out);
  for (int x = 0; x < out; ++x) o[x] = static_cast<uint8_t>(resample_sample(&K[x * ks], &row[b[2 * x]], b[2 * x + 1]));
  return o;
}

int main(int argc, char** argv) {
  // ---- the recorded tables
  CHECK(argc == 2);
  FILE* f = fopen(argv[1], "rb");
  CHECK(f != nullptr);
  int ntables = 0;
  long long coefficients = 0;
  int32_t head[4];
  while (fread(head, sizeof(int32_t), 4, f) == 4) {
    const int filter = head[0], in = head[1], out = head[2], ks = head[3];
    CHECK(sjpeg_hip_resample_ksize(filter, in, out) == ks);
    std::vector<int32_t> wb(2 * static_cast<size_t>(out)), wK(static_cast<size_t>(out) * ks), b(wb.size()), K(wK.size());
    CHECK(fread(wb.data(), sizeof(int32_t), wb.size(), f) == wb.size() && fread(wK.data(), sizeof(int32_t), wK.size(), f) == wK.size());
    CHECK(sjpeg_hip_resample_table(filter, in, out, reinterpret_cast<int32_t (*)[2]>(b.data()), K.data(), K.size()) == 0);
    if (b != wb || K != wK) { printf("FAILED: table filter %d, %d -> %d differs from the recorded one\n", filter, in, out); return 1; }
    ++ntables;
    coefficients += static_cast<long long>(K.size());
  }
  fclose(f);
  CHECK(ntables >= 30);

  // ---- the two bounds over the grid of sjpeg_hip.h, and the maxima it states
  std::vector<int> ins, outs;
  for (int v = 1; v <= 69; ++v) { ins.push_back(v); outs.push_back(v); }
  for (int v : {100, 257, 1000, 1920, 3840}) ins.push_back(v);
  for (int v : {100, 180, 320, 1000, 4000}) outs.push_back(v);
  int64_t max_k = 0, max_sum = 0;
  long long tables = 0;
  std::vector<int32_t> b, K;
  for (int filter = 0; filter < kResampleFilters; ++filter) for (int in : ins) for (int out : outs) {
    resample_table(filter, in, out, &b, &K);
    const size_t ks = static_cast<size_t>(resample_ksize(filter, in, out));
    CHECK(K.size() == ks * out && b.size() == 2u * out);
    if (!resample_table_fits(K.data(), K.size()) || !resample_sums_fit(K.data(), out, ks)) {
      printf("FAILED: filter %d, %d -> %d breaks a bound\n", filter, in, out);
      return 1;
    }
    for (int x = 0; x < out; ++x) {
      int64_t pos = 0, neg = 0;
      CHECK(b[2 * x] >= 0 && b[2 * x + 1] >= 1 && b[2 * x] + b[2 * x + 1] <= in && static_cast<size_t>(b[2 * x + 1]) <= ks);
      for (size_t t = 0; t < ks; ++t) {
        const int64_t k = K[x * ks + t];
        CHECK(t < static_cast<size_t>(b[2 * x + 1]) || k == 0);
        if (k > 0) pos += k; else neg -= k;
        if (k > max_k) max_k = k;
        if (-k > max_k) max_k = -k;
      }
      const int64_t s = kResampleHalf + 255 * (pos > neg ? pos : neg);
      if (s > max_sum) max_sum = s;
    }
    ++tables;
  }
  printf("grid: %lld tables, max |K| %lld, max sum %lld\n", tables, static_cast<long long>(max_k), static_cast<long long>(max_sum));
  CHECK(max_k == 5392348 && max_sum == 1377229532);
  // a table that breaks a bound is found: 2^23, and a row whose positive coefficients sum past 2^31 / 255
  const int32_t wide[2] = {1 << 23, 0}, heavy[3] = {4194304, 4194304, 200000};
  CHECK(!resample_table_fits(wide, 2) && resample_table_fits(heavy, 3));
  CHECK(resample_sums_fit(heavy, 1, 2) && !resample_sums_fit(heavy, 1, 3));

  // ---- the known answers of sjpeg_hip.h
  const std::vector<uint8_t> up = {0, 255}, down = {10, 20, 30, 40, 250, 240, 230, 220};
  const uint8_t want_up[5][4] = {{0, 0, 255, 255}, {0, 64, 191, 255}, {0, 19, 236, 255}, {0, 53, 202, 255}, {0, 59, 196, 255}};
  const uint8_t want_down[5][2] = {{25, 235}, {57, 207}, {38, 224}, {47, 217}, {46, 220}};
  for (int filter = 0; filter < 5; ++filter) {
    CHECK(axis(up, 4, filter) == std::vector<uint8_t>(want_up[filter], want_up[filter] + 4));
    CHECK(axis(down, 2, filter) == std::vector<uint8_t>(want_down[filter], want_down[filter] + 2));
  }
  resample_table(kResampleBilinear, 7, 3, &b, &K);
  CHECK((b == std::vector<int32_t>{0, 4, 1, 5, 4, 3}));
  CHECK((std::vector<int32_t>(K.begin() + 7, K.begin() + 14) == std::vector<int32_t>{246724, 986895, 1727066, 986895, 246724, 0, 0}));
  // the identity table gives every byte back; the clips; the arithmetic shift of a negative sum
  resample_identity_table(4, &b, &K);
  for (int v = 0; v < 256; ++v) { const uint8_t s = static_cast<uint8_t>(v); CHECK(resample_sample(&K[2], &s, 1) == v); }
  CHECK(b[4] == 2 && b[5] == 1);
  CHECK(resample_clip(-1) == 0 && resample_clip(-(1 << 22)) == 0 && resample_clip((1 << 22) - 1) == 0 && resample_clip(1 << 22) == 1);
  CHECK(resample_clip(255 * (1 << 22) + 5) == 255 && resample_clip(256 * (1 << 22)) == 255 && resample_clip(0x7fffffff) == 255);
  CHECK(resample_mac(kResampleHalf, -(1 << 22), 255) == kResampleHalf - 255 * (1 << 22));
  printf("resample math ok: %d recorded tables, %lld coefficients\n", ntables, coefficients);
  return 0;
}
