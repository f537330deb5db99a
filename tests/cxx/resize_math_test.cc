// The arithmetic of the ragged resize (sjpeg_amd/csrc/resize_math.h) on the host: the kernel reads the same text.
// The cells of an axis -- their weights, first indices and counts -- for every pair of lengths up to 70 and for the
// longest axis, and the rounding against the plain 64-bit division at every quotient's two edges.  Stand-alone, host
// compiler only.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "resize_math.h"

using namespace sjpeg_internal;

static long cells = 0, roundings = 0;

// every cell of an axis of n_src samples made n_dst long
static bool check_axis(uint32_t n_src, uint32_t n_dst) {
  const uint32_t most = (n_src + n_dst - 1) / n_dst + 1;
  uint32_t end = 0;                                  // one past the last index of the cell before
  for (uint32_t xo = 0; xo < n_dst; ++xo) {
    const uint32_t first = resize_first(xo, n_src, n_dst), count = resize_count(xo, n_src, n_dst);
    if (count < 1 || count > most || first + count > n_src) { printf("%u -> %u: cell %u has %u indices from %u\n", n_src, n_dst, xo, count, first); return false; }
    // contiguous: a cell starts where the one before ended, or on its last index
    if (xo == 0 ? first != 0 : (first != end && first + 1 != end)) { printf("%u -> %u: cell %u starts at %u, the one before ended at %u\n", n_src, n_dst, xo, first, end); return false; }
    uint64_t sum = 0;
    for (uint32_t x = first; x < first + count; ++x) {
      const uint32_t w = resize_weight(xo, x, n_src, n_dst);
      const uint64_t lo = static_cast<uint64_t>(x) * n_dst > static_cast<uint64_t>(xo) * n_src ? static_cast<uint64_t>(x) * n_dst : static_cast<uint64_t>(xo) * n_src;
      const uint64_t a = static_cast<uint64_t>(x + 1) * n_dst, b = static_cast<uint64_t>(xo + 1) * n_src, hi = a < b ? a : b;
      if (w == 0 || w != hi - lo) { printf("%u -> %u: weight of %u in cell %u is %u\n", n_src, n_dst, x, xo, w); return false; }
      sum += w;
    }
    if (sum != n_src) { printf("%u -> %u: the weights of cell %u sum to %llu\n", n_src, n_dst, xo, static_cast<unsigned long long>(sum)); return false; }
    if ((first > 0 && resize_weight(xo, first - 1, n_src, n_dst) != 0) || (first + count < n_src && resize_weight(xo, first + count, n_src, n_dst) != 0)) {
      printf("%u -> %u: cell %u has a weight outside its indices\n", n_src, n_dst, xo);
      return false;
    }
    end = first + count;
    ++cells;
  }
  if (end != n_src) { printf("%u -> %u: the last cell ends at %u\n", n_src, n_dst, end); return false; }
  return true;
}

static bool check_one(uint64_t S, uint32_t W, uint32_t H) {
  const uint64_t area = static_cast<uint64_t>(W) * H, want = (2 * S + area) / (2 * area);
  const uint32_t got = resize_round(S, W, H);
  ++roundings;
  if (got != want || got > 255u) { printf("%u x %u, S = %llu: got %u, want %llu\n", W, H, static_cast<unsigned long long>(S), got, static_cast<unsigned long long>(want)); return false; }
  return true;
}

// every quotient 0..255 at its smallest sum and the one below it, and the largest sum there is
static bool check_rounding(uint32_t W, uint32_t H) {
  const uint64_t area = static_cast<uint64_t>(W) * H;
  if (!check_one(0, W, H)) return false;
  for (uint64_t q = 1; q <= 255; ++q) {
    const uint64_t smallest = (area * (2 * q - 1) + 1) / 2;
    if ((2 * smallest + area) / (2 * area) != q || (2 * (smallest - 1) + area) / (2 * area) != q - 1) { printf("the test's own edge is wrong at %u x %u, q = %llu\n", W, H, static_cast<unsigned long long>(q)); return false; }
    if (!check_one(smallest, W, H) || !check_one(smallest - 1, W, H)) return false;
  }
  return check_one(255 * area, W, H);
}

int main() {
  for (uint32_t n_src = 1; n_src <= 70; ++n_src) {
    for (uint32_t n_dst = 1; n_dst <= n_src; ++n_dst) if (!check_axis(n_src, n_dst)) return 1;
  }
  for (uint32_t n_dst : {1u, 256u, 65534u, 65535u}) if (!check_axis(65535u, n_dst)) return 1;
  const uint32_t fixed[5][2] = {{1, 1}, {3, 1}, {65535, 1}, {65535, 65535}, {4099, 4111}};
  for (const auto& wh : fixed) if (!check_rounding(wh[0], wh[1])) return 1;
  uint64_t lcg = 0x9e3779b97f4a7c15ull;
  for (int i = 0; i < 300; ++i) {
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    const uint32_t W = 1 + static_cast<uint32_t>((lcg >> 33) % 65535u);
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    const uint32_t H = 1 + static_cast<uint32_t>((lcg >> 33) % 65535u);
    if (!check_rounding(W, H)) return 1;
  }
  printf("resize math ok: %ld cells, %ld roundings\n", cells, roundings);
  return 0;
}
