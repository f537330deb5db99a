// The rounding of 16-bit samples (sjpeg_amd/csrc/resize_math.h: resize_round_deep) against plain 64-bit division, under
// AddressSanitizer and UndefinedBehaviorSanitizer: tests/test_yuv16_cxx.py builds this file by the host compiler.  For
// every shift 0..8 and a handful of areas -- A = 1 and A = 65535 * 65535 among them -- the sums at and one around EVERY
// rounding boundary up to the clamp, a few boundaries above it, 0 and full scale (65535 A: the case that needs the
// clamp); then the own-size formula over all 65536 words, and resize_round itself where both apply.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../sjpeg_amd/csrc/resize_math.h"

using sjpeg_internal::resize_round;
using sjpeg_internal::resize_round_deep;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// the contract, as it is written: min(255, floor((2 S + A 2^s) / (A 2^(s+1))))
static uint32_t plain(uint64_t S, uint64_t A, uint32_t s) {
  const uint64_t q = (2u * S + (A << s)) / (A << (s + 1u));
  return q > 255u ? 255u : static_cast<uint32_t>(q);
}

static int one(uint64_t S, uint32_t W, uint32_t H, uint32_t s, long* checked) {
  const uint64_t A = static_cast<uint64_t>(W) * H;
  if (S > 65535u * A) return 0;
  const uint32_t got = resize_round_deep(S, W, H, s), want = plain(S, A, s);
  if (got != want) {
    printf("FAILED: S %llu W %u H %u shift %u: %u, plain division %u\n", static_cast<unsigned long long>(S), W, H, s, got, want);
    return 1;
  }
  ++*checked;
  return 0;
}

int main() {
  const uint32_t dims[][2] = {{1, 1}, {2, 1}, {1, 3}, {5, 7}, {65535, 1}, {1920, 1080}, {20000, 3}, {65535, 65535}, {65535, 65534}, {4099, 4093}};
  long checked = 0;
  for (uint32_t s = 0; s <= 8; ++s) {
    for (const auto& wh : dims) {
      const uint32_t W = wh[0], H = wh[1];
      const uint64_t A = static_cast<uint64_t>(W) * H, d = A << (s + 1u);
      const uint64_t top = 65535u * A;
      CHECK(2u * top + (A << s) < (1ull << 50));                   // the numerator's bound
      // the first S whose quotient is k: 2 S + A 2^s >= k d
      const uint32_t kmax = (65535u >> s) + 1u;
      std::vector<uint32_t> ks;                                    // every boundary up to the clamp and past it, then a few more
      for (uint32_t k = 1; k <= 260u && k <= kmax; ++k) ks.push_back(k);
      for (uint32_t k = 512; k < kmax; k *= 2) ks.push_back(k);
      if (kmax > 260u) { ks.push_back(kmax - 1u); ks.push_back(kmax); }
      for (uint32_t k : ks) {
        const uint64_t need = static_cast<uint64_t>(k) * d - (A << s), Sb = (need + 1u) / 2u;
        if (Sb > 0 && one(Sb - 1u, W, H, s, &checked)) return 1;
        if (one(Sb, W, H, s, &checked) || one(Sb + 1u, W, H, s, &checked)) return 1;
        if (Sb <= top && k <= 255) CHECK(resize_round_deep(Sb, W, H, s) == k && (Sb == 0 || resize_round_deep(Sb - 1u, W, H, s) == k - 1u));
      }
      if (one(0, W, H, s, &checked) || one(top, W, H, s, &checked) || one(top - 1u, W, H, s, &checked)) return 1;
      CHECK(resize_round_deep(top, W, H, s) == 255u);              // full scale: 256 before the clamp at shift 8
      // a constant picture of x is x's own-size value at any area
      for (uint32_t x : {0u, 1u, 127u, 128u, 255u, 256u, 1023u, 0x7fffu, 0x8000u, 0xff7fu, 0xff80u, 0xffffu}) {
        const uint32_t own = (x + ((1u << s) >> 1)) >> s;
        CHECK(resize_round_deep(x * A, W, H, s) == (own > 255u ? 255u : own));
      }
    }
    // own size, every word
    for (uint32_t x = 0; x < 65536u; ++x) {
      const uint32_t own = (x + ((1u << s) >> 1)) >> s;
      CHECK(resize_round_deep(x, 1u, 1u, s) == (own > 255u ? 255u : own));
      ++checked;
    }
  }
  // shift 0 on bytes is resize_round, which is what it was
  for (const auto& wh : dims) {
    const uint64_t A = static_cast<uint64_t>(wh[0]) * wh[1];
    for (uint64_t S : {uint64_t(0), A / 2u, A / 2u + 1u, 127u * A + A / 2u, 255u * A - 1u, 255u * A}) {
      CHECK(resize_round(S, wh[0], wh[1]) == resize_round_deep(S, wh[0], wh[1], 0u));
      CHECK(resize_round(S, wh[0], wh[1]) == static_cast<uint32_t>((2u * S + A) / (2u * A)));
    }
  }
  printf("yuv16 rounding ok: %ld sums\n", checked);
  return 0;
}
