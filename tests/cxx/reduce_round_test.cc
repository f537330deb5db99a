// The rounding of the ragged reduction (sjpeg_amd/csrc/reduce_round.h) on the host: the kernel reads the same text.
// Every factor 1..8 and every sum a box of s * s bytes can have, against the plain integer division; and the layout
// helpers' rows and pictures (whole dwords, multiples of 16).  Stand-alone, host compiler only.
#include <stdint.h>
#include <stdio.h>

#include "reduce_round.h"

int main() {
  using namespace sjpeg_internal;
  long checked = 0;
  for (int s = 1; s <= kReduceMax; ++s) {
    const uint32_t n = static_cast<uint32_t>(s * s);
    if (static_cast<uint64_t>(reduce_magic(s)) * n < (1u << 20) || static_cast<uint64_t>(reduce_magic(s) - 1) * n >= (1u << 20)) {
      printf("factor %d: magic %u is not ceil(2^20 / %u)\n", s, reduce_magic(s), n);
      return 1;
    }
    for (uint32_t sum = 0; sum <= 255u * n; ++sum) {
      const uint32_t want = (sum + n / 2) / n, got = reduce_round(sum, s);
      if (got != want || got > 255u) {
        printf("factor %d sum %u: got %u, want %u\n", s, sum, got, want);
        return 1;
      }
      ++checked;
    }
    // the product stays inside 32 bits at the largest sum
    if ((static_cast<uint64_t>(255u * n + n / 2) * reduce_magic(s)) >> 32 != 0) {
      printf("factor %d: the product overflows\n", s);
      return 1;
    }
  }
  for (int w = 1; w <= 70; ++w) {
    for (int c = 1; c <= 3; c += 2) {
      const size_t rs = reduced_row_stride(w, c);
      if (rs % 4 != 0 || rs < static_cast<size_t>(w) * c || rs >= static_cast<size_t>(w) * c + 4) { printf("row stride of %d x %d\n", w, c); return 1; }
      // the last group's dwords end inside the row
      const size_t groups = (static_cast<size_t>(w) + 3) / 4, last = (groups - 1) * (c == 3 ? 12 : 4);
      if (last >= rs) { printf("group start past the row: %d x %d\n", w, c); return 1; }
      for (int h = 1; h <= 9; ++h) {
        const size_t pb = reduced_picture_bytes(w, h, c);
        if (pb % 16 != 0 || pb < rs * h || pb >= rs * h + 16) { printf("picture bytes of %d x %d x %d\n", w, h, c); return 1; }
      }
    }
  }
  if (reduced_dim(17, 8) != 3 || reduced_dim(1, 8) != 1 || reduced_dim(65535, 1) != 65535 || reduced_dim(16, 8) != 2) { printf("reduced_dim\n"); return 1; }
  printf("reduce rounding ok: %ld sums\n", checked);
  return 0;
}
