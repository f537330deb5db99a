// The lane's part of stuff_chunks_wave (sjpeg_amd/csrc/stuff_wave_body.h, the kernel's own source) on the CPU, as the
// other *_kernel_emul.cc files run theirs: a "wave" is 64 calls of the lane's functions, once in the order 0..63 and
// once 63..0 -- the kernel has no LDS, no barrier and no order between lanes, so the lanes need no threads; the scan of
// the counts between the two halves of a lane's work is a plain loop here and DPP there.  What the kernel does around
// the body -- the four sub-blocks of a chunk, the clipped loads, the running count -- is restated below as the kernel
// has it.  The un-stuffed stream lies in a heap buffer of exactly the words K3 would have written (the last word's
// bytes behind the stream's end are 1-bits, the words behind it another pattern; the buffer ends at the next multiple
// of four words, as ubuf_words does), the output in a buffer pre-filled with a sentinel, and EVERY store goes through
// SJPEG_STUFF_STORE, which counts the writes of every byte address.  Held for every stream:
//   * the output equals the plain definition: copy, 0x00 behind every 0xFF;
//   * no address is written twice, and every byte of the body is written;
//   * none is written outside [base, base + nbytes + total_ff);
//   * the sentinel survives on both sides.
// Streams: the file of tests/test_stuff_wave_cxx.py (every stream of tests/stitch_cases.py that the band route uses, with
// its header's length as the misalignment of `base`), every 0xFF mask of one lane (65 536) between plain and between
// all-0xFF neighbours, a 0xFF at bytes 1023 / 1024 and 4095 / 4096, a KiB and a whole chunk of 0xFF, stream lengths
// 1..17 and 4096 k, k +- 1, each at all 16 alignments of `base`.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

static uint8_t* g_lo = nullptr;          // the whole output buffer, sentinels included
static size_t g_len = 0;
static std::vector<uint8_t> g_writes;    // stores per byte of it
static bool g_bad = false;
static void record_store(const uint8_t* p, int n) {
  if (p < g_lo || p + n > g_lo + g_len) {
    if (!g_bad) printf("a store of %d bytes at offset %td lies outside the buffer\n", n, p - g_lo);
    g_bad = true;
    return;
  }
  for (int i = 0; i < n; ++i) {
    if (g_writes[(p - g_lo) + i] < 255) ++g_writes[(p - g_lo) + i];
  }
}
#define SJPEG_STUFF_STORE(p, n) record_store((p), (n))
#include "stuff_wave_body.h"

using namespace sjpeg_internal;

constexpr uint32_t kChunkBytes = 4096, kChunkWords = 1024, kSub = 1024;
constexpr uint8_t kSentinel = 0xA5;
constexpr size_t kPad = 96;
static long long g_streams = 0, g_fast = 0, g_one = 0, g_slow = 0;

// one wave, one chunk: what stuff_chunks_wave does behind its early return
static void wave(const uint32_t* ub /*the chunk's words*/, uint32_t rest, uint8_t* base, bool reversed) {
  uint32_t q[4][64][4];
  int valid[4][64];
  for (int k = 0; k < 4; ++k) {
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t at = k * kSub + 16u * lane;
      valid[k][lane] = stuff_valid(rest, at);
      memcpy(q[k][lane], ub + ((valid[k][lane] != 0 ? at : 0u) >> 2), 16);
    }
  }
  uint32_t running = 0;
  for (int k = 0; k < 4; ++k) {
    uint32_t count[64], incl[64], sum = 0;
    for (int i = 0; i < 64; ++i) {
      const int lane = reversed ? 63 - i : i;
      const StuffLane l = stuff_lane(q[k][lane][0], q[k][lane][1], q[k][lane][2], q[k][lane][3]);
      count[lane] = stuff_count(l, valid[k][lane]);
    }
    for (int lane = 0; lane < 64; ++lane) { sum += count[lane]; incl[lane] = sum; }
    for (int i = 0; i < 64; ++i) {
      const uint32_t lane = reversed ? 63 - i : i;
      if (valid[k][lane] == 16 && count[lane] == 0) ++g_fast;
      else if (valid[k][lane] == 16 && count[lane] == 1) ++g_one;
      else if (valid[k][lane] != 0) ++g_slow;
      const StuffLane l = stuff_lane(q[k][lane][0], q[k][lane][1], q[k][lane][2], q[k][lane][3]);
      stuff_store(base, k * kSub + 16u * lane + running + (incl[lane] - count[lane]), l, valid[k][lane], count[lane]);
    }
    running += incl[63];
  }
}

static bool run(const std::string& name, const uint8_t* raw, size_t U, unsigned align) {
  // the plain definition
  std::vector<uint8_t> want;
  want.reserve(U + U / 64 + 16);
  for (size_t i = 0; i < U; ++i) {
    want.push_back(raw[i]);
    if (raw[i] == 0xFF) want.push_back(0);
  }
  // the stream as K3 leaves it: MSB-first words, 1-bits up to the end of the last word, then whatever
  const size_t words = ((((U + 3) >> 2) + 1) + 3) & ~size_t(3);
  uint32_t* ub = static_cast<uint32_t*>(malloc(words * 4));             // (exactly: a read behind it is the sanitizer's)
  for (size_t w = 0; w < words; ++w) {
    uint32_t v = 0;
    for (int b = 0; b < 4; ++b) {
      const size_t i = 4 * w + b;
      const uint8_t byte = i < U ? raw[i] : (i >> 2) == ((U - 1) >> 2) ? 0xFF : (i & 1 ? 0xFF : 0x5A);
      v |= static_cast<uint32_t>(byte) << (24 - 8 * b);
    }
    ub[w] = v;
  }
  const size_t nchunks = (U + kChunkBytes - 1) / kChunkBytes;
  std::vector<size_t> chunk_off(nchunks + 1, 0);                        // K4's scan of K3's counts
  for (size_t c = 0; c < nchunks; ++c) {
    size_t n = 0;
    for (size_t i = c * kChunkBytes; i < U && i < (c + 1) * kChunkBytes; ++i) n += raw[i] == 0xFF;
    chunk_off[c + 1] = chunk_off[c] + n;
  }
  bool ok = true;
  for (int reversed = 0; reversed < 2 && ok; ++reversed) {
    g_len = kPad + 16 + want.size() + kPad;
    uint8_t* buf = static_cast<uint8_t*>(aligned_alloc(16, (g_len + 15) & ~size_t(15)));
    memset(buf, kSentinel, g_len);
    g_lo = buf;
    g_writes.assign(g_len, 0);
    g_bad = false;
    uint8_t* const body = buf + kPad + align;                            // (kPad is a multiple of 16)
    for (size_t i = 0; i < nchunks; ++i) {
      const size_t c = reversed ? nchunks - 1 - i : i;
      const size_t left = U - c * kChunkBytes;
      wave(ub + c * kChunkWords, left < kChunkBytes ? static_cast<uint32_t>(left) : kChunkBytes, body + c * kChunkBytes + chunk_off[c],
           reversed != 0);
    }
    const size_t lo = kPad + align, hi = lo + want.size();
    if (g_bad) ok = false;
    for (size_t i = 0; i < g_len && ok; ++i) {
      const bool inside = i >= lo && i < hi;
      if (g_writes[i] != (inside ? 1 : 0)) {
        printf("%s (base mod 16 = %u, lanes %s): byte %td of the body written %d times\n", name.c_str(), align, reversed ? "63..0" : "0..63",
               static_cast<ptrdiff_t>(i) - static_cast<ptrdiff_t>(lo), g_writes[i]);
        ok = false;
      } else if (buf[i] != (inside ? want[i - lo] : kSentinel)) {
        printf("%s (base mod 16 = %u, lanes %s): byte %td of the body is %02x, not %02x\n", name.c_str(), align, reversed ? "63..0" : "0..63",
               static_cast<ptrdiff_t>(i) - static_cast<ptrdiff_t>(lo), buf[i], inside ? want[i - lo] : kSentinel);
        ok = false;
      }
    }
    free(buf);
  }
  free(ub);
  ++g_streams;
  return ok;
}

static uint32_t g_rng = 12345u;
static uint8_t plain_byte() {                                 // 0 .. 254
  g_rng = g_rng * 1664525u + 1013904223u;
  return static_cast<uint8_t>((g_rng >> 24) % 255u);
}
static std::vector<uint8_t> plain(size_t n) {
  std::vector<uint8_t> v(n);
  for (auto& b : v) b = plain_byte();
  return v;
}

int main(int argc, char** argv) {
  bool ok = true;
  // ---- the streams of the band route
  long long from_file = 0;
  if (argc > 1) {
    FILE* f = fopen(argv[1], "rb");
    if (f == nullptr) { printf("cannot open %s\n", argv[1]); return 2; }
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    for (uint32_t i = 0; i < n && ok; ++i) {
      uint32_t name_len = 0, header_len = 0;
      uint64_t U = 0;
      if (fread(&name_len, 4, 1, f) != 1 || fread(&header_len, 4, 1, f) != 1 || fread(&U, 8, 1, f) != 1) return 2;
      std::string name(name_len, ' ');
      std::vector<uint8_t> raw(U);
      if (fread(&name[0], 1, name_len, f) != name_len || fread(raw.data(), 1, U, f) != U) return 2;
      ok = run(name, raw.data(), U, header_len & 15u) && ok;
      ++from_file;
    }
    fclose(f);
  }
  // ---- every 0xFF mask of one lane, between plain and between all-0xFF neighbours: 85 masks to a chunk
  for (int ffn = 0; ffn < 2 && ok; ++ffn) {
    for (uint32_t m0 = 0; m0 < 65536u && ok; m0 += 85) {
      std::vector<uint8_t> raw = plain(kChunkBytes);
      for (uint32_t j = 0; j < 85 && m0 + j < 65536u; ++j) {
        const uint32_t mask = m0 + j;
        uint8_t* g = raw.data() + 16 * (3 * j);
        if (ffn) { memset(g, 0xFF, 16); memset(g + 32, 0xFF, 16); }
        for (int b = 0; b < 16; ++b) if (mask >> b & 1) g[16 + b] = 0xFF;
      }
      ok = run("masks from " + std::to_string(m0) + (ffn ? ", all-0xFF neighbours" : ", plain neighbours"), raw.data(), raw.size(), (m0 / 85) & 15u) && ok;
    }
  }
  // ---- designed streams, each at all 16 alignments of base
  std::vector<std::pair<std::string, std::vector<uint8_t>>> designed;
  for (size_t at : {size_t(1023), size_t(1024), size_t(4095), size_t(4096)}) {
    for (int run_len = 1; run_len <= 3; ++run_len) {
      std::vector<uint8_t> raw = plain(2 * kChunkBytes + 37);
      for (int i = 0; i < run_len; ++i) raw[at - (run_len - 1) / 2 + i] = 0xFF;
      designed.push_back({"0xFF run of " + std::to_string(run_len) + " around byte " + std::to_string(at), raw});
    }
  }
  {
    std::vector<uint8_t> raw = plain(2 * kChunkBytes + 5);
    for (size_t at : {size_t(1023), size_t(1024), size_t(4095), size_t(4096)}) raw[at] = 0xFF;
    designed.push_back({"0xFF at 1023, 1024, 4095 and 4096", raw});
    raw = plain(3 * kChunkBytes);
    memset(raw.data() + 1024, 0xFF, 1024);
    designed.push_back({"a KiB of 0xFF", raw});
    memset(raw.data() + 1024, 0x11, 1024);
    memset(raw.data() + 1024 + 512, 0xFF, 1024);
    designed.push_back({"a KiB of 0xFF across two sub-blocks", raw});
    raw = plain(3 * kChunkBytes + 100);
    memset(raw.data() + kChunkBytes, 0xFF, kChunkBytes);
    designed.push_back({"a chunk of 0xFF", raw});
    designed.push_back({"two chunks of 0xFF", std::vector<uint8_t>(2 * kChunkBytes, 0xFF)});
  }
  std::vector<size_t> lengths;
  for (size_t u = 1; u <= 17; ++u) lengths.push_back(u);
  for (size_t k = 1; k <= 3; ++k) for (int d = -1; d <= 1; ++d) lengths.push_back(k * kChunkBytes + d);
  for (size_t k : {size_t(1023), size_t(1024), size_t(1025), size_t(2047), size_t(2049), size_t(3072), size_t(4080), size_t(4081)}) lengths.push_back(k);
  for (size_t u : lengths) {
    std::vector<uint8_t> raw = plain(u);
    designed.push_back({"length " + std::to_string(u) + ", plain", raw});
    raw[u - 1] = 0xFF;
    if (u > 1) raw[(u - 1) / 2] = 0xFF;
    designed.push_back({"length " + std::to_string(u) + ", the last byte 0xFF", raw});
    if (u > 1) { raw[u - 2] = 0xFF; raw[u - 1] = 0x7E; designed.push_back({"length " + std::to_string(u) + ", the last but one 0xFF", raw}); }
    designed.push_back({"length " + std::to_string(u) + ", all 0xFF", std::vector<uint8_t>(u, 0xFF)});
  }
  for (const auto& d : designed) {
    for (unsigned align = 0; align < 16 && ok; ++align) ok = run(d.first, d.second.data(), d.second.size(), align) && ok;
  }
  if (!ok) return 1;
  printf("stuff wave emulation ok: %lld streams (%lld of the band route), %lld lanes by the 16-byte store, %lld with one 0xFF, "
         "%lld in pieces; every body byte written once, none outside\n", g_streams, from_file, g_fast, g_one, g_slow);
  return 0;
}
