// stuff_wave_body.h -- what ONE LANE of stuff_chunks_wave (stitch_kernels.h, K5 of the launches that are not fused) does
// with its 16 bytes of the un-stuffed stream: count their 0xFF bytes, and write them, with a 0x00 behind every 0xFF,
// straight to the output.  Stated once for the kernel and for the host: tests/cxx/stuff_wave_emul.cc runs these
// functions for the 64 lanes of a wave in both orders and holds every store to the invariant below.  Plain C++ (a host
// compiler reads it as it is); the wave's scan of the counts is the kernel's (and the emulation's) own.
//
// THE INVARIANT: every byte of a frame's body is written exactly once, by the lane that owns its source byte; a 0x00 is
// written by the lane that owns the 0xFF in front of it; no lane ever stores past its last byte.  So there is no
// neighbour to complete, no word "behind", no ordering between lanes, and no two stores of a lane overlap.
#ifndef SJPEG_AMD_STUFF_WAVE_BODY_H_
#define SJPEG_AMD_STUFF_WAVE_BODY_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define SJPEG_STUFF_HD __host__ __device__ __forceinline__
#else
#define SJPEG_STUFF_HD inline
#endif
// every store goes through here: (address, bytes).  The emulation records them; the kernel has nothing to say.
#ifndef SJPEG_STUFF_STORE
#define SJPEG_STUFF_STORE(p, n) ((void)0)
#endif

namespace sjpeg_internal {

// 0x80 in every byte of w that equals 0xFF (exact, no carries between bytes)
SJPEG_STUFF_HD uint32_t ff_bytes(uint32_t w) {
  // low seven bits all set <=> + 1 carries into bit 7 (never out of the byte), and bit 7 itself set
  return ((w & 0x7f7f7f7fu) + 0x01010101u) & w & 0x80808080u;
}
SJPEG_STUFF_HD uint32_t count_ff(uint32_t w, int nbytes /*valid leading bytes, MSB first*/) {
  uint32_t n = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    if (b < nbytes && ((w >> (24 - 8 * b)) & 0xffu) == 0xffu) ++n;
  }
  return n;
}

// bytes at any address: the 16-byte one is ONE global_store_dwordx4 on gfx950 (checked in the ISA)
struct __attribute__((packed, aligned(1))) StuffBytes16 { uint32_t v[4]; };
struct __attribute__((packed, aligned(1))) StuffBytes8 { uint32_t v[2]; };
struct __attribute__((packed, aligned(1))) StuffBytes4 { uint32_t v; };
struct __attribute__((packed, aligned(1))) StuffBytes2 { uint16_t v; };

// the lane's bytes of the stream: 16, fewer where the stream ends inside them, none behind its end
// (rest: bytes of the stream from the chunk's first on, 4096 at most; at: the lane's first, in the chunk)
SJPEG_STUFF_HD int stuff_valid(uint32_t rest, uint32_t at) {
  const int v = static_cast<int>(rest) - static_cast<int>(at);
  return v < 0 ? 0 : v > 16 ? 16 : v;
}

// What a lane holds of its 16 bytes: w, the four words MSB first as K3 leaves them; d, the same as memory-order dwords
// (byte i of the lane is byte i & 3 of d[i >> 2]); t, 0x80 in every byte of d that is 0xFF.
struct StuffLane { uint32_t w[4], d[4], t[4]; };
SJPEG_STUFF_HD StuffLane stuff_lane(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
  StuffLane l;
  l.w[0] = w0; l.w[1] = w1; l.w[2] = w2; l.w[3] = w3;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    l.d[j] = __builtin_bswap32(l.w[j]);
    l.t[j] = ff_bytes(l.d[j]);
  }
  return l;
}

// 0xFF bytes among the lane's valid ones
SJPEG_STUFF_HD uint32_t stuff_count(const StuffLane& l, int valid) {
  uint32_t n = 0;
  if (valid == 16) {
#pragma unroll
    for (int j = 0; j < 4; ++j) n += static_cast<uint32_t>(__builtin_popcount(l.t[j]));
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) n += count_ff(l.w[j], valid - 4 * j);
  }
  return n;
}

// (hi:lo) >> s, s = 0..31: the low dword (one v_alignbit_b32)
SJPEG_STUFF_HD uint32_t stuff_shr(uint32_t hi, uint32_t lo, uint32_t s) {
  return static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | lo) >> s);
}

// The lane's `valid` bytes and the 0x00 behind each of its `count` 0xFF bytes, valid + count bytes in all, to
// base + off .. -- exact lengths only.  base is the chunk's (wave-uniform), off the lane's place behind it.
SJPEG_STUFF_HD void stuff_store(uint8_t* base, uint32_t off, const StuffLane& l, int valid, uint32_t count) {
  uint32_t d0 = l.d[0], d1 = l.d[1], d2 = l.d[2], d3 = l.d[3];
  if (valid == 16 && count == 0u) {                          // 94 % of the lanes: one store
    SJPEG_STUFF_STORE(base + off, 16);
    *reinterpret_cast<StuffBytes16*>(base + off) = StuffBytes16{{d0, d1, d2, d3}};
    return;
  }
  if (valid == 0) return;
  if (valid == 16 && count == 1u) {
    // Nearly every other lane: ONE 0xFF, at byte f.  Bytes 0 .. f stay, the rest moves up a byte and leaves the 0x00
    // behind the 0xFF -- 17 bytes: one 16-byte store and one byte.  The bits that stay: t, as one number of 128 bits,
    // has the top bit of byte f set and no other; t | (t - 1) is that bit and every bit below it.
    const unsigned __int128 t = static_cast<unsigned __int128>(l.t[0]) | static_cast<unsigned __int128>(l.t[1]) << 32 |
                                static_cast<unsigned __int128>(l.t[2]) << 64 | static_cast<unsigned __int128>(l.t[3]) << 96;
    const unsigned __int128 low128 = t | (t - 1);
    uint32_t stay[4], move[4];
    const uint32_t d[4] = {d0, d1, d2, d3};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t low = static_cast<uint32_t>(low128 >> (32 * k));
      stay[k] = d[k] & low;
      move[k] = d[k] & ~low;
    }
    SJPEG_STUFF_STORE(base + off, 16);
    *reinterpret_cast<StuffBytes16*>(base + off) =
        StuffBytes16{{stay[0] | move[0] << 8, stay[1] | stuff_shr(move[1], move[0], 24), stay[2] | stuff_shr(move[2], move[1], 24),
                      stay[3] | stuff_shr(move[3], move[2], 24)}};
    SJPEG_STUFF_STORE(base + (off + 16u), 1);
    base[off + 16u] = static_cast<uint8_t>(move[3] >> 24);
    return;
  }
  // The rest -- two 0xFF bytes or more, or the lane the stream ends in: one round per 0xFF byte and one for what lies
  // behind the last: the bytes up to and with the 0xFF in pieces of 16 / 8 / 4 / 2 / 1, then its 0x00.  d0 .. d3 are
  // shifted down by what was written: the piece at hand always starts at byte 0 of d0, and a dword that no remaining
  // byte can reach may hold anything.
  // mask, bit i: byte i of the lane is a 0xFF of the stream (the 0x80 of every byte gathered by one multiply: bits 7, 15,
  // 23, 31 land at 28 .. 31, and no two products of single bits at the same place)
  uint32_t mask = (l.t[0] * 0x00204081u) >> 28 | ((l.t[1] * 0x00204081u) >> 28) << 4 |
                  ((l.t[2] * 0x00204081u) >> 28) << 8 | ((l.t[3] * 0x00204081u) >> 28) << 12;
  mask &= 0xffffu >> (16 - valid);
  uint32_t pos = 0;
  for (;;) {
    const uint32_t end = mask != 0u ? static_cast<uint32_t>(__builtin_ctz(mask)) + 1u : static_cast<uint32_t>(valid);
    const uint32_t n = end - pos;                            // 0 .. 16
    if (n & 16u) {
      SJPEG_STUFF_STORE(base + off, 16);
      *reinterpret_cast<StuffBytes16*>(base + off) = StuffBytes16{{d0, d1, d2, d3}};
    }
    if (n & 8u) {
      SJPEG_STUFF_STORE(base + off, 8);
      *reinterpret_cast<StuffBytes8*>(base + off) = StuffBytes8{{d0, d1}};
      d0 = d2; d1 = d3;
    }
    if (n & 4u) {
      SJPEG_STUFF_STORE(base + (off + (n & 8u)), 4);
      *reinterpret_cast<StuffBytes4*>(base + (off + (n & 8u))) = StuffBytes4{d0};
      d0 = d1; d1 = d2; d2 = d3;
    }
    if (n & 2u) {
      SJPEG_STUFF_STORE(base + (off + (n & 12u)), 2);
      *reinterpret_cast<StuffBytes2*>(base + (off + (n & 12u))) = StuffBytes2{static_cast<uint16_t>(d0)};
    }
    if (n & 1u) {
      SJPEG_STUFF_STORE(base + (off + (n & 14u)), 1);
      base[off + (n & 14u)] = static_cast<uint8_t>(d0 >> (8u * (n & 2u)));
    }
    const uint32_t r = 8u * (n & 3u);
    d0 = stuff_shr(d1, d0, r); d1 = stuff_shr(d2, d1, r); d2 = stuff_shr(d3, d2, r); d3 >>= r;
    off += n;
    if (mask == 0u) break;
    SJPEG_STUFF_STORE(base + off, 1);
    base[off] = 0;
    off += 1u;
    mask &= mask - 1u;
    pos = end;
  }
}

}  // namespace sjpeg_internal

#endif  // SJPEG_AMD_STUFF_WAVE_BODY_H_
