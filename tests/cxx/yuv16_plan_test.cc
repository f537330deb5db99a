// The plan of a deep call (sjpeg_amd/csrc/yuv_resize_plan.cc with a sjpeg_hip_yuv_depth) and a walk of what the resize
// kernel's deep instantiations read, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/test_yuv16_cxx.py
// builds this file by the host compiler.  For the four formats x shifts {0, 2, 8} x orientations 1..8 x a few size
// pairs the batch is planned; then every plane is walked tile by tile as resize.hip walks it -- the same segment, the
// same capacity of the stage in 16-bit samples, the same chunks, the same staging rule: whole dwords, then at most one
// trailing 16-bit element -- with every source row in a heap buffer of EXACTLY the row's size, so that a read past a
// row's last sample is an error here.  The samples summed from the stage and rounded by resize_round_deep must be the
// contract's: the plain weighted sum over the whole plane, divided with 64-bit integers.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../sjpeg_amd/csrc/ragged_aux.h"
#include "../../sjpeg_amd/csrc/resize_math.h"
#include "sjpeg_hip.h"

static std::string g_error;
namespace sjpeg_internal {
int set_error(int code, const std::string& msg) { g_error = msg; return code; }
}  // namespace sjpeg_internal

using namespace sjpeg_internal;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #c, g_error.c_str()); return 1; } } while (0)

constexpr unsigned kStageBytes = 16384;      // resize.hip's
static unsigned align4(unsigned n) { return (n + 3u) & ~3u; }

// a plane's rows, each in a buffer of exactly its bytes
struct Rows {
  std::vector<std::unique_ptr<uint8_t[]>> row;
  size_t bytes = 0;
  uint16_t word(int y, size_t k) const { uint16_t v; memcpy(&v, row[y].get() + 2 * k, 2); return v; }
};

static long g_chunked = 0, g_tails = 0;

// resize.hip's stage_words over one row: nw samples from byte `at` of the row into the stage at l
static int stage_words(const Rows& rows, int y, size_t at, unsigned nw, uint8_t* stage, uint8_t* written, unsigned l) {
  const unsigned nd = nw >> 1;
  CHECK(at % 2 == 0 && l % 4 == 0 && l + 2u * nw <= kStageBytes);
  for (unsigned i = 0; i < nd; ++i) {
    CHECK(at + 4u * i + 4u <= rows.bytes);                         // no dword reaches past the row's last sample
    memcpy(stage + l + 4u * i, rows.row[y].get() + at + 4u * i, 4);
    memset(written + l + 4u * i, 1, 4);
  }
  if (nw & 1u) {
    CHECK(at + 2u * nw <= rows.bytes);
    memcpy(stage + l + 2u * (nw - 1u), rows.row[y].get() + at + 2u * (nw - 1u), 2);
    memset(written + l + 2u * (nw - 1u), 1, 2);
    ++g_tails;
  }
  return 0;
}

// the kernel's walk of one plane: made[(y * w2 + x) * channels + c]
static int walk_plane(const YuvPlane& p, unsigned shift, const Rows& rows, std::vector<uint8_t>* made) {
  const ResizeFrame& d = p.r;
  const uint32_t W = d.W, H = d.H, w2 = d.w2, h2 = d.h2;
  const unsigned channels = p.channels;
  const bool packed = channels == 2;
  made->assign(static_cast<size_t>(w2) * h2 * channels, 0xEE);
  std::vector<uint8_t> stage(kStageBytes), written(kStageBytes);
  const unsigned tiles_y = (h2 + d.th - 1) / d.th;
  for (unsigned tyi = 0; tyi < tiles_y; ++tyi) {
    for (unsigned txi = 0; txi < d.tiles_x; ++txi) {
      const uint32_t ox0 = txi * d.tw, oy0 = tyi * d.th;
      const uint32_t tw = std::min<uint32_t>(d.tw, w2 - ox0), th = std::min<uint32_t>(d.th, h2 - oy0);
      const uint32_t xs = resize_first(ox0, W, w2), xe = resize_first(ox0 + tw - 1u, W, w2) + resize_count(ox0 + tw - 1u, W, w2);
      const uint32_t ys = resize_first(oy0, H, h2), ye = resize_first(oy0 + th - 1u, H, h2) + resize_count(oy0 + th - 1u, H, h2);
      CHECK(xe <= W && ye <= H);
      const unsigned esz = 2, lstep = (packed ? 2u : 1u) * esz;
      const unsigned cap = packed ? kStageBytes / lstep : (kStageBytes / (channels * esz)) & ~3u;
      CHECK(cap == (packed ? 4096u : 8192u));
      const unsigned seg = xe - xs, clen_max = std::min(seg, cap);
      const unsigned cpitch = packed ? 0u : align4(clen_max * esz);
      const unsigned rpitch = packed ? align4(clen_max * lstep) : cpitch * channels;
      const unsigned R = seg > cap ? 1u : kStageBytes / rpitch;
      CHECK(R >= 1 && R * rpitch <= kStageBytes);
      if (seg > cap) ++g_chunked;
      unsigned coff[2] = {packed ? static_cast<unsigned>(d.off[0]) * esz : 0u, packed ? static_cast<unsigned>(d.off[1]) * esz : 0u};
      std::vector<uint32_t> h(static_cast<size_t>(tw) * 2, 0u);
      std::vector<uint64_t> acc(static_cast<size_t>(tw) * 2, 0ull);
      uint32_t yo = oy0;
      for (uint32_t yb = ys; yb < ye; yb += R) {
        const unsigned nr = std::min(R, ye - yb);
        for (uint32_t xc = xs; xc < xe; xc += cap) {
          const unsigned clen = std::min(cap, xe - xc);
          std::fill(written.begin(), written.end(), 0);
          for (unsigned r = 0; r < nr; ++r) {
            if (packed) {
              if (stage_words(rows, yb + r, static_cast<size_t>(xc) * lstep, clen * 2u, stage.data(), written.data(), r * rpitch)) return 1;
            } else {
              if (stage_words(rows, yb + r, (static_cast<size_t>(d.off[0]) + xc) * 2, clen, stage.data(), written.data(), r * rpitch)) return 1;
            }
          }
          const bool first = xc == xs, last = xc + clen == xe;
          uint32_t yo_chunk = yo;
          for (unsigned r = 0; r < nr; ++r) {
            const uint32_t y = yb + r;
            for (uint32_t j = 0; j < tw; ++j) {
              const uint32_t cx0 = resize_first(ox0 + j, W, w2), cx1 = cx0 + resize_count(ox0 + j, W, w2);
              const uint32_t lo = std::max(cx0, xc), hi = std::min(cx1, xc + clen);
              if (first) { h[2 * j] = 0u; h[2 * j + 1] = 0u; }
              for (uint32_t x = lo; x < hi; ++x) {
                const uint32_t w = resize_weight(ox0 + j, x, W, w2);
                for (unsigned c = 0; c < channels; ++c) {
                  const unsigned at = r * rpitch + (x - xc) * lstep + coff[c];
                  CHECK(at + 2u <= kStageBytes && written[at] && written[at + 1]);
                  uint16_t v; memcpy(&v, stage.data() + at, 2);
                  const uint64_t sum = static_cast<uint64_t>(h[2 * j + c]) + static_cast<uint64_t>(w) * v;
                  CHECK(sum < (1ull << 32));                       // the 32-bit h stays
                  h[2 * j + c] = static_cast<uint32_t>(sum);
                }
              }
              if (!last) continue;
              const uint32_t wy = resize_weight(yo_chunk, y, H, h2);
              for (unsigned c = 0; c < channels; ++c) acc[2 * j + c] += static_cast<uint64_t>(wy) * h[2 * j + c];
              if (static_cast<uint64_t>(y + 1u) * h2 >= static_cast<uint64_t>(yo_chunk + 1u) * H) {
                for (unsigned c = 0; c < channels; ++c) {
                  CHECK(acc[2 * j + c] < (1ull << 48));            // ... and the 64-bit acc
                  (*made)[(static_cast<size_t>(yo_chunk) * w2 + ox0 + j) * channels + c] =
                      static_cast<uint8_t>(resize_round_deep(acc[2 * j + c], W, H, shift));
                }
                const uint32_t wn = yo_chunk + 1u < oy0 + th ? resize_weight(yo_chunk + 1u, y, H, h2) : 0u;
                for (unsigned c = 0; c < channels; ++c) acc[2 * j + c] = static_cast<uint64_t>(wn) * h[2 * j + c];
              }
            }
            if (last && static_cast<uint64_t>(y + 1u) * h2 >= static_cast<uint64_t>(yo_chunk + 1u) * H) ++yo_chunk;
          }
          yo = yo_chunk;
        }
      }
      CHECK(yo == oy0 + th);
    }
  }
  return 0;
}

// the contract on the whole plane, nothing shared with the walk but the weights
static int contract_plane(const YuvPlane& p, unsigned shift, const Rows& rows, const std::vector<uint8_t>& made) {
  const ResizeFrame& d = p.r;
  const uint32_t W = d.W, H = d.H, w2 = d.w2, h2 = d.h2;
  const unsigned channels = p.channels;
  const uint64_t A = static_cast<uint64_t>(W) * H;
  for (uint32_t j = 0; j < h2; ++j) {
    for (uint32_t i = 0; i < w2; ++i) {
      for (unsigned c = 0; c < channels; ++c) {
        uint64_t S = 0;
        for (uint32_t y = resize_first(j, H, h2); y < resize_first(j, H, h2) + resize_count(j, H, h2); ++y) {
          uint64_t hs = 0;
          for (uint32_t x = resize_first(i, W, w2); x < resize_first(i, W, w2) + resize_count(i, W, w2); ++x) {
            const size_t k = channels == 2 ? 2u * x + static_cast<size_t>(d.off[c]) : x;
            hs += static_cast<uint64_t>(resize_weight(i, x, W, w2)) * rows.word(y, k);
          }
          S += resize_weight(j, y, H, h2) * hs;
        }
        const uint64_t q = (2u * S + (A << shift)) / (A << (shift + 1u));
        CHECK(made[(static_cast<size_t>(j) * w2 + i) * channels + c] == (q > 255u ? 255u : q));
      }
    }
  }
  return 0;
}

static int one_plan(int format, unsigned shift, int orient, const int (&src)[2], const int (&dst)[2], uint32_t* seed, long* plans) {
  auto next = [&]() { *seed = *seed * 1664525u + 1013904223u; return *seed >> 8; };
  const int nplanes = format == SJPEG_HIP_SRC_NV12 || format == SJPEG_HIP_SRC_NV21 ? 2 : 3;
  const bool full = format == SJPEG_HIP_SRC_YUV444;
  std::unique_ptr<sjpeg_hip_ragged_frame[]> frames(new sjpeg_hip_ragged_frame[1]);
  std::unique_ptr<int32_t[][2]> sizes(new int32_t[1][2]);
  std::unique_ptr<uint8_t[]> orients(new uint8_t[1]);
  std::unique_ptr<sjpeg_hip_yuv_depth> depth(new sjpeg_hip_yuv_depth);
  memset(&frames[0], 0, sizeof(frames[0]));
  frames[0].width = src[0]; frames[0].height = src[1];
  sizes[0][0] = dst[0]; sizes[0][1] = dst[1];
  orients[0] = static_cast<uint8_t>(orient);
  depth->bytes = 2; depth->shift = static_cast<uint8_t>(shift); depth->reserved[0] = depth->reserved[1] = 0;
  Rows rows[3];
  for (int i = 0; i < nplanes; ++i) {
    const int pw = i == 0 || full ? src[0] : (src[0] + 1) / 2, ph = i == 0 || full ? src[1] : (src[1] + 1) / 2;
    rows[i].bytes = static_cast<size_t>(pw) * (nplanes == 2 && i == 1 ? 4 : 2);
    // (words of every size: mostly at the depth's scale, some with bits above it, some full scale)
    const unsigned kind = next() % 4;
    for (int y = 0; y < ph; ++y) {
      rows[i].row.emplace_back(new uint8_t[rows[i].bytes]);
      for (size_t k = 0; k < rows[i].bytes / 2; ++k) {
        const uint16_t v = kind == 0 ? 0xffffu : static_cast<uint16_t>(kind == 1 ? next() : next() & ((256u << shift) - 1u));
        memcpy(rows[i].row.back().get() + 2 * k, &v, 2);
      }
    }
    frames[0].plane[i] = rows[i].row[0].get();
    frames[0].row_stride[i] = static_cast<int64_t>(rows[i].bytes);
  }
  YuvResizePlan plan, plain;
  CHECK(yuv_resize_plan("test", format, 1, frames.get(), sizes.get(), orients.get(), &plan, depth.get()) == 0);
  CHECK(yuv_resize_plan("test", format, 1, frames.get(), sizes.get(), orients.get(), &plain) == 0);
  ++*plans;
  // the depth marks the plan and changes nothing else: the made planes are bytes
  CHECK(plan.deep && plan.shift == shift && !plain.deep);
  CHECK(plan.bytes == plain.bytes && plan.tiles == plain.tiles && plan.planes.size() == plain.planes.size());
  CHECK(plan.bytes == sjpeg_hip_resize_ragged_yuv_bytes(format, 1, frames.get(), sizes.get(), orients.get()));
  for (size_t k = 0; k < plan.planes.size(); ++k) CHECK(memcmp(&plan.planes[k], &plain.planes[k], sizeof(YuvPlane)) == 0);
  CHECK(plan.planes.size() == static_cast<size_t>(nplanes));
  for (int i = 0; i < nplanes; ++i) {
    const YuvPlane& p = plan.planes[i];
    CHECK(p.r.src == frames[0].plane[i] && p.r.orient == static_cast<unsigned>(orient));
    if (orient > 1) continue;                                      // (the walk reads the same bytes at every orientation)
    std::vector<uint8_t> made;
    if (walk_plane(p, shift, rows[i], &made) != 0) return 1;
    if (contract_plane(p, shift, rows[i], made) != 0) return 1;
  }
  return 0;
}

static int refusals() {
  std::unique_ptr<sjpeg_hip_ragged_frame[]> frames(new sjpeg_hip_ragged_frame[1]);
  memset(&frames[0], 0, sizeof(frames[0]));
  frames[0].width = 16; frames[0].height = 8;
  std::unique_ptr<sjpeg_hip_yuv_depth> depth(new sjpeg_hip_yuv_depth);
  YuvResizePlan plan;
  auto refused = [&](uint8_t bytes, uint8_t shift, uint8_t r0, uint8_t r1, const char* words) {
    depth->bytes = bytes; depth->shift = shift; depth->reserved[0] = r0; depth->reserved[1] = r1;
    return yuv_resize_plan("t", SJPEG_HIP_SRC_NV12, 1, frames.get(), nullptr, nullptr, &plan, depth.get()) == SJPEG_HIP_EINVAL &&
           yuv_depth_check("t", depth.get()) == SJPEG_HIP_EINVAL && g_error.find(words) != std::string::npos;
  };
  CHECK(refused(1, 8, 0, 0, "depth: bytes 1 is not 2"));
  CHECK(refused(4, 8, 0, 0, "depth: bytes 4 is not 2"));
  CHECK(refused(2, 9, 0, 0, "depth: shift 9 is not one of 0..8"));
  CHECK(refused(2, 8, 1, 0, "depth: reserved must be 0"));
  CHECK(refused(2, 8, 0, 7, "depth: reserved must be 0"));
  CHECK(yuv_depth_check("t", nullptr) == SJPEG_HIP_EINVAL && g_error == "t: depth == NULL");
  depth->bytes = 2; depth->shift = 0; depth->reserved[0] = depth->reserved[1] = 0;
  CHECK(yuv_depth_check("t", depth.get()) == 0);
  CHECK(yuv_resize_plan("t", SJPEG_HIP_SRC_RGB, 1, frames.get(), nullptr, nullptr, &plan, depth.get()) == SJPEG_HIP_EINVAL);
  CHECK(g_error.find("SJPEG_HIP_SRC_RGB is not a YUV-plane format") != std::string::npos);
  // the host helper: the own-size formula, every field checked
  std::unique_ptr<uint16_t[]> in(new uint16_t[4]{0x7f, 0x80, 0xff80, 0xffff});
  std::unique_ptr<uint8_t[]> out(new uint8_t[4]);
  depth->shift = 8;
  CHECK(sjpeg_hip_yuv16_samples(depth.get(), 4, in.get(), out.get()) == 0 && out[0] == 0 && out[1] == 1 && out[2] == 255 && out[3] == 255);
  CHECK(sjpeg_hip_yuv16_samples(nullptr, 4, in.get(), out.get()) == SJPEG_HIP_EINVAL);
  CHECK(sjpeg_hip_yuv16_samples(depth.get(), 4, nullptr, out.get()) == SJPEG_HIP_EINVAL);
  CHECK(sjpeg_hip_yuv16_samples(depth.get(), 0, nullptr, nullptr) == 0);
  return 0;
}

int main() {
  const int formats[4] = {SJPEG_HIP_SRC_YUV444, SJPEG_HIP_SRC_YUV420, SJPEG_HIP_SRC_NV12, SJPEG_HIP_SRC_NV21};
  // odd sizes and chroma of (w + 1) / 2, own size and about 2 / 3, trailing elements and dword tails; several rows a
  // stage and several tiles; a luma segment above 8192 samples and a UV segment above 4096 pairs (both in chunks), and
  // the widths at and one around the two capacities
  const int pairs[][2][2] = {{{1, 1}, {1, 1}}, {{2, 2}, {2, 2}}, {{2, 2}, {1, 1}}, {{3, 5}, {3, 5}}, {{3, 5}, {2, 3}}, {{17, 9}, {17, 9}},
                             {{17, 9}, {11, 6}}, {{37, 23}, {13, 9}}, {{640, 70}, {5, 33}}, {{700, 40}, {300, 17}}, {{20001, 3}, {3, 2}},
                             {{8192, 2}, {1, 1}}, {{8193, 2}, {1, 2}}, {{16385, 2}, {2, 1}}, {{16386, 3}, {1, 1}}};
  uint32_t seed = 20262;
  long plans = 0;
  for (int format : formats) {
    for (unsigned shift : {0u, 2u, 8u}) {
      for (int orient = 1; orient <= 8; ++orient) {
        for (const auto& pr : pairs) {
          if (one_plan(format, shift, orient, pr[0], pr[1], &seed, &plans) != 0) return 1;
        }
      }
    }
  }
  if (g_chunked == 0 || g_tails == 0) { printf("FAILED: no chunked tile (%ld) or no trailing element (%ld) was walked\n", g_chunked, g_tails); return 1; }
  if (refusals() != 0) return 1;
  printf("yuv16 plan ok: %ld plans, %ld chunked tiles\n", plans, g_chunked);
  return 0;
}
