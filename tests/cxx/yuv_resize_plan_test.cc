// The host half of the YUV-plane resize (sjpeg_amd/csrc/yuv_resize_plan.cc) alone, under AddressSanitizer and
// UndefinedBehaviorSanitizer: tests/test_yuv_resize_plan_cxx.py builds this file with it by the host compiler.  Every
// array handed over lies in a heap buffer of exactly its size.  For batches of all four formats, every orientation and
// sizes from 1 x 1 to the source's, the plan is checked against the header's words: the planes of frame after frame Y,
// U, V, each at a multiple of 16, rows whole dwords apart, inside `bytes` and apart from each other; the tiles of the
// descriptors back to back; the frames reported with the upright size.  Bad arguments come back as SJPEG_HIP_EINVAL.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../sjpeg_amd/csrc/ragged_aux.h"
#include "sjpeg_hip.h"

static std::string g_error;
namespace sjpeg_internal {
int set_error(int code, const std::string& msg) { g_error = msg; return code; }
}  // namespace sjpeg_internal

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #c, g_error.c_str()); return 1; } } while (0)

static int chroma_dim(int format, int v) { return format == SJPEG_HIP_SRC_YUV444 ? v : (v + 1) / 2; }

static int one_batch(int format, int nframes, uint32_t* seed, long* plans) {
  auto next = [&]() { *seed = *seed * 1664525u + 1013904223u; return *seed >> 8; };
  const int nplanes = format == SJPEG_HIP_SRC_NV12 || format == SJPEG_HIP_SRC_NV21 ? 2 : 3;
  std::unique_ptr<sjpeg_hip_ragged_frame[]> frames(new sjpeg_hip_ragged_frame[nframes]);
  std::unique_ptr<int32_t[][2]> sizes(new int32_t[nframes][2]);
  std::unique_ptr<uint8_t[]> orients(new uint8_t[nframes]);
  for (int f = 0; f < nframes; ++f) {
    memset(&frames[f], 0, sizeof(frames[f]));
    const int big = next() % 16 == 0;
    frames[f].width = 1 + static_cast<int>(next() % (big ? 65535 : 700));
    frames[f].height = 1 + static_cast<int>(next() % (big ? 65535 : 90));
    for (int i = 0; i < nplanes; ++i) {
      frames[f].plane[i] = reinterpret_cast<void*>(static_cast<uintptr_t>(0x10000000u + 0x1000000u * i));
      frames[f].row_stride[i] = (next() % 2 ? 1 : -1) * (1 << 18);
    }
    frames[f].out_offset = 4096u * f;
    frames[f].out_capacity = 4096;
    sizes[f][0] = next() % 4 == 0 ? frames[f].width : 1 + static_cast<int>(next() % frames[f].width);
    sizes[f][1] = next() % 4 == 0 ? frames[f].height : 1 + static_cast<int>(next() % frames[f].height);
    orients[f] = static_cast<uint8_t>(1 + next() % 8);
  }
  for (int variant = 0; variant < 4; ++variant) {
    const int32_t (*sz)[2] = variant & 1 ? nullptr : sizes.get();
    const uint8_t* orr = variant & 2 ? nullptr : orients.get();
    sjpeg_internal::YuvResizePlan plan;
    CHECK(sjpeg_internal::yuv_resize_plan("test", format, nframes, frames.get(), sz, orr, &plan) == 0);
    ++*plans;
    CHECK(plan.nframes == nframes && plan.planes.size() == static_cast<size_t>(nframes) * nplanes);
    CHECK(plan.resized_format == (format == SJPEG_HIP_SRC_YUV444 ? SJPEG_HIP_SRC_YUV444 : SJPEG_HIP_SRC_YUV420));
    CHECK(sjpeg_hip_resize_ragged_yuv_bytes(format, nframes, frames.get(), sz, orr) == plan.bytes);
    std::unique_ptr<sjpeg_hip_ragged_frame[]> out(new sjpeg_hip_ragged_frame[nframes]);
    uint8_t* const base = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(0x40000000u));
    sjpeg_internal::yuv_resize_plan_frames(plan, frames.get(), base, out.get());
    size_t at = 0;
    unsigned long long tiles = 0;
    size_t k = 0;
    for (int f = 0; f < nframes; ++f) {
      const int w2 = sz != nullptr ? sz[f][0] : frames[f].width, h2 = sz != nullptr ? sz[f][1] : frames[f].height;
      const int o = orr != nullptr ? orr[f] : 1;
      const int uw = o >= 5 ? h2 : w2, uh = o >= 5 ? w2 : h2;
      CHECK(out[f].width == uw && out[f].height == uh);
      CHECK(out[f].out_offset == frames[f].out_offset && out[f].out_capacity == frames[f].out_capacity);
      for (int c = 0; c < 3; ++c) {                // the layout of the header, restated
        const int pw = c == 0 ? w2 : chroma_dim(format, w2), ph = c == 0 ? h2 : chroma_dim(format, h2);
        const int upw = o >= 5 ? ph : pw, uph = o >= 5 ? pw : ph;
        int hw, hh;
        CHECK(sjpeg_hip_yuv_plane_size(plan.resized_format, uw, uh, c, &hw, &hh) == 0 && hw == upw && hh == uph);
        const size_t stride = (static_cast<size_t>(upw) + 3) & ~static_cast<size_t>(3);
        CHECK(out[f].plane[c] == base + at && out[f].row_stride[c] == static_cast<int64_t>(stride));
        at += (stride * uph + 15) & ~static_cast<size_t>(15);
      }
      for (int i = 0; i < nplanes; ++i, ++k) {
        const sjpeg_internal::YuvPlane& p = plan.planes[k];
        const sjpeg_internal::ResizeFrame& d = p.r;
        CHECK(p.frame == f && p.channels == (nplanes == 2 && i == 1 ? 2 : 1));
        CHECK(d.src == frames[f].plane[i] && d.row_stride == frames[f].row_stride[i]);
        CHECK(d.W == (i == 0 ? frames[f].width : chroma_dim(format, frames[f].width)));
        CHECK(d.H == (i == 0 ? frames[f].height : chroma_dim(format, frames[f].height)));
        CHECK(d.w2 == (i == 0 ? w2 : chroma_dim(format, w2)) && d.h2 == (i == 0 ? h2 : chroma_dim(format, h2)));
        CHECK(d.w2 >= 1 && d.w2 <= d.W && d.h2 >= 1 && d.h2 <= d.H);
        CHECK(d.orient == static_cast<unsigned>(o));
        CHECK(d.tw >= 4 && d.tw <= 256 && (d.tw & (d.tw - 1)) == 0 && d.th >= 1 && d.th <= 16);
        CHECK(d.tile_base == tiles);
        CHECK(d.tiles_x == static_cast<unsigned>((d.w2 + d.tw - 1) / d.tw));
        tiles += static_cast<unsigned long long>(d.tiles_x) * ((d.h2 + d.th - 1) / d.th);
        CHECK(base + reinterpret_cast<uintptr_t>(d.dst) == out[f].plane[i]);
        CHECK(d.dst_stride == static_cast<unsigned>(out[f].row_stride[i]));
        if (p.channels == 2) {
          CHECK(base + reinterpret_cast<uintptr_t>(p.dst2) == out[f].plane[2]);
          CHECK(d.off[0] == (format == SJPEG_HIP_SRC_NV12 ? 0 : 1) && d.off[1] == (format == SJPEG_HIP_SRC_NV12 ? 1 : 0));
        }
      }
    }
    CHECK(at == plan.bytes && tiles == plan.tiles && k == plan.planes.size());
  }
  return 0;
}

static int refusals() {
  std::unique_ptr<sjpeg_hip_ragged_frame[]> frames(new sjpeg_hip_ragged_frame[2]);
  std::unique_ptr<int32_t[][2]> sizes(new int32_t[2][2]);
  std::unique_ptr<uint8_t[]> orients(new uint8_t[2]);
  for (int f = 0; f < 2; ++f) {
    memset(&frames[f], 0, sizeof(frames[f]));
    frames[f].width = 16; frames[f].height = 8;
    sizes[f][0] = 8; sizes[f][1] = 8;
    orients[f] = 6;
  }
  sjpeg_internal::YuvResizePlan plan;
  const int nv = SJPEG_HIP_SRC_NV12;
  CHECK(sjpeg_internal::yuv_resize_plan("t", SJPEG_HIP_SRC_RGB, 2, frames.get(), sizes.get(), orients.get(), &plan) == SJPEG_HIP_EINVAL);
  CHECK(g_error.find("SJPEG_HIP_SRC_RGB is not a YUV-plane format") != std::string::npos);
  CHECK(sjpeg_internal::yuv_resize_plan("t", SJPEG_HIP_SRC_GRAY_F16, 2, frames.get(), nullptr, nullptr, &plan) == SJPEG_HIP_EINVAL);
  CHECK(g_error.find("SJPEG_HIP_SRC_GRAY_F16") != std::string::npos);
  CHECK(sjpeg_internal::yuv_resize_plan("t", -1, 2, frames.get(), nullptr, nullptr, &plan) == SJPEG_HIP_EINVAL);
  CHECK(sjpeg_internal::yuv_resize_plan("t", 21, 2, frames.get(), nullptr, nullptr, &plan) == SJPEG_HIP_EINVAL);
  CHECK(sjpeg_internal::yuv_resize_plan("t", nv, 0, frames.get(), nullptr, nullptr, &plan) == SJPEG_HIP_EINVAL);
  sizes[1][0] = 17;
  CHECK(sjpeg_internal::yuv_resize_plan("t", nv, 2, frames.get(), sizes.get(), orients.get(), &plan) == SJPEG_HIP_EINVAL);
  CHECK(g_error.find("frame 1") != std::string::npos && g_error.find("above the source's 16x8") != std::string::npos);
  sizes[1][0] = 0;
  CHECK(sjpeg_internal::yuv_resize_plan("t", nv, 2, frames.get(), sizes.get(), orients.get(), &plan) == SJPEG_HIP_EINVAL);
  CHECK(g_error.find("below 1x1") != std::string::npos);
  sizes[1][0] = 8; orients[0] = 9;
  CHECK(sjpeg_internal::yuv_resize_plan("t", nv, 2, frames.get(), sizes.get(), orients.get(), &plan) == SJPEG_HIP_EINVAL);
  CHECK(g_error.find("frame 0") != std::string::npos && g_error.find("orientation 9") != std::string::npos);
  orients[0] = 1; frames[1].width = 65536;
  CHECK(sjpeg_internal::yuv_resize_plan("t", nv, 2, frames.get(), nullptr, orients.get(), &plan) == SJPEG_HIP_EINVAL);
  CHECK(g_error.find("bad dimensions") != std::string::npos);
  CHECK(plan.planes.empty() && plan.bytes == 0);               // a refused batch leaves no plan
  CHECK(sjpeg_hip_resize_ragged_yuv_bytes(nv, 2, nullptr, nullptr, nullptr) == 0);
  int pw = 7, ph = 7;
  CHECK(sjpeg_hip_yuv_plane_size(SJPEG_HIP_SRC_BGRA, 8, 8, 0, &pw, &ph) == SJPEG_HIP_EINVAL && pw == 7 && ph == 7);
  CHECK(sjpeg_hip_yuv_plane_size(nv, 8, 8, 3, &pw, &ph) == SJPEG_HIP_EINVAL);
  CHECK(sjpeg_hip_yuv_plane_size(nv, 65535, 65535, 2, &pw, &ph) == 0 && pw == 32768 && ph == 32768);
  // the tile limit: 65535 frames of 65535 x 65535 at their own size pass 2^31 tiles
  const int many = 4096;
  std::unique_ptr<sjpeg_hip_ragged_frame[]> big(new sjpeg_hip_ragged_frame[many]);
  for (int f = 0; f < many; ++f) { memset(&big[f], 0, sizeof(big[f])); big[f].width = 65535; big[f].height = 65535; }
  CHECK(sjpeg_internal::yuv_resize_plan("t", SJPEG_HIP_SRC_YUV444, many, big.get(), nullptr, nullptr, &plan) == SJPEG_HIP_EINVAL);
  CHECK(g_error.find("too many tiles for one launch") != std::string::npos);
  return 0;
}

int main() {
  const int formats[4] = {SJPEG_HIP_SRC_YUV444, SJPEG_HIP_SRC_YUV420, SJPEG_HIP_SRC_NV12, SJPEG_HIP_SRC_NV21};
  uint32_t seed = 20241;
  long plans = 0;
  for (int round = 0; round < 40; ++round) {
    for (int format : formats) {
      if (one_batch(format, 1 + round % 9, &seed, &plans) != 0) return 1;
    }
  }
  if (refusals() != 0) return 1;
  printf("yuv resize plan ok: %ld plans\n", plans);
  return 0;
}
