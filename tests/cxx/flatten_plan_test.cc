// The host half of alpha flattening -- the flatten in resize_plan and sheet_plan (sjpeg_amd/csrc/resize_plan.cc,
// sheet_plan.cc) -- under AddressSanitizer and UndefinedBehaviorSanitizer: tests/test_flatten_cxx.py builds this file
// with them by the host compiler.  Every array handed over lies in a heap buffer of exactly its size.  A flat plan is
// the plan of the same frames as SJPEG_HIP_SRC_RGB pictures but for where the samples are read; every refusal names
// what it refuses.
#include <math.h>
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
static bool said(const char* w) { return g_error.find(w) != std::string::npos; }

int main() {
  using namespace sjpeg_internal;
  const int alpha[5] = {SJPEG_HIP_SRC_BGRA, SJPEG_HIP_SRC_RGBA, SJPEG_HIP_SRC_RGBA_F32, SJPEG_HIP_SRC_RGBA_F16, SJPEG_HIP_SRC_RGBA_BF16};
  const int esz[5] = {1, 1, 4, 2, 2};
  const int n = 5;
  uint32_t seed = 12345u;
  auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
  long plans = 0;
  for (int round = 0; round < 40; ++round) {
    for (int k = 0; k < 5; ++k) {
      std::unique_ptr<sjpeg_hip_ragged_frame[]> frames(new sjpeg_hip_ragged_frame[n]);
      std::unique_ptr<int32_t[][2]> sizes(new int32_t[n][2]);
      std::unique_ptr<uint8_t[]> orients(new uint8_t[n]);
      std::unique_ptr<sjpeg_hip_flatten> fl(new sjpeg_hip_flatten);
      memset(fl.get(), 0, sizeof(sjpeg_hip_flatten));
      fl->background[0] = 17; fl->background[1] = 128; fl->background[2] = 250;
      fl->premultiplied = static_cast<uint8_t>(round & 1);
      fl->alpha_scale = 255.0f; fl->alpha_bias = 0.0f;
      for (int f = 0; f < n; ++f) {
        memset(&frames[f], 0, sizeof(frames[f]));
        frames[f].width = 1 + static_cast<int>(next() % 700); frames[f].height = 1 + static_cast<int>(next() % 90);
        frames[f].plane[0] = reinterpret_cast<void*>(static_cast<uintptr_t>(1) << 30);
        // exactly a row with its alpha, of either sign
        frames[f].row_stride[0] = (next() & 1 ? -1 : 1) * 4ll * frames[f].width * esz[k];
        sizes[f][0] = 1 + static_cast<int>(next() % frames[f].width); sizes[f][1] = 1 + static_cast<int>(next() % frames[f].height);
        orients[f] = static_cast<uint8_t>(1 + next() % 8);
      }
      ResizePlan flat, rgb, plain;
      CHECK(resize_plan("t", alpha[k], n, frames.get(), sizes.get(), orients.get(), &flat, fl.get()) == 0);
      CHECK(resize_plan("t", SJPEG_HIP_SRC_RGB, n, frames.get(), sizes.get(), orients.get(), &rgb) == 0);
      CHECK(resize_plan("t", alpha[k], n, frames.get(), sizes.get(), orients.get(), &plain) == 0);
      CHECK(flat.flat && !rgb.flat && !plain.flat && flat.resized_format == SJPEG_HIP_SRC_RGB);
      CHECK(memcmp(&flat.flatten, fl.get(), sizeof(sjpeg_hip_flatten)) == 0);
      CHECK(flat.bytes == rgb.bytes && flat.tiles == rgb.tiles && flat.frames.size() == rgb.frames.size());
      for (int f = 0; f < n; ++f) {
        const ResizeFrame &a = flat.frames[f], &b = rgb.frames[f], &c = plain.frames[f];
        CHECK(a.dst == b.dst && a.dst_stride == b.dst_stride && a.tile_base == b.tile_base && a.tw == b.tw && a.th == b.th && a.orient == b.orient);
        CHECK(a.w2 == b.w2 && a.h2 == b.h2 && a.off[0] == c.off[0] && a.off[1] == c.off[1] && a.off[2] == c.off[2] && a.row_stride == c.row_stride);
      }
      // sizes NULL, orientations NULL: planned all the same -- the flatten-copy
      CHECK(resize_plan("t", alpha[k], n, frames.get(), nullptr, nullptr, &flat, fl.get()) == 0 && flat.flat && flat.tiles > 0);
      // a row one element short: refused under flatten for the floats, planned without it
      const int f = static_cast<int>(next() % n);
      const int64_t keep = frames[f].row_stride[0];
      frames[f].row_stride[0] = keep < 0 ? keep + esz[k] : keep - esz[k];
      CHECK(resize_plan("t", alpha[k], n, frames.get(), nullptr, nullptr, &flat, fl.get()) == SJPEG_HIP_EINVAL);
      CHECK(said("alpha") && said(("frame " + std::to_string(f) + ":").c_str()));
      CHECK(resize_plan("t", alpha[k], n, frames.get(), nullptr, nullptr, &plain) == 0);
      frames[f].row_stride[0] = keep;
      // the flatten's own fields
      fl->premultiplied = 2;
      CHECK(resize_plan("t", alpha[k], n, frames.get(), nullptr, nullptr, &flat, fl.get()) == SJPEG_HIP_EINVAL && said("premultiplied 2"));
      fl->premultiplied = 0;
      fl->alpha_scale = NAN;
      CHECK((resize_plan("t", alpha[k], n, frames.get(), nullptr, nullptr, &flat, fl.get()) == SJPEG_HIP_EINVAL && said("finite")) == (esz[k] != 1 || k >= 2));
      fl->alpha_scale = 255.0f; fl->alpha_bias = INFINITY;
      CHECK((resize_plan("t", alpha[k], n, frames.get(), nullptr, nullptr, &flat, fl.get()) == 0) == (k < 2));
      fl->alpha_bias = 0.0f;
      // sheets: the flat plan has the places and the bytes of the RGB one
      std::unique_ptr<sjpeg_hip_sheet> sheet(new sjpeg_hip_sheet);
      memset(sheet.get(), 0, sizeof(sjpeg_hip_sheet));
      sheet->cols = 2; sheet->rows = 2; sheet->cell_width = 21; sheet->cell_height = 17; sheet->gutter = 3; sheet->margin = 5;
      SheetPlan sf, sr;
      CHECK(sheet_plan("t", alpha[k], n, frames.get(), sheet.get(), nullptr, orients.get(), &sf, fl.get()) == 0);
      CHECK(sheet_plan("t", SJPEG_HIP_SRC_RGB, n, frames.get(), sheet.get(), nullptr, orients.get(), &sr) == 0);
      CHECK(sf.rgb.flat && !sr.rgb.flat && sf.bytes == sr.bytes && sf.nsheets == sr.nsheets && sf.out_format == SJPEG_HIP_SRC_RGB);
      CHECK(memcmp(sf.places.data(), sr.places.data(), sizeof(SheetPlace) * n) == 0);
      for (int g = 0; g < n; ++g) CHECK(sf.rgb.frames[g].dst == sr.rgb.frames[g].dst && sf.rgb.frames[g].orient == sr.rgb.frames[g].orient);
      plans += 6;
    }
  }
  // formats without alpha, by name
  std::unique_ptr<sjpeg_hip_ragged_frame[]> one(new sjpeg_hip_ragged_frame[1]);
  memset(&one[0], 0, sizeof(one[0]));
  one[0].width = 16; one[0].height = 16;
  for (int i = 0; i < 3; ++i) { one[0].plane[i] = reinterpret_cast<void*>(static_cast<uintptr_t>(1) << 30); one[0].row_stride[i] = 1 << 12; }
  std::unique_ptr<sjpeg_hip_flatten> fl(new sjpeg_hip_flatten);
  memset(fl.get(), 0, sizeof(sjpeg_hip_flatten));
  fl->alpha_scale = 255.0f;
  std::unique_ptr<sjpeg_hip_sheet> sheet(new sjpeg_hip_sheet);
  memset(sheet.get(), 0, sizeof(sjpeg_hip_sheet));
  sheet->cols = 1; sheet->rows = 1; sheet->cell_width = 16; sheet->cell_height = 16;
  int refused = 0;
  for (int format = 0; format < kSourceFormats; ++format) {
    const SourceLayout& L = *source_layout(format);
    const bool has_alpha = L.rgb_like && !L.one_pitch && L.plane[0].step == 4;
    ResizePlan p;
    SheetPlan s;
    const int rc = resize_plan("t", format, 1, one.get(), nullptr, nullptr, &p, fl.get());
    const int rs = sheet_plan("t", format, 1, one.get(), sheet.get(), nullptr, nullptr, &s, fl.get());
    CHECK((rc == 0) == has_alpha && (rs == 0) == has_alpha);
    if (!has_alpha) {
      CHECK(said("no alpha") && said(source_format_name(format)));
      ++refused;
    }
  }
  CHECK(refused == kSourceFormats - 5);
  printf("flatten plan ok: %ld plans, %d formats refused by name\n", plans, refused);
  return 0;
}
