// resize_plan.cc -- the host half of the ragged resize of the RGB-like and gray formats (sjpeg_hip_resize_ragged_src,
// sjpeg_hip_orient_ragged_src; sjpeg_hip.h): the fitted and the upright size, the checks of the sizes and orientations,
// and the plan -- one descriptor per frame -- that resize.hip's kernel runs over.  Plain C++, no device work: a host
// compiler reads it as it is (tests/cxx/sheet_plan_test.cc), like yuv_resize_plan.cc beside it.
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "light_math.h"
#include "orient_math.h"
#include "ragged_aux.h"
#include "reduce_round.h"
#include "sjpeg_hip.h"
#include "source_layout.h"

namespace {

using sjpeg_internal::ResizeFrame;

const char* yuv_format_name(int format) {
  switch (format) {
    case SJPEG_HIP_SRC_YUV444: return "SJPEG_HIP_SRC_YUV444";
    case SJPEG_HIP_SRC_YUV420: return "SJPEG_HIP_SRC_YUV420";
    case SJPEG_HIP_SRC_NV12: return "SJPEG_HIP_SRC_NV12";
    case SJPEG_HIP_SRC_NV21: return "SJPEG_HIP_SRC_NV21";
    default: return "this format";
  }
}

// a format the kernel reads: every RGB-like row of the table and the gray ones
bool resizable(const sjpeg_internal::SourceLayout& L) { return L.rgb_like || (L.planes == 1 && L.implied == SJPEG_HIP_YUV400); }

}  // namespace

namespace sjpeg_internal {

int flatten_check(const std::string& who, int format, const sjpeg_hip_flatten& flatten) {
  const SourceLayout* const L = source_layout(format);
  if (L == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": unknown source format");
  // an alpha format: one plane of pixels of four bytes or elements, R, G, B and the alpha behind them
  if (!(L->rgb_like && !L->one_pitch && L->plane[0].step == 4)) {
    return set_error(SJPEG_HIP_EINVAL, who + ": flatten: " + source_format_name(format) + " has no alpha channel (a flattened source is "
                                           "SJPEG_HIP_SRC_BGRA, _RGBA or _RGBA_F32 / _F16 / _BF16)");
  }
  if (flatten.premultiplied > 1) {
    return set_error(SJPEG_HIP_EINVAL, who + ": flatten: premultiplied " + std::to_string(flatten.premultiplied) + " is not 0 (straight alpha) or 1");
  }
  if (L->kind != kElemU8 && !(std::isfinite(flatten.alpha_scale) && std::isfinite(flatten.alpha_bias))) {
    return set_error(SJPEG_HIP_EINVAL, who + ": flatten: alpha_scale and alpha_bias must be finite");
  }
  return 0;
}

int light_check(const std::string& who, int light, int format) {
  if (light != SJPEG_HIP_LIGHT_CODED && light != SJPEG_HIP_LIGHT_LINEAR_SRGB) {
    return set_error(SJPEG_HIP_EINVAL, who + ": light " + std::to_string(light) + " is not SJPEG_HIP_LIGHT_CODED (0) or SJPEG_HIP_LIGHT_LINEAR_SRGB (1)");
  }
  const SourceLayout* const L = source_layout(format);
  if (light != SJPEG_HIP_LIGHT_CODED && L != nullptr && !resizable(*L)) {
    return set_error(SJPEG_HIP_EINVAL, who + ": light: the samples of " + source_format_name(format) +
                                           " are not RGB light (linear light takes an RGB-like or a gray format)");
  }
  return 0;
}

int resize_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                const uint8_t* orientations, ResizePlan* plan, const sjpeg_hip_flatten* flatten) {
  const SourceLayout* const L = source_layout(format);
  if (L == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": unknown source format");
  if (nframes < 1 || nframes > 65535) return set_error(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
  if (flatten != nullptr) { if (int rc = flatten_check(who, format, *flatten)) return rc; }
  bool turned = false;
  for (int f = 0; f < nframes; ++f) {
    const sjpeg_hip_ragged_frame& fr = frames[f];
    const std::string frame = who + ": frame " + std::to_string(f) + ": ";
    if (fr.width < 1 || fr.height < 1 || fr.width > 65535 || fr.height > 65535) {
      return set_error(SJPEG_HIP_EINVAL, frame + "bad dimensions " + std::to_string(fr.width) + "x" + std::to_string(fr.height));
    }
    if (orientations != nullptr && (orientations[f] < 1 || orientations[f] > 8)) {
      return set_error(SJPEG_HIP_EINVAL, frame + "orientation " + std::to_string(orientations[f]) + " is not one of 1..8 (EXIF tag 0x0112)");
    }
    turned = turned || (orientations != nullptr && orientations[f] != 1);
    if (flatten != nullptr) {
      // the fourth element of every pixel is read: a row holds its last one (the float formats' rows may else end
      // behind the last colour sample)
      const long long row = 4ll * fr.width * L->esz, have = fr.row_stride[0] < 0 ? -fr.row_stride[0] : fr.row_stride[0];
      if (have < row) {
        return set_error(SJPEG_HIP_EINVAL, frame + "|row_stride| " + std::to_string(have) + " is below the " + std::to_string(row) +
                                               " bytes of a row with its alpha (width * 4 * element size): a flattened source's alpha is read");
      }
    }
    if (sizes == nullptr) continue;
    const std::string size = "size " + std::to_string(sizes[f][0]) + "x" + std::to_string(sizes[f][1]);
    if (sizes[f][0] < 1 || sizes[f][1] < 1) return set_error(SJPEG_HIP_EINVAL, frame + size + " is below 1x1");
    if (sizes[f][0] > fr.width || sizes[f][1] > fr.height) {
      return set_error(SJPEG_HIP_EINVAL, frame + size + " is above the source's " + std::to_string(fr.width) + "x" + std::to_string(fr.height) +
                                             " (pictures are made smaller, never larger)");
    }
  }
  if (!resizable(*L) && turned) {
    return set_error(SJPEG_HIP_EINVAL, who + ": " + yuv_format_name(format) + " pictures are not oriented (an orientation other than 1 takes an RGB-like or a gray format)");
  }
  if (!resizable(*L)) {
    return set_error(SJPEG_HIP_EINVAL, who + ": " + yuv_format_name(format) + " pictures are not resized (a size other than the source's takes an RGB-like or a gray format)");
  }
  const int channels = L->rgb_like ? 3 : 1;
  plan->format = format;
  plan->resized_format = channels == 3 ? SJPEG_HIP_SRC_RGB : SJPEG_HIP_SRC_GRAY;
  plan->flat = flatten != nullptr;
  if (flatten != nullptr) plan->flatten = *flatten;
  plan->frames.assign(static_cast<size_t>(nframes), ResizeFrame());
  size_t at = 0;
  unsigned long long tiles = 0;
  for (int f = 0; f < nframes; ++f) {
    const sjpeg_hip_ragged_frame& fr = frames[f];
    ResizeFrame& d = plan->frames[f];
    memset(&d, 0, sizeof(d));
    const uint8_t* planes[3];
    long long rows[3];
    layout_planes(*L, fr.plane, fr.row_stride, nullptr, planes, rows, nullptr);
    d.src = static_cast<const uint8_t*>(fr.plane[0]);
    d.row_stride = rows[0];
    long long g = 0, b = 0;
    if (channels == 3) layout_rgb_offsets(*L, fr.plane, &g, &b);
    d.off[0] = channels == 3 ? L->r_off : 0; d.off[1] = g; d.off[2] = b;
    d.W = fr.width; d.H = fr.height;
    d.w2 = sizes != nullptr ? sizes[f][0] : fr.width; d.h2 = sizes != nullptr ? sizes[f][1] : fr.height;
    const unsigned long long frame_tiles = resize_tile_rule(&d);
    // the picture in the buffer is the UPRIGHT one: h' x w' for the orientations that transpose
    d.orient = orientations != nullptr ? orientations[f] : 1u;
    uint32_t uw, uh;
    oriented_size(static_cast<uint32_t>(d.w2), static_cast<uint32_t>(d.h2), static_cast<int>(d.orient), &uw, &uh);
    d.dst_stride = static_cast<unsigned>(reduced_row_stride(static_cast<int>(uw), channels));
    d.dst = reinterpret_cast<uint8_t*>(at);                       // (from the buffer's start: engine_resize adds it)
    d.tile_base = static_cast<unsigned>(tiles);
    at += reduced_picture_bytes(static_cast<int>(uw), static_cast<int>(uh), channels);
    tiles += frame_tiles;
    if (tiles > 0x7fffffffull) return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": the batch has too many tiles for one launch");
  }
  plan->bytes = at;
  plan->tiles = static_cast<unsigned>(tiles);
  return 0;
}

void resize_plan_frames(const ResizePlan& plan, const sjpeg_hip_ragged_frame* frames, uint8_t* base, sjpeg_hip_ragged_frame* out) {
  for (size_t f = 0; f < plan.frames.size(); ++f) {
    const ResizeFrame& d = plan.frames[f];
    sjpeg_hip_ragged_frame r;
    memset(&r, 0, sizeof(r));
    r.plane[0] = base + reinterpret_cast<uintptr_t>(d.dst);
    r.row_stride[0] = static_cast<int64_t>(d.dst_stride);
    uint32_t uw, uh;
    oriented_size(static_cast<uint32_t>(d.w2), static_cast<uint32_t>(d.h2), static_cast<int>(d.orient), &uw, &uh);
    r.width = static_cast<int32_t>(uw); r.height = static_cast<int32_t>(uh);
    r.out_offset = frames[f].out_offset; r.out_capacity = frames[f].out_capacity;
    out[f] = r;
  }
}

}  // namespace sjpeg_internal

extern "C" {

int sjpeg_hip_fit_size(int width, int height, int box_width, int box_height, int* fitted_width, int* fitted_height) {
  static const std::string who = "sjpeg_hip_fit_size";
  if (fitted_width == nullptr || fitted_height == nullptr) return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": fitted_width or fitted_height == NULL");
  if (width < 1 || height < 1 || width > 65535 || height > 65535) {
    return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": bad dimensions " + std::to_string(width) + "x" + std::to_string(height));
  }
  if (box_width < 1 || box_height < 1 || box_width > 65535 || box_height > 65535) {
    return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": bad box " + std::to_string(box_width) + "x" + std::to_string(box_height));
  }
  const long long W = width, H = height, bw = box_width, bh = box_height;
  long long w = W, h = H;
  if (W > bw || H > bh) {
    if (W * bh >= H * bw) {
      w = bw; h = (H * bw + W / 2) / W;
    } else {
      h = bh; w = (W * bh + H / 2) / H;
    }
  }
  *fitted_width = static_cast<int>(w < 1 ? 1 : w);
  *fitted_height = static_cast<int>(h < 1 ? 1 : h);
  return 0;
}

int sjpeg_hip_light_table(int light, uint16_t table[256]) {
  static const std::string who = "sjpeg_hip_light_table";
  if (table == nullptr) return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": table == NULL");
  if (int rc = sjpeg_internal::light_check(who, light, -1)) return rc;
  for (int b = 0; b < 256; ++b) table[b] = light == SJPEG_HIP_LIGHT_CODED ? static_cast<uint16_t>(b) : sjpeg_internal::kLightSrgb[b];
  return 0;
}

int sjpeg_hip_light_round(int light, uint64_t S, uint32_t W, uint32_t H, uint32_t* byte) {
  static const std::string who = "sjpeg_hip_light_round";
  if (byte == nullptr) return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": byte == NULL");
  if (int rc = sjpeg_internal::light_check(who, light, -1)) return rc;
  if (W < 1 || H < 1 || W > 65535 || H > 65535) {
    return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": bad dimensions " + std::to_string(W) + "x" + std::to_string(H));
  }
  const uint64_t top = (light == SJPEG_HIP_LIGHT_CODED ? 255ull : 65535ull) * W * H;
  if (S > top) return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": S " + std::to_string(S) + " is above the " + std::to_string(top) + " of a full-scale cell");
  *byte = light == SJPEG_HIP_LIGHT_CODED ? sjpeg_internal::resize_round(S, W, H) : sjpeg_internal::light_round(S, W, H, sjpeg_internal::kLightSrgb);
  return 0;
}

size_t sjpeg_hip_resize_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2]) {
  if (frames == nullptr) return 0;
  try {
    sjpeg_internal::ResizePlan plan;
    if (sjpeg_internal::resize_plan("sjpeg_hip_resize_ragged_bytes", format, nframes, frames, sizes, nullptr, &plan) != 0) return 0;
    return plan.bytes;
  } catch (...) {
    return 0;
  }
}

int sjpeg_hip_oriented_size(int width, int height, int orientation, int* ow, int* oh) {
  static const std::string who = "sjpeg_hip_oriented_size";
  if (ow == nullptr || oh == nullptr) return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": ow or oh == NULL");
  if (width < 1 || height < 1 || width > 65535 || height > 65535) {
    return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": bad dimensions " + std::to_string(width) + "x" + std::to_string(height));
  }
  if (orientation < 1 || orientation > 8) {
    return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": orientation " + std::to_string(orientation) + " is not one of 1..8 (EXIF tag 0x0112)");
  }
  uint32_t uw, uh;
  sjpeg_internal::oriented_size(static_cast<uint32_t>(width), static_cast<uint32_t>(height), orientation, &uw, &uh);
  *ow = static_cast<int>(uw);
  *oh = static_cast<int>(uh);
  return 0;
}

size_t sjpeg_hip_orient_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                                     const uint8_t* orientations) {
  if (frames == nullptr) return 0;
  try {
    sjpeg_internal::ResizePlan plan;
    if (sjpeg_internal::resize_plan("sjpeg_hip_orient_ragged_bytes", format, nframes, frames, sizes, orientations, &plan) != 0) return 0;
    return plan.bytes;
  } catch (...) {
    return 0;
  }
}

}  // extern "C"
