// yuv_colour_plan.cc -- the host half of the video colour conversion (sjpeg_hip_convert_ragged_yuv_src,
// sjpeg_hip_encode_ragged_yuv_converted_src and the _yuv_colour sheet entries; sjpeg_hip.h): the checks of the colours,
// the plan -- one descriptor per frame, made from the planes' plan of yuv_resize_plan.cc or the placed one of
// sheet_plan.cc, which yuv_colour.hip's kernel runs over -- and the formula on single samples.  Plain C++, no device
// work: tests/cxx/yuv_colour_plan_test.cc compiles it as it is.
#include <stdint.h>
#include <string.h>

#include <string>

#include "orient_math.h"
#include "ragged_aux.h"
#include "sjpeg_hip.h"
#include "yuv_colour_math.h"

namespace sjpeg_internal {

// a colour the entries take: both fields 0..1, nothing in `reserved`
static bool colour_ok(const sjpeg_hip_yuv_colour& c) { return c.matrix <= 1 && c.range <= 1 && c.reserved[0] == 0 && c.reserved[1] == 0; }

int yuv_colour_check(const std::string& who, int nframes, const sjpeg_hip_yuv_colour* colour, int colour_per_frame) {
  if (colour == nullptr) return 0;
  const int n = colour_per_frame != 0 ? nframes : 1;
  for (int f = 0; f < n; ++f) {
    const sjpeg_hip_yuv_colour& c = colour[f];
    if (colour_ok(c)) continue;
    const std::string where = who + ": " + (colour_per_frame != 0 ? "frame " + std::to_string(f) + ": " : std::string()) + "colour: ";
    if (c.matrix > 1) {
      return set_error(SJPEG_HIP_EINVAL, where + "matrix " + std::to_string(c.matrix) + " is not one of 0..1 (SJPEG_HIP_MATRIX_BT601, _BT709)");
    }
    if (c.range > 1) {
      return set_error(SJPEG_HIP_EINVAL, where + "range " + std::to_string(c.range) + " is not one of 0..1 (SJPEG_HIP_RANGE_FULL, _LIMITED)");
    }
    return set_error(SJPEG_HIP_EINVAL, where + "reserved must be 0");
  }
  return 0;
}

bool yuv_colour_all_identity(int nframes, const sjpeg_hip_yuv_colour* colour, int colour_per_frame) {
  if (colour == nullptr) return true;
  const int n = colour_per_frame != 0 ? nframes : 1;
  for (int f = 0; f < n; ++f) {
    if (!colour_ok(colour[f]) || !yuv_colour_is_identity(colour[f].matrix, colour[f].range)) return false;
  }
  return true;
}

int yuv_colour_plan(const std::string& who, const YuvResizePlan& planes, const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                    YuvColourPlan* plan) {
  *plan = YuvColourPlan();
  const int nframes = planes.nframes;
  if (int rc = yuv_colour_check(who, nframes, colour, colour_per_frame)) return rc;
  plan->frames.assign(static_cast<size_t>(nframes), YuvColourFrame());
  unsigned long long tiles = 0;
  size_t k = 0;
  for (int f = 0; f < nframes; ++f) {
    YuvColourFrame& c = plan->frames[static_cast<size_t>(f)];
    memset(&c, 0, sizeof(c));
    // the frame's descriptors in a row: Y, then U and V, or the pair
    const YuvPlane& py = planes.planes[k];
    const YuvPlane& pu = planes.planes[k + 1];
    const bool pair = pu.channels == 2;
    const ResizeFrame& pv = pair ? pu.r : planes.planes[k + 2].r;
    k += pair ? 2 : 3;
    const bool placed = (py.r.orient & kResizePlaced) != 0;
    const int orient = static_cast<int>(py.r.orient & ~kResizePlaced);
    plan->placed = plan->placed || placed;
    uint32_t uw, uh, cw, ch;
    oriented_size(static_cast<uint32_t>(py.r.w2), static_cast<uint32_t>(py.r.h2), orient, &uw, &uh);
    oriented_size(static_cast<uint32_t>(pu.r.w2), static_cast<uint32_t>(pu.r.h2), orient, &cw, &ch);
    c.y = py.r.dst;
    c.u = pu.r.dst;
    c.v = pair ? pu.dst2 : pv.dst;
    c.y_stride = py.r.dst_stride;
    c.c_stride = pu.r.dst_stride;                                  // (V's plane is laid out as U's)
    c.uw = static_cast<int>(uw); c.uh = static_cast<int>(uh);
    c.cw = static_cast<int>(cw); c.ch = static_cast<int>(ch);
    c.s = planes.resized_format == SJPEG_HIP_SRC_YUV444 ? 1 : 2;
    // (a placed plane starts at any byte of its sheet plane; the sheet planes start at multiples of 16 and their rows
    // are whole dwords apart, so the offset from the buffer's start has the address's low bits, in every row)
    c.lead = placed ? static_cast<int>(reinterpret_cast<uintptr_t>(c.u) & 3u) : 0;
    c.groups = (static_cast<unsigned>(c.lead) + cw + 3u) / 4u;
    const sjpeg_hip_yuv_colour col = colour == nullptr ? sjpeg_hip_yuv_colour{0, 0, {0, 0}} : colour[colour_per_frame != 0 ? f : 0];
    c.table = yuv_colour_table(col.matrix, col.range);
    c.tile_base = static_cast<unsigned>(tiles);
    if (!yuv_colour_is_identity(col.matrix, col.range)) tiles += (static_cast<unsigned long long>(c.groups) * ch + 255u) / 256u;
    if (tiles > 0x7fffffffull) {
      *plan = YuvColourPlan();
      return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": the batch has too many tiles for one launch");
    }
  }
  plan->tiles = static_cast<unsigned>(tiles);
  return 0;
}

}  // namespace sjpeg_internal

extern "C" {

int sjpeg_hip_yuv_colour_samples(const sjpeg_hip_yuv_colour* colour, size_t n, const uint8_t (*yuv_in)[3], uint8_t (*yuv_out)[3]) {
  static const std::string who = "sjpeg_hip_yuv_colour_samples";
  using namespace sjpeg_internal;
  try {
    if (colour == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": colour == NULL");
    if (int rc = yuv_colour_check(who, 1, colour, 0)) return rc;
    if (n != 0 && (yuv_in == nullptr || yuv_out == nullptr)) return set_error(SJPEG_HIP_EINVAL, who + ": yuv_in or yuv_out == NULL");
    const YuvColourTable t = yuv_colour_table(colour->matrix, colour->range);
    for (size_t i = 0; i < n; ++i) {
      const int32_t y = yuv_in[i][0], u = static_cast<int32_t>(yuv_in[i][1]) - 128, v = static_cast<int32_t>(yuv_in[i][2]) - 128;
      yuv_out[i][0] = static_cast<uint8_t>(yuv_colour_luma(t, y, u, v));
      yuv_out[i][1] = static_cast<uint8_t>(yuv_colour_chroma(t, 1, u, v));
      yuv_out[i][2] = static_cast<uint8_t>(yuv_colour_chroma(t, 2, u, v));
    }
    return 0;
  } catch (...) {
    return set_error(SJPEG_HIP_ENOMEM, who + ": out of host memory");
  }
}

}  // extern "C"
