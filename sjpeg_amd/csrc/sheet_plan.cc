// sheet_plan.cc -- the host half of the contact sheets (sjpeg_hip_sheet_ragged_src, sjpeg_hip_encode_ragged_sheet_src;
// sjpeg_hip.h): the sheet's size and checks, the place of every thumbnail, and the plan.  The thumbnails are planned
// by resize_plan / yuv_resize_plan -- their checks, their tile rule, their descriptors --; what is added here is where
// each one lands: every descriptor's dst (and dst2) is rewritten to the thumbnail's first sample inside its sheet
// plane, its dst_stride to that plane's, and it is marked kResizePlaced.  Plain C++, no device work: a host compiler
// reads it as it is (tests/cxx/sheet_plan_test.cc), like yuv_resize_plan.cc.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "orient_math.h"
#include "ragged_aux.h"
#include "reduce_round.h"
#include "sjpeg_hip.h"
#include "source_layout.h"

namespace sjpeg_internal {

int sheet_check(const std::string& who, const sjpeg_hip_sheet* sheet, int format, int* width, int* height) {
  const SourceLayout* const L = source_layout(format);
  if (L == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": unknown source format");
  if (sheet == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": sheet == NULL");
  const sjpeg_hip_sheet& s = *sheet;
  struct Field { const char* name; int32_t v, lo; };
  const Field fields[6] = {{"cols", s.cols, 1},   {"rows", s.rows, 1},     {"cell_width", s.cell_width, 1}, {"cell_height", s.cell_height, 1},
                           {"gutter", s.gutter, 0}, {"margin", s.margin, 0}};
  for (const Field& f : fields) {
    if (f.v < f.lo || f.v > 65535) {
      return set_error(SJPEG_HIP_EINVAL, who + ": sheet: " + f.name + " " + std::to_string(f.v) + " is not one of " + std::to_string(f.lo) + "..65535");
    }
  }
  if (s.reserved != 0) return set_error(SJPEG_HIP_EINVAL, who + ": sheet: reserved must be 0");
  const long long sw = 2ll * s.margin + 1ll * s.cols * s.cell_width + (s.cols - 1ll) * s.gutter;
  const long long sh = 2ll * s.margin + 1ll * s.rows * s.cell_height + (s.rows - 1ll) * s.gutter;
  if (sw > 65535 || sh > 65535) {
    return set_error(SJPEG_HIP_EINVAL, who + ": sheet: the sheet would be " + std::to_string(sw) + "x" + std::to_string(sh) + ", above 65535");
  }
  if (L->implied == SJPEG_HIP_YUV420) {
    for (int k = 2; k < 6; ++k) {
      if (fields[k].v % 2 != 0) {
        return set_error(SJPEG_HIP_EINVAL, who + ": sheet: " + fields[k].name + " " + std::to_string(fields[k].v) + " is odd: a 4:2:0 format (" +
                                               source_format_name(format) + ") takes even cell_width, cell_height, gutter and margin (chroma lands at half the luma's place)");
      }
    }
  }
  *width = static_cast<int>(sw);
  *height = static_cast<int>(sh);
  return 0;
}

int sheet_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_sheet* sheet,
               const int32_t (*sizes)[2], const uint8_t* orientations, SheetPlan* plan, const sjpeg_hip_flatten* flatten,
               const sjpeg_hip_yuv_depth* depth) {
  int SW = 0, SH = 0;
  if (int rc = sheet_check(who, sheet, format, &SW, &SH)) return rc;
  const SourceLayout* const L = source_layout(format);
  if (frames == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": frames == NULL");
  if (nframes < 1 || nframes > 65535) return set_error(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
  if (flatten != nullptr) { if (int rc = flatten_check(who, format, *flatten)) return rc; }   // (a YUV-plane format falls here)
  const sjpeg_hip_sheet& s = *sheet;
  const bool yuv = L->cls == kSrcPlanes && L->planes >= 2;         // luma and chroma planes of bytes: the per-plane plan
  const bool half = L->implied == SJPEG_HIP_YUV420;
  // sizes == NULL: every frame fitted into its cell, the box turned with the frame (a frame the plans refuse keeps its
  // own size: they say what is wrong with it)
  std::vector<int32_t> fitted;
  if (sizes == nullptr) {
    fitted.assign(static_cast<size_t>(nframes) * 2, 0);
    for (int f = 0; f < nframes; ++f) {
      const bool turned = orientations != nullptr && orient_transposes(orientations[f]);
      int w = frames[f].width, h = frames[f].height;
      sjpeg_hip_fit_size(w, h, turned ? s.cell_height : s.cell_width, turned ? s.cell_width : s.cell_height, &w, &h);
      fitted[2 * f] = w; fitted[2 * f + 1] = h;
    }
    sizes = reinterpret_cast<const int32_t (*)[2]>(fitted.data());
  }
  *plan = SheetPlan();
  if (yuv) {
    if (int rc = yuv_resize_plan(who, format, nframes, frames, sizes, orientations, &plan->planes, depth)) return rc;
  } else {
    if (int rc = resize_plan(who, format, nframes, frames, sizes, orientations, &plan->rgb, flatten)) return rc;
  }
  const int channels = yuv ? 1 : plan->rgb.resized_format == SJPEG_HIP_SRC_RGB ? 3 : 1;
  const long long per_sheet = 1ll * s.cols * s.rows;
  plan->format = format;
  plan->out_format = yuv ? plan->planes.resized_format : plan->rgb.resized_format;
  plan->yuv = yuv;
  plan->nframes = nframes;
  plan->nsheets = static_cast<int>((nframes + per_sheet - 1) / per_sheet);
  plan->width = SW; plan->height = SH;
  // the sheet's planes: the layout of the resized pictures, a sheet a picture
  SheetFill& fill = plan->fill;
  fill.nsheets = plan->nsheets;
  fill.nplanes = yuv ? 3 : 1;
  unsigned stride[3] = {0, 0, 0};
  size_t at = 0;
  for (int c = 0; c < fill.nplanes; ++c) {
    const int pw = c > 0 && half ? SW / 2 : SW, ph = c > 0 && half ? SH / 2 : SH;
    stride[c] = static_cast<unsigned>(reduced_row_stride(pw, channels));
    fill.off[c] = at;
    fill.rows[c] = static_cast<unsigned>(ph);
    fill.row_dwords[c] = stride[c] / 4u;
    at += reduced_picture_bytes(pw, ph, channels);
    for (int k = 0; k < 3; ++k) {
      uint32_t dword = 0;
      for (int b = 0; b < 4; ++b) dword |= static_cast<uint32_t>(s.background[channels == 3 ? (4 * k + b) % 3 : c]) << (8 * b);
      fill.pattern[c][k] = dword;
    }
  }
  fill.sheet_bytes = at;
  plan->bytes = at * static_cast<size_t>(plan->nsheets);
  // every thumbnail held to its cell and given its place
  plan->places.assign(static_cast<size_t>(nframes), SheetPlace());
  for (int f = 0; f < nframes; ++f) {
    const int o = orientations != nullptr ? orientations[f] : 1;
    uint32_t uw, uh;
    oriented_size(static_cast<uint32_t>(sizes[f][0]), static_cast<uint32_t>(sizes[f][1]), o, &uw, &uh);
    if (uw > static_cast<uint32_t>(s.cell_width) || uh > static_cast<uint32_t>(s.cell_height)) {
      *plan = SheetPlan();
      return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": the thumbnail of size " + std::to_string(sizes[f][0]) + "x" +
                                             std::to_string(sizes[f][1]) + ", " + std::to_string(uw) + "x" + std::to_string(uh) + " upright (orientation " +
                                             std::to_string(o) + "), is above the cell's " + std::to_string(s.cell_width) + "x" + std::to_string(s.cell_height));
    }
    const int k = static_cast<int>(f % per_sheet), i = k % s.cols, j = k / s.cols;
    int ex = (s.cell_width - static_cast<int>(uw)) / 2, ey = (s.cell_height - static_cast<int>(uh)) / 2;
    if (half) { ex &= ~1; ey &= ~1; }
    SheetPlace& p = plan->places[f];
    p.sheet = static_cast<int32_t>(f / per_sheet);
    p.x0 = s.margin + i * (s.cell_width + s.gutter) + ex;
    p.y0 = s.margin + j * (s.cell_height + s.gutter) + ey;
    p.uw = static_cast<int32_t>(uw); p.uh = static_cast<int32_t>(uh);
  }
  // ... and the descriptors rewritten: dst the thumbnail's first sample inside its sheet plane, counted from the
  // buffer's start as the plans count; dst_stride the sheet plane's
  auto placed = [&](const SheetPlace& p, int c) -> uint8_t* {
    const size_t x = c > 0 && half ? p.x0 / 2 : p.x0, y = c > 0 && half ? p.y0 / 2 : p.y0;
    return reinterpret_cast<uint8_t*>(static_cast<size_t>(p.sheet) * fill.sheet_bytes + fill.off[c] + y * stride[c] + x * channels);
  };
  if (yuv) {
    int c = 0;
    for (size_t k = 0; k < plan->planes.planes.size(); ++k) {
      YuvPlane& yp = plan->planes.planes[k];
      c = k > 0 && plan->planes.planes[k - 1].frame == yp.frame ? c + 1 : 0;       // (a frame's descriptors in a row: Y, U, V or Y, UV)
      yp.r.dst = placed(plan->places[yp.frame], c);
      yp.r.dst_stride = stride[c];
      if (yp.channels == 2) yp.dst2 = placed(plan->places[yp.frame], 2);           // (V's sheet plane is laid out as U's)
      yp.r.orient |= kResizePlaced;
    }
    plan->planes.bytes = plan->bytes;
  } else {
    for (int f = 0; f < nframes; ++f) {
      ResizeFrame& d = plan->rgb.frames[f];
      d.dst = placed(plan->places[f], 0);
      d.dst_stride = stride[0];
      d.orient |= kResizePlaced;
    }
    plan->rgb.bytes = plan->bytes;
  }
  return 0;
}

void sheet_plan_frames(const SheetPlan& plan, uint8_t* base, sjpeg_hip_ragged_frame* out) {
  for (int s = 0; s < plan.nsheets; ++s) {
    sjpeg_hip_ragged_frame r;
    memset(&r, 0, sizeof(r));
    r.width = plan.width; r.height = plan.height;
    for (int c = 0; c < plan.fill.nplanes; ++c) {
      r.plane[c] = base + static_cast<size_t>(s) * plan.fill.sheet_bytes + plan.fill.off[c];
      r.row_stride[c] = static_cast<int64_t>(plan.fill.row_dwords[c]) * 4;
    }
    out[s] = r;
  }
}

}  // namespace sjpeg_internal

extern "C" {

int sjpeg_hip_sheet_size(const sjpeg_hip_sheet* sheet, int format, int* width, int* height) {
  static const std::string who = "sjpeg_hip_sheet_size";
  if (width == nullptr || height == nullptr) return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": width or height == NULL");
  try {
    return sjpeg_internal::sheet_check(who, sheet, format, width, height);
  } catch (...) {
    return sjpeg_internal::set_error(SJPEG_HIP_ENOMEM, who + ": out of host memory");
  }
}

int sjpeg_hip_sheet_places(int format, int nframes, const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_sheet* sheet,
                           const int32_t (*sizes)[2], const uint8_t* orientations, int32_t (*places)[5]) {
  static const std::string who = "sjpeg_hip_sheet_places";
  if (places == nullptr) return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": places == NULL");
  try {
    sjpeg_internal::SheetPlan plan;
    if (int rc = sjpeg_internal::sheet_plan(who, format, nframes, frames, sheet, sizes, orientations, &plan)) return rc;
    for (int f = 0; f < nframes; ++f) {
      const sjpeg_internal::SheetPlace& p = plan.places[f];
      places[f][0] = p.sheet; places[f][1] = p.x0; places[f][2] = p.y0; places[f][3] = p.uw; places[f][4] = p.uh;
    }
    return 0;
  } catch (...) {
    return sjpeg_internal::set_error(SJPEG_HIP_ENOMEM, who + ": out of host memory");
  }
}

size_t sjpeg_hip_sheet_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_sheet* sheet,
                                    const int32_t (*sizes)[2], const uint8_t* orientations) {
  try {
    sjpeg_internal::SheetPlan plan;
    if (sjpeg_internal::sheet_plan("sjpeg_hip_sheet_ragged_bytes", format, nframes, frames, sheet, sizes, orientations, &plan) != 0) return 0;
    return plan.bytes;
  } catch (...) {
    return 0;
  }
}

}  // extern "C"
