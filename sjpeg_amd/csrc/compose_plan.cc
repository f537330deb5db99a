// compose_plan.cc -- the host half of the compose stage (sjpeg_hip_compose_ragged_src and the _composed_ entries;
// sjpeg_hip.h): the checks of the structs, the overlays and the places, Pillow's rules of size and place -- the only
// double work there is, done here once --, and the plan: one descriptor per canvas over the made pictures of the kind
// that made them, its places resolved to canvas coordinates, and the tile count of the launch compose.hip runs over
// them.  Plain C++, no device work: tests/cxx/compose_plan_test.cc compiles it as it is.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "compose_math.h"
#include "ragged_aux.h"
#include "reduce_round.h"
#include "sjpeg_hip.h"

namespace sjpeg_internal {

namespace {

std::string frame_prefix(const std::string& who, int f, int per_frame) {
  return who + ": " + (per_frame != 0 ? "frame " + std::to_string(f) + ": " : std::string());
}

bool reserved_clear(const sjpeg_hip_compose& c) { return c.reserved[0] == 0 && c.reserved[1] == 0 && c.reserved[2] == 0 && c.reserved[3] == 0; }

// 0, or the refusal of one frame's struct by what it says alone (prefix: who and the frame)
int one_check(const std::string& prefix, const sjpeg_hip_compose& c, int nplaces) {
  if (!reserved_clear(c)) return set_error(SJPEG_HIP_EINVAL, prefix + "compose: reserved must be 0");
  if (c.mode > 1) return set_error(SJPEG_HIP_EINVAL, prefix + "compose: mode " + std::to_string(c.mode) + " is not 0 (at px, py) or 1 (by the centering)");
  const bool own = c.canvas_width == 0 && c.canvas_height == 0;
  if (!own && (c.canvas_width < 1 || c.canvas_width > 65535 || c.canvas_height < 1 || c.canvas_height > 65535)) {
    return set_error(SJPEG_HIP_EINVAL, prefix + "compose: canvas " + std::to_string(c.canvas_width) + "x" + std::to_string(c.canvas_height) +
                                           " is not 0x0 (the picture's own size) or 1..65535 a side");
  }
  if (c.mode == 1 && !(isfinite(c.cx) && isfinite(c.cy))) return set_error(SJPEG_HIP_EINVAL, prefix + "compose: the centering is not finite");
  if (c.first_place < 0 || c.nplaces < 0 || static_cast<int64_t>(c.first_place) + c.nplaces > nplaces) {
    return set_error(SJPEG_HIP_EINVAL, prefix + "compose: places " + std::to_string(c.first_place) + " .. " +
                                           std::to_string(static_cast<int64_t>(c.first_place) + c.nplaces) + " are not within the call's " +
                                           std::to_string(nplaces) + " places");
  }
  if (c.nplaces > kComposePlacesMax) {
    return set_error(SJPEG_HIP_EINVAL, prefix + "compose: " + std::to_string(c.nplaces) + " places are more than " + std::to_string(kComposePlacesMax));
  }
  return 0;
}

}  // namespace

int compose_check(const std::string& who, int nframes, const sjpeg_hip_compose* compose, int compose_per_frame, const sjpeg_hip_overlay* overlays,
                  int noverlays, const sjpeg_hip_overlay_place* places, int nplaces) {
  if (noverlays < 0 || (noverlays > 0 && overlays == nullptr)) return set_error(SJPEG_HIP_EINVAL, who + ": overlays == NULL or noverlays is negative");
  if (nplaces < 0 || (nplaces > 0 && places == nullptr)) return set_error(SJPEG_HIP_EINVAL, who + ": places == NULL or nplaces is negative");
  for (int o = 0; o < noverlays; ++o) {
    const sjpeg_hip_overlay& v = overlays[o];
    const std::string prefix = who + ": overlay " + std::to_string(o) + ": ";
    if (v.rgba == nullptr) return set_error(SJPEG_HIP_EINVAL, prefix + "rgba == NULL");
    if ((reinterpret_cast<uintptr_t>(v.rgba) & 3u) != 0) return set_error(SJPEG_HIP_EINVAL, prefix + "rgba must be a multiple of 4");
    if (v.width < 1 || v.width > 65535 || v.height < 1 || v.height > 65535) {
      return set_error(SJPEG_HIP_EINVAL, prefix + "width " + std::to_string(v.width) + " or height " + std::to_string(v.height) + " is not one of 1..65535");
    }
    if (v.stride < 4 * static_cast<int64_t>(v.width) || (v.stride & 3) != 0 || v.stride > 0x7fffffff) {
      return set_error(SJPEG_HIP_EINVAL, prefix + "stride " + std::to_string(v.stride) + " is below 4 * width or not a multiple of 4");
    }
  }
  for (int i = 0; i < nplaces; ++i) {
    const sjpeg_hip_overlay_place& p = places[i];
    const std::string prefix = who + ": place " + std::to_string(i) + ": ";
    if (p.reserved[0] != 0 || p.reserved[1] != 0 || p.reserved[2] != 0) return set_error(SJPEG_HIP_EINVAL, prefix + "reserved must be 0");
    if (p.anchor >= kComposeAnchors) {
      return set_error(SJPEG_HIP_EINVAL, prefix + "anchor " + std::to_string(p.anchor) + " is not one of 0..4 (top-left, top-right, bottom-left, bottom-right, centre)");
    }
    if (p.overlay < 0 || p.overlay >= noverlays) {
      return set_error(SJPEG_HIP_EINVAL, prefix + "overlay " + std::to_string(p.overlay) + " is not one of the call's " + std::to_string(noverlays) + " overlays");
    }
  }
  if (compose == nullptr) return 0;
  const int n = compose_per_frame != 0 ? nframes : 1;
  for (int f = 0; f < n; ++f) {
    if (int rc = one_check(frame_prefix(who, f, compose_per_frame), compose[f], nplaces)) return rc;
  }
  return 0;
}

bool compose_all_none(int nframes, const sjpeg_hip_compose* compose, int compose_per_frame) {
  if (compose == nullptr) return true;
  const int n = compose_per_frame != 0 ? nframes : 1;
  for (int f = 0; f < n; ++f) {
    const sjpeg_hip_compose& c = compose[f];
    if (c.canvas_width != 0 || c.canvas_height != 0 || c.nplaces != 0 || c.mode > 1 || !reserved_clear(c)) return false;
    if (c.mode == 0 && (c.px != 0 || c.py != 0)) return false;
    if (c.mode == 1 && !(isfinite(c.cx) && isfinite(c.cy))) return false;
  }
  return true;
}

int compose_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* made, const uint8_t* base,
                 const sjpeg_hip_compose* compose, int compose_per_frame, const sjpeg_hip_overlay* overlays, int noverlays,
                 const sjpeg_hip_overlay_place* places, int nplaces, ComposePlan* plan) {
  *plan = ComposePlan();
  if (int rc = compose_check(who, nframes, compose, compose_per_frame, overlays, noverlays, places, nplaces)) return rc;
  if (format != SJPEG_HIP_SRC_RGB && format != SJPEG_HIP_SRC_GRAY) {
    return set_error(SJPEG_HIP_EINVAL, who + ": compose: made pictures of format " + std::to_string(format) + " are not composed (RGB and gray ones are)");
  }
  const unsigned step = format == SJPEG_HIP_SRC_RGB ? 3u : 1u;
  plan->frames.reserve(static_cast<size_t>(nframes));
  unsigned long long tiles = 0;
  size_t at = 0;
  sjpeg_hip_compose none;
  memset(&none, 0, sizeof(none));
  for (int f = 0; f < nframes; ++f) {
    const sjpeg_hip_ragged_frame& fr = made[f];
    const sjpeg_hip_compose& c = compose == nullptr ? none : compose[compose_per_frame != 0 ? f : 0];
    const std::string prefix = who + ": frame " + std::to_string(f) + ": compose: ";
    ComposeFrame d;
    memset(&d, 0, sizeof(d));
    const uintptr_t off = reinterpret_cast<uintptr_t>(fr.plane[0]) - reinterpret_cast<uintptr_t>(base);
    const int64_t stride = fr.row_stride[0];
    const int64_t row_bytes = static_cast<int64_t>(fr.width) * step;
    if (fr.width < 1 || fr.height < 1 || fr.width > 65535 || fr.height > 65535 || (off & 3u) != 0 || stride < ((row_bytes + 3) & ~int64_t(3)) ||
        (stride & 3) != 0 || stride > 0x7fffffff) {
      *plan = ComposePlan();
      return set_error(SJPEG_HIP_EINVAL, prefix + "the made picture is not rows of whole dwords");
    }
    const bool own = c.canvas_width == 0 && c.canvas_height == 0;
    const int cw = own ? fr.width : c.canvas_width, ch = own ? fr.height : c.canvas_height;
    long long px = c.px, py = c.py;
    if (c.mode == 1) {
      // (a picture larger than its canvas has no place by the rule: refused below by a place that is outside)
      px = fr.width <= cw ? compose_pad_offset(cw, fr.width, c.cx) : -1;
      py = fr.height <= ch ? compose_pad_offset(ch, fr.height, c.cy) : -1;
    }
    if (px < 0 || py < 0 || px + fr.width > cw || py + fr.height > ch) {
      *plan = ComposePlan();
      return set_error(SJPEG_HIP_EINVAL, prefix + "the " + std::to_string(fr.width) + "x" + std::to_string(fr.height) + " picture" +
                                             (c.mode == 0 ? " at (" + std::to_string(px) + ", " + std::to_string(py) + ")" : std::string()) +
                                             " is not wholly inside the " + std::to_string(cw) + "x" + std::to_string(ch) + " canvas");
    }
    d.made = reinterpret_cast<const uint8_t*>(off);
    d.dst = reinterpret_cast<uint8_t*>(at);
    d.cw = static_cast<unsigned>(cw); d.ch = static_cast<unsigned>(ch);
    d.w = static_cast<unsigned>(fr.width); d.h = static_cast<unsigned>(fr.height);
    d.px = static_cast<unsigned>(px); d.py = static_cast<unsigned>(py);
    d.src_stride = static_cast<unsigned>(stride);
    d.dst_stride = static_cast<unsigned>(reduced_row_stride(cw, static_cast<int>(step)));
    d.step = step;
    d.colour = static_cast<unsigned>(c.colour[0]) | static_cast<unsigned>(c.colour[1]) << 8 | static_cast<unsigned>(c.colour[2]) << 16;
    for (int i = 0; i < c.nplaces; ++i) {
      const sjpeg_hip_overlay_place& p = places[c.first_place + i];
      const sjpeg_hip_overlay& v = overlays[p.overlay];
      long long ox, oy;
      compose_anchor(p.anchor, cw, ch, v.width, v.height, p.x, p.y, &ox, &oy);
      if (ox >= cw || oy >= ch || ox + v.width <= 0 || oy + v.height <= 0) continue;      // wholly outside: it does nothing
      ComposePlace& q = d.place[d.nplaces++];
      q.rgba = static_cast<const uint8_t*>(v.rgba);
      q.ox = static_cast<int>(ox); q.oy = static_cast<int>(oy);
      q.ow = static_cast<unsigned>(v.width); q.oh = static_cast<unsigned>(v.height);
      q.stride = static_cast<unsigned>(v.stride);
    }
    if (d.nplaces != 0 || d.cw != d.w || d.ch != d.h) plan->identity = false;
    d.tile_base = static_cast<unsigned>(tiles);
    tiles += compose_tiles(d.dst_stride / 4, d.ch);
    if (tiles > 0x7fffffffull) {
      *plan = ComposePlan();
      return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": the batch has too many tiles for one launch");
    }
    at += reduced_picture_bytes(cw, ch, static_cast<int>(step));
    plan->frames.push_back(d);
  }
  plan->tiles = static_cast<unsigned>(tiles);
  plan->bytes = at;
  return 0;
}

void compose_plan_frames(const ComposePlan& plan, const sjpeg_hip_ragged_frame* frames, uint8_t* base, sjpeg_hip_ragged_frame* out) {
  for (size_t f = 0; f < plan.frames.size(); ++f) {
    const ComposeFrame& d = plan.frames[f];
    sjpeg_hip_ragged_frame r;
    memset(&r, 0, sizeof(r));
    r.plane[0] = base + reinterpret_cast<uintptr_t>(d.dst);
    r.row_stride[0] = static_cast<int64_t>(d.dst_stride);
    r.width = static_cast<int32_t>(d.cw); r.height = static_cast<int32_t>(d.ch);
    r.out_offset = frames[f].out_offset; r.out_capacity = frames[f].out_capacity;
    out[f] = r;
  }
}

}  // namespace sjpeg_internal

extern "C" {

int sjpeg_hip_contain_size(int width, int height, int box_width, int box_height, int32_t* out) {
  static const std::string who = "sjpeg_hip_contain_size";
  using namespace sjpeg_internal;
  if (out == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": out == NULL");
  if (width < 1 || height < 1 || width > 65535 || height > 65535 || box_width < 1 || box_height < 1 || box_width > 65535 || box_height > 65535) {
    return set_error(SJPEG_HIP_EINVAL, who + ": the picture " + std::to_string(width) + "x" + std::to_string(height) + " or the box " +
                                           std::to_string(box_width) + "x" + std::to_string(box_height) + " has a side that is not one of 1..65535");
  }
  long long w, h;
  compose_contain_size(width, height, box_width, box_height, &w, &h);
  if (w < 1 || h < 1) {
    return set_error(SJPEG_HIP_EINVAL, who + ": a " + std::to_string(width) + "x" + std::to_string(height) + " picture contained in " +
                                           std::to_string(box_width) + "x" + std::to_string(box_height) + " has a side of 0 (Pillow raises)");
  }
  out[0] = static_cast<int32_t>(w); out[1] = static_cast<int32_t>(h);
  return 0;
}

int sjpeg_hip_pad_place(int width, int height, int canvas_width, int canvas_height, double cx, double cy, int32_t* out) {
  static const std::string who = "sjpeg_hip_pad_place";
  using namespace sjpeg_internal;
  if (out == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": out == NULL");
  if (!(isfinite(cx) && isfinite(cy))) return set_error(SJPEG_HIP_EINVAL, who + ": the centering is not finite");
  if (width < 1 || height < 1 || canvas_width > 65535 || canvas_height > 65535 || width > canvas_width || height > canvas_height) {
    return set_error(SJPEG_HIP_EINVAL, who + ": the " + std::to_string(width) + "x" + std::to_string(height) + " picture is not wholly inside the " +
                                           std::to_string(canvas_width) + "x" + std::to_string(canvas_height) + " canvas");
  }
  out[0] = static_cast<int32_t>(compose_pad_offset(canvas_width, width, cx));
  out[1] = static_cast<int32_t>(compose_pad_offset(canvas_height, height, cy));
  return 0;
}

int sjpeg_hip_compose_sample(int dst, int r, int g, int b, int a, int gray) {
  using namespace sjpeg_internal;
  const uint32_t src = gray != 0 ? compose_luma(r & 255, g & 255, b & 255) : static_cast<uint32_t>(r & 255);
  return static_cast<int>(compose_blend(static_cast<uint32_t>(dst & 255), src, static_cast<uint32_t>(a & 255)));
}

}  // extern "C"
