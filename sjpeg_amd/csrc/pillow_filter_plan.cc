// pillow_filter_plan.cc -- the host half of Pillow's BoxBlur, GaussianBlur and UnsharpMask (sjpeg_hip_filter_ragged_src
// and the _filtered_ entries; sjpeg_hip.h): the checks of the parameters, the weights of every axis -- the only float
// work there is, done here once --, and the plan: one descriptor per made picture, read off the made frames of the kind
// that made them, and the tile counts of the two launches pillow_filter.hip runs over them.  Plain C++, no device work:
// tests/cxx/pillow_filter_plan_test.cc compiles it as it is.
#include <math.h>
#include <stdint.h>

#include <string>

#include "pillow_filter_math.h"
#include "ragged_aux.h"
#include "sjpeg_hip.h"

namespace sjpeg_internal {

namespace {

// what is wrong with one axis of a kind, or "" -- the words behind "radius_x " / "radius_y "
std::string axis_refusal(int kind, float radius, PillowFilterAxis* axis) {
  if (!isfinite(radius) || radius < 0.0f) return "is not a finite number of 0 or more";
  *axis = pillow_filter_axis(kind, radius);
  if (axis->passes != 0 && axis->r > kPillowFilterRadiusMax) {
    return "gives a box radius above " + std::to_string(kPillowFilterRadiusMax) + " (Pillow has no such limit; this kernel's staging has)";
  }
  if (!pillow_filter_axis_bound(*axis)) return "gives weights above 2^24";
  return std::string();
}

// 0, or the refusal of one frame's filter (prefix: who and the frame)
int one_check(const std::string& prefix, const sjpeg_hip_pillow_filter& f, PillowFilterAxis axis[2]) {
  axis[0] = axis[1] = pillow_filter_axis(0, 0.0f);
  if (f.reserved[0] != 0 || f.reserved[1] != 0 || f.reserved[2] != 0 || f.reserved[3] != 0) {
    return set_error(SJPEG_HIP_EINVAL, prefix + "filter: reserved must be 0");
  }
  if (f.kind > 3) return set_error(SJPEG_HIP_EINVAL, prefix + "filter: kind " + std::to_string(f.kind) + " is not one of 0..3 (none, box, gaussian, unsharp mask)");
  if (f.kind == 0) return 0;
  const float radius[2] = {f.radius_x, f.radius_y};
  for (int a = 0; a < 2; ++a) {
    const std::string why = axis_refusal(f.kind, radius[a], &axis[a]);
    if (!why.empty()) return set_error(SJPEG_HIP_EINVAL, prefix + "filter: radius_" + (a == 0 ? "x " : "y ") + why);
  }
  if (f.kind == 3 && !(f.radius_x == f.radius_y)) {
    return set_error(SJPEG_HIP_EINVAL, prefix + "filter: an unsharp mask has one radius (radius_x must equal radius_y)");
  }
  return 0;
}

std::string frame_prefix(const std::string& who, int f, int per_frame) {
  return who + ": " + (per_frame != 0 ? "frame " + std::to_string(f) + ": " : std::string());
}

}  // namespace

int pillow_filter_check(const std::string& who, int nframes, const sjpeg_hip_pillow_filter* filter, int filter_per_frame) {
  if (filter == nullptr) return 0;
  const int n = filter_per_frame != 0 ? nframes : 1;
  PillowFilterAxis axis[2];
  for (int f = 0; f < n; ++f) {
    if (int rc = one_check(frame_prefix(who, f, filter_per_frame), filter[f], axis)) return rc;
  }
  return 0;
}

bool pillow_filter_all_none(int nframes, const sjpeg_hip_pillow_filter* filter, int filter_per_frame) {
  if (filter == nullptr) return true;
  const int n = filter_per_frame != 0 ? nframes : 1;
  for (int f = 0; f < n; ++f) {
    const sjpeg_hip_pillow_filter& p = filter[f];
    if (p.kind != 0 || p.reserved[0] != 0 || p.reserved[1] != 0 || p.reserved[2] != 0 || p.reserved[3] != 0) return false;
  }
  return true;
}

int pillow_filter_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* made, const uint8_t* base,
                       const sjpeg_hip_pillow_filter* filter, int filter_per_frame, PillowFilterPlan* plan) {
  *plan = PillowFilterPlan();
  if (format != SJPEG_HIP_SRC_RGB && format != SJPEG_HIP_SRC_GRAY) {
    return set_error(SJPEG_HIP_EINVAL, who + ": filter: made pictures of format " + std::to_string(format) + " are not filtered (RGB and gray ones are)");
  }
  const unsigned step = format == SJPEG_HIP_SRC_RGB ? 3u : 1u;
  plan->planes.reserve(static_cast<size_t>(nframes));
  unsigned long long tiles[2] = {0, 0};
  for (int f = 0; f < nframes; ++f) {
    const sjpeg_hip_ragged_frame& fr = made[f];
    const sjpeg_hip_pillow_filter none = {0, 0, 0, 0.0f, 0.0f, {0, 0, 0, 0}};
    const sjpeg_hip_pillow_filter& p = filter == nullptr ? none : filter[filter_per_frame != 0 ? f : 0];
    PillowFilterPlane d;
    // (a filter for the whole call is named without a frame, as the check alone names it)
    if (int rc = one_check(frame_prefix(who, f, filter_per_frame), p, d.axis)) { *plan = PillowFilterPlan(); return rc; }
    const uintptr_t off = reinterpret_cast<uintptr_t>(fr.plane[0]) - reinterpret_cast<uintptr_t>(base);
    d.made = reinterpret_cast<const uint8_t*>(off);
    d.mid = d.dst = reinterpret_cast<uint8_t*>(off);
    const int64_t stride = fr.row_stride[0];
    const int64_t row_bytes = static_cast<int64_t>(fr.width) * step;
    if (fr.width < 1 || fr.height < 1 || (off & 3u) != 0 || stride < ((row_bytes + 3) & ~int64_t(3)) || (stride & 3) != 0 || stride > 0x7fffffff) {
      *plan = PillowFilterPlan();
      return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": filter: the made picture is not rows of whole dwords");
    }
    d.width = static_cast<unsigned>(fr.width);
    d.rows = static_cast<unsigned>(fr.height);
    d.stride = static_cast<unsigned>(stride);
    d.step = step;
    d.kind = p.kind;
    d.percent = p.kind == 3 ? p.percent : 0u;
    d.threshold = p.kind == 3 ? p.threshold : 0u;
    d.tile_base[0] = static_cast<unsigned>(tiles[0]);
    d.tile_base[1] = static_cast<unsigned>(tiles[1]);
    tiles[0] += pillow_row_tiles(d.width, d.rows);
    tiles[1] += pillow_col_tiles(static_cast<unsigned>((row_bytes + 3) / 4), d.rows);
    if (tiles[0] > 0x7fffffffull || tiles[1] > 0x7fffffffull) {
      *plan = PillowFilterPlan();
      return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": the batch has too many tiles for one launch");
    }
    plan->planes.push_back(d);
  }
  plan->tiles[0] = static_cast<unsigned>(tiles[0]);
  plan->tiles[1] = static_cast<unsigned>(tiles[1]);
  return 0;
}

}  // namespace sjpeg_internal

extern "C" {

int sjpeg_hip_pillow_filter_weights(int kind, float radius, uint32_t* r, uint32_t* ww, uint32_t* fw, uint32_t* passes) {
  static const std::string who = "sjpeg_hip_pillow_filter_weights";
  using namespace sjpeg_internal;
  if (r == nullptr || ww == nullptr || fw == nullptr || passes == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": r, ww, fw or passes == NULL");
  if (kind < 1 || kind > 3) return set_error(SJPEG_HIP_EINVAL, who + ": kind " + std::to_string(kind) + " is not one of 1..3 (box, gaussian, unsharp mask)");
  PillowFilterAxis a;
  const std::string why = axis_refusal(kind, radius, &a);
  if (!why.empty()) return set_error(SJPEG_HIP_EINVAL, who + ": radius " + why);
  *r = a.r; *ww = a.ww; *fw = a.fw; *passes = a.passes;
  return 0;
}

}  // extern "C"
