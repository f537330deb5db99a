// unsharp_plan.cc -- the host half of the unsharp mask (sjpeg_hip_unsharp_ragged_src and the other _unsharp entries;
// sjpeg_hip.h): the checks of the parameters, the plan -- one descriptor per plane to write, made from the made pictures
// as frames of their made format, whichever plan made them, which unsharp.hip's kernel runs over -- and the formula on
// a single neighbourhood.  Plain C++, no device work: tests/cxx/unsharp_plan_test.cc compiles it as it is.
#include <stdint.h>

#include <string>

#include "ragged_aux.h"
#include "sjpeg_hip.h"
#include "unsharp_math.h"

namespace sjpeg_internal {

int unsharp_check(const std::string& who, int nframes, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame) {
  if (unsharp == nullptr) return 0;
  const int n = unsharp_per_frame != 0 ? nframes : 1;
  for (int f = 0; f < n; ++f) {
    if (unsharp[f].reserved[0] == 0 && unsharp[f].reserved[1] == 0) continue;
    return set_error(SJPEG_HIP_EINVAL, who + ": " + (unsharp_per_frame != 0 ? "frame " + std::to_string(f) + ": " : std::string()) +
                                           "unsharp: reserved must be 0");
  }
  return 0;
}

bool unsharp_all_zero(int nframes, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame) {
  if (unsharp == nullptr) return true;
  const int n = unsharp_per_frame != 0 ? nframes : 1;
  for (int f = 0; f < n; ++f) {
    if (unsharp[f].amount != 0 || unsharp[f].reserved[0] != 0 || unsharp[f].reserved[1] != 0) return false;
  }
  return true;
}

int unsharp_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* made, const uint8_t* base,
                 const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, UnsharpPlan* plan) {
  *plan = UnsharpPlan();
  if (int rc = unsharp_check(who, nframes, unsharp, unsharp_per_frame)) return rc;
  const bool planes3 = format == SJPEG_HIP_SRC_YUV420 || format == SJPEG_HIP_SRC_YUV444;
  if (!planes3 && format != SJPEG_HIP_SRC_RGB && format != SJPEG_HIP_SRC_GRAY) {
    return set_error(SJPEG_HIP_EINVAL, who + ": unsharp: made pictures of format " + std::to_string(format) + " are not sharpened");
  }
  const SourceLayout* const L = source_layout(format);
  const unsigned step = format == SJPEG_HIP_SRC_RGB ? 3u : 1u;
  plan->planes.reserve(static_cast<size_t>(nframes) * (planes3 ? 3u : 1u));
  unsigned long long tiles = 0;
  for (int f = 0; f < nframes; ++f) {
    const sjpeg_hip_ragged_frame& fr = made[f];
    const sjpeg_hip_unsharp u = unsharp == nullptr ? sjpeg_hip_unsharp{0, 0, {0, 0}} : unsharp[unsharp_per_frame != 0 ? f : 0];
    for (int c = 0; c < (planes3 ? 3 : 1); ++c) {
      int pw = fr.width, ph = fr.height;
      if (planes3) yuv_plane_dims(*L, fr.width, fr.height, c, &pw, &ph);
      UnsharpPlane d;
      const uintptr_t off = reinterpret_cast<uintptr_t>(fr.plane[c]) - reinterpret_cast<uintptr_t>(base);
      d.src = reinterpret_cast<const uint8_t*>(off);
      d.dst = reinterpret_cast<uint8_t*>(off);
      d.width_bytes = static_cast<unsigned>(pw) * step;
      d.rows = static_cast<unsigned>(ph);
      const int64_t stride = fr.row_stride[c];
      if (pw < 1 || ph < 1 || (off & 3u) != 0 || stride < static_cast<int64_t>((d.width_bytes + 3u) & ~3u) || (stride & 3) != 0 ||
          stride > 0x7fffffff) {
        *plan = UnsharpPlan();
        return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": unsharp: plane " + std::to_string(c) +
                                               " of the made picture is not rows of whole dwords");
      }
      d.src_stride = d.dst_stride = static_cast<unsigned>(stride);
      d.step = step;
      d.amount = c == 0 ? u.amount : 0u;                            // (U and V: copied)
      d.threshold = c == 0 ? u.threshold : 0u;
      d.tile_base = static_cast<unsigned>(tiles);
      const unsigned dwords = (d.width_bytes + 3u) / 4u;
      tiles += static_cast<unsigned long long>((dwords + kUnsharpTileDwords - 1) / kUnsharpTileDwords) *
               ((d.rows + kUnsharpTileRows - 1) / kUnsharpTileRows);
      if (tiles > 0x7fffffffull) {
        *plan = UnsharpPlan();
        return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": the batch has too many tiles for one launch");
      }
      plan->planes.push_back(d);
    }
  }
  plan->tiles = static_cast<unsigned>(tiles);
  return 0;
}

}  // namespace sjpeg_internal

extern "C" {

int sjpeg_hip_unsharp_sample(int amount, int threshold, const uint8_t n[9], uint32_t* byte) {
  static const std::string who = "sjpeg_hip_unsharp_sample";
  using sjpeg_internal::set_error;
  if (n == nullptr || byte == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": n or byte == NULL");
  if (amount < 0 || amount > 255) return set_error(SJPEG_HIP_EINVAL, who + ": amount " + std::to_string(amount) + " is not one of 0..255");
  if (threshold < 0 || threshold > 255) {
    return set_error(SJPEG_HIP_EINVAL, who + ": threshold " + std::to_string(threshold) + " is not one of 0..255");
  }
  *byte = static_cast<uint32_t>(sjpeg_internal::unsharp_sample(n, amount, threshold));
  return 0;
}

}  // extern "C"
