// resample_plan.cc -- the host half of resampling with Pillow's filters (sjpeg_hip_resample_ragged_src and the
// _resampled_ entries; sjpeg_hip.h): the checks of the parameters, the tables -- built in double by resample_math.h,
// once per (filter, in, out) of a call, each held to the two bounds the kernel relies on -- and the plan, one descriptor
// per frame, that resample.hip's kernel runs over.  Plain C++, no device work: tests/cxx/resample_plan_test.cc compiles
// it as it is.
#include <stdint.h>
#include <string.h>

#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "orient_math.h"
#include "ragged_aux.h"
#include "reduce_round.h"
#include "resample_math.h"
#include "sjpeg_hip.h"
#include "source_layout.h"

namespace {

using sjpeg_internal::ResampleFrame;
using sjpeg_internal::set_error;

const char* const kFilterNames[sjpeg_internal::kResampleFilters] = {"SJPEG_HIP_RESAMPLE_BOX", "SJPEG_HIP_RESAMPLE_BILINEAR", "SJPEG_HIP_RESAMPLE_HAMMING",
                                                                    "SJPEG_HIP_RESAMPLE_BICUBIC", "SJPEG_HIP_RESAMPLE_LANCZOS"};

// a format the kernel reads: every RGB-like row of the table and the gray ones
bool resamplable(const sjpeg_internal::SourceLayout& L) { return L.rgb_like || (L.planes == 1 && L.implied == SJPEG_HIP_YUV400); }

struct TableAt { size_t bounds, K; int ksize; };      // where a table lies among the call's, in int32s

}  // namespace

namespace sjpeg_internal {

int resample_check(const std::string& who, int nframes, const sjpeg_hip_resample* resample, int resample_per_frame) {
  if (resample == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": resample == NULL");
  const int n = resample_per_frame != 0 ? nframes : 1;
  for (int f = 0; f < n; ++f) {
    const std::string frame = who + ": " + (resample_per_frame != 0 ? "frame " + std::to_string(f) + ": " : std::string());
    if (resample[f].filter >= kResampleFilters) {
      return set_error(SJPEG_HIP_EINVAL, frame + "resample: filter " + std::to_string(resample[f].filter) +
                                             " is not one of SJPEG_HIP_RESAMPLE_BOX (0) .. SJPEG_HIP_RESAMPLE_LANCZOS (4)");
    }
    if (resample[f].reserved[0] != 0 || resample[f].reserved[1] != 0 || resample[f].reserved[2] != 0) {
      return set_error(SJPEG_HIP_EINVAL, frame + "resample: reserved must be 0");
    }
  }
  return 0;
}

int resample_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                  const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_flatten* flatten,
                  ResamplePlan* plan) {
  *plan = ResamplePlan();
  const SourceLayout* const L = source_layout(format);
  if (L == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": unknown source format");
  if (!resamplable(*L)) {
    return set_error(SJPEG_HIP_EINVAL, who + ": " + source_format_name(format) + " pictures are not resampled (resampling takes an RGB-like or a "
                                           "gray format; decoded video, bytes or 16-bit samples, is resized by the _yuv_ entries)");
  }
  if (nframes < 1 || nframes > 65535) return set_error(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
  if (int rc = resample_check(who, nframes, resample, resample_per_frame)) return rc;
  if (flatten != nullptr) { if (int rc = flatten_check(who, format, *flatten)) return rc; }
  for (int f = 0; f < nframes; ++f) {
    const sjpeg_hip_ragged_frame& fr = frames[f];
    const std::string frame = who + ": frame " + std::to_string(f) + ": ";
    if (fr.width < 1 || fr.height < 1 || fr.width > 65535 || fr.height > 65535) {
      return set_error(SJPEG_HIP_EINVAL, frame + "bad dimensions " + std::to_string(fr.width) + "x" + std::to_string(fr.height));
    }
    if (orientations != nullptr && (orientations[f] < 1 || orientations[f] > 8)) {
      return set_error(SJPEG_HIP_EINVAL, frame + "orientation " + std::to_string(orientations[f]) + " is not one of 1..8 (EXIF tag 0x0112)");
    }
    if (flatten != nullptr) {
      const long long row = 4ll * fr.width * L->esz, have = fr.row_stride[0] < 0 ? -fr.row_stride[0] : fr.row_stride[0];
      if (have < row) {
        return set_error(SJPEG_HIP_EINVAL, frame + "|row_stride| " + std::to_string(have) + " is below the " + std::to_string(row) +
                                               " bytes of a row with its alpha (width * 4 * element size): a flattened source's alpha is read");
      }
    }
    if (sizes == nullptr) continue;
    const std::string size = "size " + std::to_string(sizes[f][0]) + "x" + std::to_string(sizes[f][1]);
    if (sizes[f][0] < 1 || sizes[f][1] < 1) return set_error(SJPEG_HIP_EINVAL, frame + size + " is below 1x1");
    if (sizes[f][0] > 65535 || sizes[f][1] > 65535) return set_error(SJPEG_HIP_EINVAL, frame + size + " is above 65535x65535");
  }
  const int channels = L->rgb_like ? 3 : 1;
  plan->format = format;
  plan->resized_format = channels == 3 ? SJPEG_HIP_SRC_RGB : SJPEG_HIP_SRC_GRAY;
  plan->flat = flatten != nullptr;
  if (flatten != nullptr) plan->flatten = *flatten;
  plan->frames.assign(static_cast<size_t>(nframes), ResampleFrame());
  // the call's tables by (filter, in, out); filter -1: the identity of a pass that is not run
  std::map<std::tuple<int, int, int>, TableAt> tables;
  std::vector<int32_t> bounds, K;
  auto table_of = [&](int f, char axis, int filter, int in, int out, TableAt* at) -> int {
    const std::tuple<int, int, int> key(in == out ? -1 : filter, in, out);
    const auto it = tables.find(key);
    if (it != tables.end()) { *at = it->second; return 0; }
    const std::string what = who + ": frame " + std::to_string(f) + ": the " + axis + " axis, " + std::to_string(in) + " to " + std::to_string(out) +
                             " samples with " + kFilterNames[filter] + ", ";
    long long ksize = 1;
    if (in == out) {
      resample_identity_table(in, &bounds, &K);
    } else {
      ksize = resample_ksize(filter, in, out);
      if (ksize > kResampleKsizeMax) {
        return set_error(SJPEG_HIP_EINVAL, what + "takes a window of " + std::to_string(ksize) + " samples, above the cap of " +
                                               std::to_string(kResampleKsizeMax));
      }
      resample_table(filter, in, out, &bounds, &K);
    }
    // what the kernel relies on: the two bounds of resample_math.h, and windows that lie inside the axis in order
    if (!resample_table_fits(K.data(), K.size())) return set_error(SJPEG_HIP_EINVAL, what + "has a coefficient of 2^23 or more");
    if (!resample_sums_fit(K.data(), static_cast<size_t>(out), static_cast<size_t>(ksize))) {
      return set_error(SJPEG_HIP_EINVAL, what + "has a sample whose sum may leave 32 bits");
    }
    for (int xx = 0; xx < out; ++xx) {
      const int32_t xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
      const bool ordered = xx == 0 || (xmin >= bounds[2 * xx - 2] && xmin + n >= bounds[2 * xx - 2] + bounds[2 * xx - 1]);
      if (xmin < 0 || n < 1 || n > ksize || xmin + n > in || !ordered) return set_error(SJPEG_HIP_EINVAL, what + "has a window outside the axis");
    }
    at->bounds = plan->tables.size();
    plan->tables.insert(plan->tables.end(), bounds.begin(), bounds.end());
    at->K = plan->tables.size();
    plan->tables.insert(plan->tables.end(), K.begin(), K.end());
    at->ksize = static_cast<int>(ksize);
    tables.emplace(key, *at);
    ++plan->ntables;
    return 0;
  };
  size_t at = 0;
  unsigned long long tiles = 0;
  for (int f = 0; f < nframes; ++f) {
    const sjpeg_hip_ragged_frame& fr = frames[f];
    ResampleFrame& d = plan->frames[f];
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
    const int filter = resample[resample_per_frame != 0 ? f : 0].filter;
    TableAt tx, ty;
    if (int rc = table_of(f, 'x', filter, d.W, d.w2, &tx)) { *plan = ResamplePlan(); return rc; }
    if (int rc = table_of(f, 'y', filter, d.H, d.h2, &ty)) { *plan = ResamplePlan(); return rc; }
    d.xb = reinterpret_cast<const int32_t*>(tx.bounds * sizeof(int32_t)); d.xk = reinterpret_cast<const int32_t*>(tx.K * sizeof(int32_t));
    d.yb = reinterpret_cast<const int32_t*>(ty.bounds * sizeof(int32_t)); d.yk = reinterpret_cast<const int32_t*>(ty.K * sizeof(int32_t));
    d.ksx = tx.ksize; d.ksy = ty.ksize;
    // the widest tile whose segment of a source row fits the stage
    const int32_t* const xb = plan->tables.data() + tx.bounds;
    int tw = static_cast<int>(kResampleTileCols);
    for (;; tw /= 2) {
      unsigned longest = 0;
      for (int x0 = 0; x0 < d.w2; x0 += tw) {
        const int x1 = (x0 + tw < d.w2 ? x0 + tw : d.w2) - 1;
        const unsigned seg = static_cast<unsigned>(xb[2 * x1] + xb[2 * x1 + 1] - xb[2 * x0]);
        if (seg > longest) longest = seg;
      }
      if (longest <= kResampleSegmentMax) break;
      if (tw == 4) {
        *plan = ResamplePlan();
        return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": the x axis has a tile whose windows span " +
                                               std::to_string(longest) + " source pixels, above " + std::to_string(kResampleSegmentMax));
      }
    }
    d.tw = tw;
    d.tiles_x = static_cast<unsigned>((d.w2 + tw - 1) / tw);
    d.orient = orientations != nullptr ? orientations[f] : 1u;
    uint32_t uw, uh;
    oriented_size(static_cast<uint32_t>(d.w2), static_cast<uint32_t>(d.h2), static_cast<int>(d.orient), &uw, &uh);
    d.dst_stride = static_cast<unsigned>(reduced_row_stride(static_cast<int>(uw), channels));
    d.dst = reinterpret_cast<uint8_t*>(at);                         // (from the buffer's start: engine_resample adds it)
    d.tile_base = static_cast<unsigned>(tiles);
    at += reduced_picture_bytes(static_cast<int>(uw), static_cast<int>(uh), channels);
    tiles += static_cast<unsigned long long>(d.tiles_x) * ((static_cast<unsigned>(d.h2) + kResampleTileRows - 1) / kResampleTileRows);
    if (tiles > 0x7fffffffull) {
      *plan = ResamplePlan();
      return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": the batch has too many tiles for one launch");
    }
  }
  plan->bytes = at;
  plan->tiles = static_cast<unsigned>(tiles);
  return 0;
}

void resample_plan_frames(const ResamplePlan& plan, const sjpeg_hip_ragged_frame* frames, uint8_t* base, sjpeg_hip_ragged_frame* out) {
  for (size_t f = 0; f < plan.frames.size(); ++f) {
    const ResampleFrame& d = plan.frames[f];
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

int sjpeg_hip_resample_ksize(int filter, int in, int out) {
  static const std::string who = "sjpeg_hip_resample_ksize";
  using namespace sjpeg_internal;
  if (filter < 0 || filter >= kResampleFilters) {
    set_error(SJPEG_HIP_EINVAL, who + ": filter " + std::to_string(filter) + " is not one of SJPEG_HIP_RESAMPLE_BOX (0) .. SJPEG_HIP_RESAMPLE_LANCZOS (4)");
    return 0;
  }
  if (in < 1 || out < 1 || in > 65535 || out > 65535) {
    set_error(SJPEG_HIP_EINVAL, who + ": in " + std::to_string(in) + " or out " + std::to_string(out) + " is not one of 1..65535");
    return 0;
  }
  const long long k = resample_ksize(filter, in, out);
  return k > 0x7fffffff ? 0x7fffffff : static_cast<int>(k);
}

int sjpeg_hip_resample_table(int filter, int in, int out, int32_t (*bounds)[2], int32_t* K, size_t K_capacity) {
  static const std::string who = "sjpeg_hip_resample_table";
  using namespace sjpeg_internal;
  if (bounds == nullptr || K == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": bounds or K == NULL");
  const int ksize = sjpeg_hip_resample_ksize(filter, in, out);
  if (ksize == 0) return SJPEG_HIP_EINVAL;                       // (the message is sjpeg_hip_resample_ksize's)
  const size_t need = static_cast<size_t>(ksize) * static_cast<size_t>(out);
  if (K_capacity < need) {
    return set_error(SJPEG_HIP_EINVAL, who + ": K_capacity " + std::to_string(K_capacity) + " is below the " + std::to_string(need) +
                                           " coefficients of the table (out * sjpeg_hip_resample_ksize)");
  }
  try {
    std::vector<int32_t> b, k;
    resample_table(filter, in, out, &b, &k);
    memcpy(bounds, b.data(), b.size() * sizeof(int32_t));
    memcpy(K, k.data(), k.size() * sizeof(int32_t));
    if (!resample_table_fits(k.data(), k.size()) || !resample_sums_fit(k.data(), static_cast<size_t>(out), static_cast<size_t>(ksize))) {
      return set_error(SJPEG_HIP_EINVAL, who + ": the table breaks a bound the kernel relies on (resample_math.h)");
    }
    return 0;
  } catch (...) {
    return set_error(SJPEG_HIP_ENOMEM, who + ": out of host memory");
  }
}

size_t sjpeg_hip_resample_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                                       const uint8_t* orientations) {
  if (frames == nullptr) return 0;
  try {
    // (the layout does not depend on the filter; the sizes are checked as the call checks them)
    const sjpeg_hip_resample box = {SJPEG_HIP_RESAMPLE_BOX, {0, 0, 0}};
    sjpeg_internal::ResamplePlan plan;
    if (sjpeg_internal::resample_plan("sjpeg_hip_resample_ragged_bytes", format, nframes, frames, sizes, orientations, &box, 0, nullptr, &plan) != 0) {
      return 0;
    }
    return plan.bytes;
  } catch (...) {
    return 0;
  }
}

}  // extern "C"
