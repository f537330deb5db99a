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

// the plan of either family: box NULL -- the _resampled_ entries -- is the whole picture and no gap for every frame, and
// nothing of the box entries' rules is applied
static int plan_frames(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                       const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_resample_box* box,
                       int box_per_frame, const sjpeg_hip_flatten* flatten, ResamplePlan* plan) {
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
  // the call's tables by (filter, in, out, the box's two ends as float32); filter -1: the identity of a pass that is not run
  std::map<std::tuple<int, int, int, float, float>, TableAt> tables;
  std::vector<int32_t> bounds, K;
  auto table_of = [&](int f, char axis, int filter, int in, int out, float b0, float b1, TableAt* at) -> int {
    const bool runs = resample_box_pass_runs(in, out, b0, b1);
    const std::tuple<int, int, int, float, float> key(runs ? filter : -1, in, out, b0, b1);
    const auto it = tables.find(key);
    if (it != tables.end()) { *at = it->second; return 0; }
    const std::string what = who + ": frame " + std::to_string(f) + ": the " + axis + " axis, " + std::to_string(in) + " to " + std::to_string(out) +
                             " samples with " + kFilterNames[filter] + ", ";
    long long ksize = 1;
    if (!runs) {
      resample_identity_table(in, &bounds, &K);
    } else {
      ksize = resample_box_ksize(filter, b0, b1, out);
      if (ksize > kResampleKsizeMax) {
        return set_error(SJPEG_HIP_EINVAL, what + "takes a window of " + std::to_string(ksize) + " samples, above the cap of " +
                                               std::to_string(kResampleKsizeMax));
      }
      resample_box_table(filter, in, out, b0, b1, &bounds, &K);
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
    float bf[4] = {0.0f, 0.0f, static_cast<float>(d.W), static_cast<float>(d.H)};
    if (box != nullptr) {
      // the box entries: the box checked, the reduce decided, the tall picture refused (resample_math.h)
      const sjpeg_hip_resample_box& bx = box[box_per_frame != 0 ? f : 0];
      const std::string frame = who + ": frame " + std::to_string(f) + ": ";
      double whole[4] = {0, 0, static_cast<double>(d.W), static_cast<double>(d.H)};
      const bool zero = bx.box[0] == 0 && bx.box[1] == 0 && bx.box[2] == 0 && bx.box[3] == 0;
      ResampleBoxDecision dec;
      const int bad = resample_box_decide(filter, d.W, d.H, d.w2, d.h2, zero ? whole : bx.box, bx.reducing_gap, &dec);
      if (bad != kBoxOk) *plan = ResamplePlan();
      const std::string size = std::to_string(fr.width) + "x" + std::to_string(fr.height);
      if (bad == kBoxBad) {
        return set_error(SJPEG_HIP_EINVAL, frame + "box (" + std::to_string(bx.box[0]) + ", " + std::to_string(bx.box[1]) + ", " +
                                               std::to_string(bx.box[2]) + ", " + std::to_string(bx.box[3]) + ") is empty or leaves the " + size +
                                               " picture (0 <= left < right <= width and 0 <= top < bottom <= height)");
      }
      if (bad == kBoxGapBad) return set_error(SJPEG_HIP_EINVAL, frame + "reducing_gap " + std::to_string(bx.reducing_gap) + " is not 0 (none) or 1.0 .. 65536.0");
      if (bad == kBoxFactorAbove) {
        return set_error(SJPEG_HIP_EINVAL, frame + "reduce factors " + std::to_string(dec.fx) + "x" + std::to_string(dec.fy) + " are above the cap of " +
                                               std::to_string(kResampleFactorMax));
      }
      if (bad == kBoxTall) {
        return set_error(SJPEG_HIP_EINVAL, frame + "a picture of " + std::to_string(dec.W) + "x" + std::to_string(dec.H) +
                                               " samples, more than 100 times as tall as wide, brought to fewer rows is not made: Pillow resamples "
                                               "it along y first");
      }
      ResampleStage st = {dec.fx, dec.fy, dec.safe[0], dec.safe[1], dec.safe[2] - dec.safe[0], dec.safe[3] - dec.safe[1],
                          {dec.m[0], dec.m[1], dec.m[2], dec.m[3]}};
      const uint32_t blocks[4] = {static_cast<uint32_t>(st.fx * st.fy), static_cast<uint32_t>((st.w - (dec.W - 1) * st.fx) * st.fy),
                                  static_cast<uint32_t>(st.fx * (st.h - (dec.H - 1) * st.fy)),
                                  static_cast<uint32_t>((st.w - (dec.W - 1) * st.fx) * (st.h - (dec.H - 1) * st.fy))};
      for (uint32_t n : blocks) {
        if (n < 1 || !resample_reduce_fits(n)) { *plan = ResamplePlan(); return set_error(SJPEG_HIP_EINVAL, frame + "a reduced block's sum may leave 32 bits"); }
      }
      if (plan->stages.empty() && (st.fx > 1 || st.fy > 1)) {
        // the first frame that is reduced: the frames before it are staged as they are
        for (int g = 0; g < f; ++g) plan->stages.push_back(ResampleStage{1, 1, 0, 0, plan->frames[g].W, plan->frames[g].H, {1u << 24, 1u << 24, 1u << 24, 1u << 24}});
      }
      if (!plan->stages.empty() || st.fx > 1 || st.fy > 1) plan->stages.push_back(st);
      d.W = dec.W; d.H = dec.H;
      for (int i = 0; i < 4; ++i) bf[i] = static_cast<float>(dec.box[i]);
    }
    TableAt tx, ty;
    if (int rc = table_of(f, 'x', filter, d.W, d.w2, bf[0], bf[2], &tx)) { *plan = ResamplePlan(); return rc; }
    if (int rc = table_of(f, 'y', filter, d.H, d.h2, bf[1], bf[3], &ty)) { *plan = ResamplePlan(); return rc; }
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

int resample_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                  const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_flatten* flatten,
                  ResamplePlan* plan) {
  return plan_frames(who, format, nframes, frames, sizes, orientations, resample, resample_per_frame, nullptr, 0, flatten, plan);
}

int resample_box_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                      const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_resample_box* box,
                      int box_per_frame, const sjpeg_hip_flatten* flatten, ResamplePlan* plan) {
  if (box == nullptr) { *plan = ResamplePlan(); return set_error(SJPEG_HIP_EINVAL, who + ": box == NULL"); }
  return plan_frames(who, format, nframes, frames, sizes, orientations, resample, resample_per_frame, box, box_per_frame, flatten, plan);
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

int sjpeg_hip_resample_box_ksize(int filter, int in, int out, float b0, float b1) {
  static const std::string who = "sjpeg_hip_resample_box_ksize";
  using namespace sjpeg_internal;
  if (filter < 0 || filter >= kResampleFilters) {
    set_error(SJPEG_HIP_EINVAL, who + ": filter " + std::to_string(filter) + " is not one of SJPEG_HIP_RESAMPLE_BOX (0) .. SJPEG_HIP_RESAMPLE_LANCZOS (4)");
    return 0;
  }
  if (in < 1 || out < 1 || in > 65535 || out > 65535) {
    set_error(SJPEG_HIP_EINVAL, who + ": in " + std::to_string(in) + " or out " + std::to_string(out) + " is not one of 1..65535");
    return 0;
  }
  if (!(0.0f <= b0 && b0 < b1 && b1 <= static_cast<float>(in))) {
    set_error(SJPEG_HIP_EINVAL, who + ": the box " + std::to_string(b0) + " .. " + std::to_string(b1) + " is empty or leaves the axis");
    return 0;
  }
  const long long k = resample_box_ksize(filter, b0, b1, out);
  return k > 0x7fffffff ? 0x7fffffff : static_cast<int>(k);
}

int sjpeg_hip_resample_box_table(int filter, int in, int out, float b0, float b1, int32_t (*bounds)[2], int32_t* K, size_t K_capacity) {
  static const std::string who = "sjpeg_hip_resample_box_table";
  using namespace sjpeg_internal;
  if (bounds == nullptr || K == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": bounds or K == NULL");
  const int ksize = sjpeg_hip_resample_box_ksize(filter, in, out, b0, b1);
  if (ksize == 0) return SJPEG_HIP_EINVAL;                       // (the message is sjpeg_hip_resample_box_ksize's)
  const size_t need = static_cast<size_t>(ksize) * static_cast<size_t>(out);
  if (K_capacity < need) {
    return set_error(SJPEG_HIP_EINVAL, who + ": K_capacity " + std::to_string(K_capacity) + " is below the " + std::to_string(need) +
                                           " coefficients of the table (out * sjpeg_hip_resample_box_ksize)");
  }
  try {
    std::vector<int32_t> b, k;
    resample_box_table(filter, in, out, b0, b1, &b, &k);
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

int sjpeg_hip_thumbnail_size(int width, int height, double box_width, double box_height, int32_t size[2]) {
  static const std::string who = "sjpeg_hip_thumbnail_size";
  using namespace sjpeg_internal;
  if (size == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": size == NULL");
  if (width < 1 || height < 1 || width > 65535 || height > 65535) {
    return set_error(SJPEG_HIP_EINVAL, who + ": bad dimensions " + std::to_string(width) + "x" + std::to_string(height));
  }
  if (!(box_width >= 1.0 && box_height >= 1.0 && box_width < 2147483648.0 && box_height < 2147483648.0)) {
    return set_error(SJPEG_HIP_EINVAL, who + ": box " + std::to_string(box_width) + "x" + std::to_string(box_height) + " is below 1x1 or no size");
  }
  int w2, h2;
  resample_thumbnail_size(width, height, box_width, box_height, &w2, &h2);
  size[0] = w2; size[1] = h2;
  return 0;
}

int sjpeg_hip_fit_crop(int width, int height, int out_width, int out_height, double bleed, double centering_x, double centering_y, double box[4]) {
  static const std::string who = "sjpeg_hip_fit_crop";
  using namespace sjpeg_internal;
  if (box == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": box == NULL");
  if (width < 1 || height < 1 || width > 65535 || height > 65535) {
    return set_error(SJPEG_HIP_EINVAL, who + ": bad dimensions " + std::to_string(width) + "x" + std::to_string(height));
  }
  if (out_width < 1 || out_height < 1 || out_width > 65535 || out_height > 65535) {
    return set_error(SJPEG_HIP_EINVAL, who + ": size " + std::to_string(out_width) + "x" + std::to_string(out_height) + " is not 1..65535 a side");
  }
  resample_fit_crop(width, height, out_width, out_height, bleed, centering_x, centering_y, box);
  return 0;
}

int sjpeg_hip_resample_box_decide(int filter, int width, int height, int out_width, int out_height, const sjpeg_hip_resample_box* box,
                                  sjpeg_hip_resample_box_decision* decision) {
  static const std::string who = "sjpeg_hip_resample_box_decide";
  using namespace sjpeg_internal;
  if (box == nullptr || decision == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": box or decision == NULL");
  if (filter < 0 || filter >= kResampleFilters) {
    return set_error(SJPEG_HIP_EINVAL, who + ": filter " + std::to_string(filter) + " is not one of SJPEG_HIP_RESAMPLE_BOX (0) .. SJPEG_HIP_RESAMPLE_LANCZOS (4)");
  }
  if (width < 1 || height < 1 || width > 65535 || height > 65535 || out_width < 1 || out_height < 1 || out_width > 65535 || out_height > 65535) {
    return set_error(SJPEG_HIP_EINVAL, who + ": a side of the picture or of the size is not 1..65535");
  }
  const double whole[4] = {0, 0, static_cast<double>(width), static_cast<double>(height)};
  const bool zero = box->box[0] == 0 && box->box[1] == 0 && box->box[2] == 0 && box->box[3] == 0;
  ResampleBoxDecision d;
  const int bad = resample_box_decide(filter, width, height, out_width, out_height, zero ? whole : box->box, box->reducing_gap, &d);
  if (bad == kBoxBad) return set_error(SJPEG_HIP_EINVAL, who + ": the box is empty or leaves the picture");
  if (bad == kBoxGapBad) return set_error(SJPEG_HIP_EINVAL, who + ": reducing_gap " + std::to_string(box->reducing_gap) + " is not 0 (none) or 1.0 .. 65536.0");
  if (bad == kBoxFactorAbove) {
    return set_error(SJPEG_HIP_EINVAL, who + ": reduce factors " + std::to_string(d.fx) + "x" + std::to_string(d.fy) + " are above the cap of " +
                                           std::to_string(kResampleFactorMax));
  }
  decision->factor[0] = d.fx; decision->factor[1] = d.fy;
  decision->reduced_size[0] = d.W; decision->reduced_size[1] = d.H;
  for (int i = 0; i < 4; ++i) { decision->safe_box[i] = d.safe[i]; decision->multiplier[i] = d.m[i]; decision->inner_box[i] = d.box[i]; }
  if (bad == kBoxTall) {
    return set_error(SJPEG_HIP_EINVAL, who + ": a picture of " + std::to_string(d.W) + "x" + std::to_string(d.H) +
                                           " samples, more than 100 times as tall as wide, brought to fewer rows is not made");
  }
  return 0;
}

size_t sjpeg_hip_resample_box_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                                           const uint8_t* orientations, const sjpeg_hip_resample_box* box, int box_per_frame) {
  if (frames == nullptr || box == nullptr) return 0;
  try {
    // (the layout does not depend on the filter, and the box filter's windows are the shortest: what it is refused, every filter is)
    const sjpeg_hip_resample filter = {SJPEG_HIP_RESAMPLE_BOX, {0, 0, 0}};
    sjpeg_internal::ResamplePlan plan;
    if (sjpeg_internal::resample_box_plan("sjpeg_hip_resample_box_ragged_bytes", format, nframes, frames, sizes, orientations, &filter, 0, box,
                                          box_per_frame, nullptr, &plan) != 0) {
      return 0;
    }
    return plan.bytes;
  } catch (...) {
    return 0;
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
