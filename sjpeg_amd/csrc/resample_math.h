// resample_math.h -- the arithmetic of resampling with Pillow's filters (sjpeg_hip_resample_ragged_src; resample.hip,
// resample_plan.cc), stated once for the kernel, the host and the tests: the five filters and the table of one axis
// in IEEE double (host only: they need the host's sin and cos), the accumulate-and-clip in integers (host and device),
// and the two bounds the kernel relies on.  It is Image.resize of Pillow 12.2.0 for pictures of bytes
// (sjpeg_hip.h, "THE DEFINITION").  Plain C++ (a host compiler reads it as it is: tests/cxx/resample_math_test.cc).
#ifndef SJPEG_AMD_RESAMPLE_MATH_H_
#define SJPEG_AMD_RESAMPLE_MATH_H_

#include <math.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define SJPEG_RESAMPLE_HD __host__ __device__
#else
#define SJPEG_RESAMPLE_HD
#endif

namespace sjpeg_internal {

constexpr int kResampleBits = 22;                       // a coefficient is a multiple of 2^-22
constexpr int kResampleFilters = 5;                     // SJPEG_HIP_RESAMPLE_BOX .. _LANCZOS
enum { kResampleBox = 0, kResampleBilinear = 1, kResampleHamming = 2, kResampleBicubic = 3, kResampleLanczos = 4 };

// ---- integers, host and device
// one tap: acc + K * b, |K| < 2^23 and b a byte -- both factors fit 24 bits (resample_table_fits), so the device
// multiplies with v_mad_i32_i24
SJPEG_RESAMPLE_HD inline int32_t resample_mac(int32_t acc, int32_t K, int32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return acc + __mul24(K, b);
#else
  return acc + K * b;
#endif
}
constexpr int32_t kResampleHalf = 1 << (kResampleBits - 1);   // what a sample's sum starts from
// a finished sum as its byte: an arithmetic shift, then the clip
SJPEG_RESAMPLE_HD inline int32_t resample_clip(int32_t sum) {
  const int32_t v = sum >> kResampleBits;
  return v < 0 ? 0 : v > 255 ? 255 : v;
}
// a sample of n taps
SJPEG_RESAMPLE_HD inline int32_t resample_sample(const int32_t* K, const uint8_t* b, int n, long long step = 1) {
  int32_t acc = kResampleHalf;
  for (int x = 0; x < n; ++x) acc = resample_mac(acc, K[x], b[x * step]);
  return resample_clip(acc);
}

// ---- doubles, host only
#if !defined(__HIP_DEVICE_COMPILE__)
inline double resample_support(int filter) {
  switch (filter) {
    case kResampleBox: return 0.5;
    case kResampleBilinear: case kResampleHamming: return 1.0;
    case kResampleBicubic: return 2.0;
    default: return 3.0;
  }
}
inline double resample_sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
inline double resample_filter(int filter, double x) {
  switch (filter) {
    case kResampleBox: return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
    case kResampleBilinear:
      if (x < 0.0) x = -x;
      return x < 1.0 ? 1.0 - x : 0.0;
    case kResampleHamming:
      if (x < 0.0) x = -x;
      if (x == 0.0) return 1.0;
      if (x >= 1.0) return 0.0;
      x = x * M_PI;
      return sin(x) / x * (0.54f + 0.46f * cos(x));       // (the two constants are floats promoted to double)
    case kResampleBicubic: {
      const double a = -0.5;
      if (x < 0.0) x = -x;
      if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
      if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
      return 0.0;
    }
    default:
      return -3.0 <= x && x < 3.0 ? resample_sinc(x) * resample_sinc(x / 3) : 0.0;
  }
}
// The taps a row of the table has room for, and the table, of an axis of `in` samples brought to `out` from the part
// [b0, b1) of it -- Image.resize(size, filter, box=): the box arrives as float32 and its length is taken in float32, as
// Pillow's C layer receives and subtracts it; everything else is double.  Windows are clamped to the AXIS, not to the
// box: samples outside the box are read, as Pillow reads them.  bounds[xx] = {xmin, n}, K[xx * ksize + x] for x < n, the
// rest of a row 0.  (ksize must fit the caller's memory: it is checked against the cap before the table is built.)
inline double resample_box_scale(float b0, float b1, int out) { return static_cast<double>(static_cast<float>(b1 - b0)) / out; }
inline long long resample_box_ksize(int filter, float b0, float b1, int out) {
  const double scale = resample_box_scale(b0, b1, out), fs = scale < 1.0 ? 1.0 : scale;
  return 2 * static_cast<long long>(ceil(resample_support(filter) * fs)) + 1;
}
inline void resample_box_table(int filter, int in, int out, float b0, float b1, std::vector<int32_t>* bounds, std::vector<int32_t>* K) {
  const double scale = resample_box_scale(b0, b1, out), fs = scale < 1.0 ? 1.0 : scale;
  const double support = resample_support(filter) * fs;
  const size_t ksize = static_cast<size_t>(resample_box_ksize(filter, b0, b1, out));
  bounds->assign(2 * static_cast<size_t>(out), 0);
  K->assign(ksize * static_cast<size_t>(out), 0);
  std::vector<double> w(ksize);
  for (int xx = 0; xx < out; ++xx) {
    const double center = static_cast<double>(b0) + (xx + 0.5) * scale;
    int xmin = static_cast<int>(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = static_cast<int>(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      w[x] = resample_filter(filter, (x + xmin - center + 0.5) / fs);
      ww += w[x];
    }
    (*bounds)[2 * xx] = xmin;
    (*bounds)[2 * xx + 1] = n;
    int32_t* const k = K->data() + ksize * xx;
    for (int x = 0; x < n; ++x) {
      const double v = ww != 0.0 ? w[x] / ww : w[x];
      k[x] = v < 0 ? static_cast<int32_t>(-0.5 + v * (1 << kResampleBits)) : static_cast<int32_t>(0.5 + v * (1 << kResampleBits));
    }
  }
}
// ... and of the whole axis, Image.resize(size, filter): the box is [0, in) (in below 2^24: a float holds it)
inline long long resample_ksize(int filter, int in, int out) { return resample_box_ksize(filter, 0.0f, static_cast<float>(in), out); }
inline void resample_table(int filter, int in, int out, std::vector<int32_t>* bounds, std::vector<int32_t>* K) {
  resample_box_table(filter, in, out, 0.0f, static_cast<float>(in), bounds, K);
}
// the table of a pass that is not run: one tap of 2^22 on the sample itself -- (2^21 + 2^22 b) >> 22 is b
inline void resample_identity_table(int n, std::vector<int32_t>* bounds, std::vector<int32_t>* K) {
  bounds->resize(2 * static_cast<size_t>(n));
  K->assign(static_cast<size_t>(n), 1 << kResampleBits);
  for (int x = 0; x < n; ++x) { (*bounds)[2 * x] = x; (*bounds)[2 * x + 1] = 1; }
}
#endif

// ---- the reduce in front of a resample (Image.resize(..., reducing_gap=), Image.thumbnail): Image.reduce of Pillow
// 12.2.0, an integer box average with Pillow's own rounding.  A reduced sample covers a block of n source samples --
// fx * fy, fewer on the right and bottom edge -- whose sum is S: it is ((S + n / 2) * m(n)) >> 24 in uint32, m(n) a
// FLOAT32 division truncated.  This is not the exact half-up average of reduce_round.h: the two disagree on 2.7 % of
// all (n, S) with n up to 64.
constexpr int kResampleFactorMax = 255;                 // a reduce factor above it is refused
SJPEG_RESAMPLE_HD inline uint32_t resample_reduce_sample(uint32_t S, uint32_t n, uint32_t m) { return ((S + (n >> 1)) * m) >> 24; }
#if !defined(__HIP_DEVICE_COMPILE__)
inline uint32_t resample_reduce_multiplier(uint32_t n) { return static_cast<uint32_t>(4294967296.0f / static_cast<float>(256u * n)); }
// (255 n + n / 2) * m(n) stays inside a uint32 for every block of up to kResampleFactorMax^2 samples (the plan checks it)
inline bool resample_reduce_fits(uint32_t n) {
  return (255ull * n + (n >> 1)) * resample_reduce_multiplier(n) < (1ull << 32);
}

// What a frame's box and reducing_gap come to (sjpeg_hip.h, "THE DEFINITION of the box entries"): the picture is W x H,
// the target w2 x h2, box = (l, t, r, b) in doubles, gap 0 (none) or >= 1.  All of it IEEE double as Python does it.
struct ResampleBoxDecision {
  int fx, fy;                    // the reduce factors; both 1: no reduce
  int safe[4];                   // the part of the picture that is reduced (fx = fy = 1: the whole picture)
  int W, H;                      // the size of the picture the tables are of: the reduced one
  uint32_t m[4];                 // the multipliers of an interior, right-edge, bottom-edge and corner block
  double box[4];                 // the box in that picture's samples
};
enum { kBoxOk = 0, kBoxBad = 1, kBoxGapBad = 2, kBoxFactorAbove = 3, kBoxTall = 4 };
inline int resample_box_decide(int filter, int W, int H, int w2, int h2, const double* box, double gap, ResampleBoxDecision* d) {
  const double l = box[0], t = box[1], r = box[2], b = box[3];
  // (written so that a NaN fails)
  if (!(0 <= l && 0 <= t && r <= W && b <= H && r - l > 0 && b - t > 0)) return kBoxBad;
  if (gap != 0 && !(gap >= 1.0 && gap <= 65536.0)) return kBoxGapBad;
  d->fx = d->fy = 1;
  d->safe[0] = d->safe[1] = 0; d->safe[2] = W; d->safe[3] = H;
  d->W = W; d->H = H;
  for (int i = 0; i < 4; ++i) d->box[i] = box[i];
  if (gap != 0) {
    const int fx = static_cast<int>((r - l) / w2 / gap), fy = static_cast<int>((b - t) / h2 / gap);
    d->fx = fx != 0 ? fx : 1; d->fy = fy != 0 ? fy : 1;
  }
  if (d->fx > kResampleFactorMax || d->fy > kResampleFactorMax) return kBoxFactorAbove;
  if (d->fx > 1 || d->fy > 1) {
    const double s = resample_support(filter) - 0.5, sx = (r - l) / w2, sy = (b - t) / h2;
    const int x0 = static_cast<int>(l - s * sx), y0 = static_cast<int>(t - s * sy);
    const double x1 = ceil(r + s * sx), y1 = ceil(b + s * sy);
    d->safe[0] = x0 > 0 ? x0 : 0; d->safe[1] = y0 > 0 ? y0 : 0;
    d->safe[2] = x1 < W ? static_cast<int>(x1) : W; d->safe[3] = y1 < H ? static_cast<int>(y1) : H;
    d->W = (d->safe[2] - d->safe[0] + d->fx - 1) / d->fx;
    d->H = (d->safe[3] - d->safe[1] + d->fy - 1) / d->fy;
    d->box[0] = (l - d->safe[0]) / d->fx; d->box[1] = (t - d->safe[1]) / d->fy;
    d->box[2] = (r - d->safe[0]) / d->fx; d->box[3] = (b - d->safe[1]) / d->fy;
  }
  const int ex = d->safe[2] - d->safe[0] - (d->W - 1) * d->fx, ey = d->safe[3] - d->safe[1] - (d->H - 1) * d->fy;   // the edge blocks' sides
  const uint32_t n[4] = {static_cast<uint32_t>(d->fx * d->fy), static_cast<uint32_t>(ex * d->fy), static_cast<uint32_t>(d->fx * ey),
                         static_cast<uint32_t>(ex * ey)};
  for (int i = 0; i < 4; ++i) d->m[i] = resample_reduce_multiplier(n[i]);
  // Pillow resamples such a picture along y first: its uint8 intermediate lies on the other axis
  if (d->H > 100 * d->W && h2 < d->H) return kBoxTall;
  return kBoxOk;
}
// whether the pass of an axis of `in` samples runs: Pillow's rule on the box rounded to float32
inline bool resample_box_pass_runs(int in, int out, float b0, float b1) { return out != in || b0 != 0.0f || b1 != static_cast<float>(in); }

// Image.thumbnail's size: the box sides floored (both at least 1: the caller checks), never larger than the picture,
// the aspect kept by Pillow's round_aspect -- of floor(v) and ceil(v) the one whose ratio is nearer, ties to the floor
inline void resample_thumbnail_size(int W, int H, double bw, double bh, int* w2, int* h2) {
  const double x = floor(bw), y = floor(bh);
  if (x >= W && y >= H) { *w2 = W; *h2 = H; return; }
  const double aspect = static_cast<double>(W) / H;
  auto round_aspect = [](double v, auto key) {
    const double lo = floor(v), hi = ceil(v);
    const double n = key(hi) < key(lo) ? hi : lo;
    return n > 1 ? n : 1.0;
  };
  double ox = x, oy = y;
  if (x / y >= aspect) {
    ox = round_aspect(y * aspect, [&](double n) { return fabs(aspect - n / y); });
  } else {
    oy = round_aspect(x / aspect, [&](double n) { return n == 0 ? 0.0 : fabs(aspect - x / n); });
  }
  *w2 = static_cast<int>(ox); *h2 = static_cast<int>(oy);
}
// ImageOps.fit's crop box: `bleed` of each side removed (outside [0, 0.5): 0), the rest cropped to the ratio w2 : h2
// around the centering (a coordinate outside [0, 1]: 0.5)
inline void resample_fit_crop(int W, int H, int w2, int h2, double bleed, double cx, double cy, double* box) {
  if (!(0.0 <= cx && cx <= 1.0)) cx = 0.5;
  if (!(0.0 <= cy && cy <= 1.0)) cy = 0.5;
  if (!(0.0 <= bleed && bleed < 0.5)) bleed = 0.0;
  const double bx = bleed * W, by = bleed * H;
  const double lw = W - bx * 2, lh = H - by * 2;
  const double live = lw / lh, want = static_cast<double>(w2) / h2;
  double cw = lw, ch = lh;
  if (live == want) {
  } else if (live >= want) {
    cw = want * lh;
  } else {
    ch = lw / want;
  }
  box[0] = bx + (lw - cw) * cx; box[1] = by + (lh - ch) * cy;
  box[2] = box[0] + cw; box[3] = box[1] + ch;
}
#endif

// ---- the two bounds, checked for every table the plan builds
// every |K| below 2^23: a coefficient is a signed 24-bit factor
inline bool resample_table_fits(const int32_t* K, size_t count) {
  for (size_t i = 0; i < count; ++i) if (K[i] >= (1 << 23) || K[i] <= -(1 << 23)) return false;
  return true;
}
// 2^21 + 255 * max(sum of the positive K, sum of the |negative K|) of every row below 2^31: no partial sum of a sample,
// in any order, leaves an int32
inline bool resample_sums_fit(const int32_t* K, size_t rows, size_t ksize) {
  for (size_t r = 0; r < rows; ++r) {
    int64_t pos = 0, neg = 0;
    for (size_t x = 0; x < ksize; ++x) {
      const int64_t k = K[r * ksize + x];
      if (k > 0) pos += k; else neg -= k;
    }
    if (kResampleHalf + 255 * (pos > neg ? pos : neg) >= (int64_t(1) << 31)) return false;
  }
  return true;
}

}  // namespace sjpeg_internal

#endif  // SJPEG_AMD_RESAMPLE_MATH_H_
