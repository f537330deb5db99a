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
// the taps a row of the table has room for (in, out >= 1)
inline long long resample_ksize(int filter, int in, int out) {
  const double scale = static_cast<double>(in) / out, fs = scale < 1.0 ? 1.0 : scale;
  return 2 * static_cast<long long>(ceil(resample_support(filter) * fs)) + 1;
}
// The table of an axis from `in` to `out` samples: bounds[xx] = {xmin, n}, K[xx * ksize + x] for x < n, the rest of a
// row 0.  (ksize must fit the caller's memory: it is checked against the cap before this is called.)
inline void resample_table(int filter, int in, int out, std::vector<int32_t>* bounds, std::vector<int32_t>* K) {
  const double scale = static_cast<double>(in) / out, fs = scale < 1.0 ? 1.0 : scale;
  const double support = resample_support(filter) * fs;
  const size_t ksize = static_cast<size_t>(resample_ksize(filter, in, out));
  bounds->assign(2 * static_cast<size_t>(out), 0);
  K->assign(ksize * static_cast<size_t>(out), 0);
  std::vector<double> w(ksize);
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
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
// the table of a pass that is not run: one tap of 2^22 on the sample itself -- (2^21 + 2^22 b) >> 22 is b
inline void resample_identity_table(int n, std::vector<int32_t>* bounds, std::vector<int32_t>* K) {
  bounds->resize(2 * static_cast<size_t>(n));
  K->assign(static_cast<size_t>(n), 1 << kResampleBits);
  for (int x = 0; x < n; ++x) { (*bounds)[2 * x] = x; (*bounds)[2 * x + 1] = 1; }
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
