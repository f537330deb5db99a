// resample.hip's kernel ITSELF on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/test_resample_cxx.py
// cuts the kernel's source out of sjpeg_amd/csrc/resample.hip (everything in front of the launch function, the address
// space attributes and the HIP include taken out) into resample_kernel_body.inc, and this file gives it what a host
// compiler lacks: 256 std::threads a workgroup with a std::barrier as __syncthreads, threadIdx and blockIdx per thread,
// __shared__ as static storage (workgroups run one after another), __mul24.  The plan, the sources, the cases' struct and
// the expectation are resample_plan_test.cc's.  Packed RGB, gray planes and flattened RGBA run over tile edges, tiny
// pictures, enlarging, a strip, the cap, a wide frame with a narrow tile and the eight orientations; every byte must
// equal the two passes, and no access may leave its buffer -- the LDS arrays included.
#define main plan_test_main
#include "resample_plan_test.cc"
#undef main
#include <barrier>
#include <thread>
#undef __global__
#undef __device__
#undef __host__
#undef __forceinline__
#undef __shared__
#undef __launch_bounds__
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)
struct Idx { unsigned x, y, z; };
static thread_local Idx threadIdx_, blockIdx_;
#define threadIdx threadIdx_
#define blockIdx blockIdx_
static std::barrier<>* g_bar;
static inline void __syncthreads() { g_bar->arrive_and_wait(); }
static inline int __mul24(int a, int b) { return a * b; }
using std::min; using std::max;
namespace sjpeg_internal { static inline int elem_load_u8(const uint8_t* p, int, float, float) { return *p; } }
#include "../../sjpeg_amd/csrc/flatten_math.h"
#include "resample_kernel_body.inc"

template <int kCls, bool kFlat>
static void launch(const ResampleArgs& a, unsigned tiles) {
  for (unsigned b = 0; b < tiles; ++b) {
    std::barrier<> bar(256);
    g_bar = &bar;
    std::vector<std::thread> ts;
    for (unsigned t = 0; t < 256; ++t) ts.emplace_back([&, t] { threadIdx_ = {t, 0, 0}; blockIdx_ = {b, 0, 0}; resample_kernel<kCls, kFlat>(a); });
    for (auto& t : ts) t.join();
  }
}

static int run(int format, const std::vector<Case>& cases) {
  const int channels = format == SJPEG_HIP_SRC_GRAY ? 1 : 3;
  const int step = format == SJPEG_HIP_SRC_RGBA ? 4 : channels;
  std::vector<Source> srcs; std::vector<sjpeg_hip_ragged_frame> frames; std::vector<int32_t> sizes; std::vector<uint8_t> orients; std::vector<sjpeg_hip_resample> rs;
  for (size_t k = 0; k < cases.size(); ++k) {
    srcs.push_back(make_source(cases[k].w, cases[k].h, step, 177u + k));
    frames.push_back(srcs.back().frame);
    sizes.push_back(cases[k].w2); sizes.push_back(cases[k].h2);
    orients.push_back(cases[k].orient); rs.push_back(sjpeg_hip_resample{(uint8_t)cases[k].filter, {0, 0, 0}});
  }
  const int n = cases.size();
  const sjpeg_hip_flatten fl = {{17, 128, 250}, 0, 255.0f, 0.0f};
  ResamplePlan plan;
  CHECK(resample_plan("t", format, n, frames.data(), (const int32_t (*)[2])sizes.data(), orients.data(), rs.data(), 1, step == 4 ? &fl : nullptr, &plan) == 0);
  std::unique_ptr<uint8_t[]> dst(new uint8_t[plan.bytes]);
  memset(dst.get(), 0xcd, plan.bytes);
  std::vector<ResampleFrame> desc = plan.frames;
  const uint8_t* T = (const uint8_t*)plan.tables.data();
  for (auto& d : desc) {
    d.dst = dst.get() + (uintptr_t)d.dst;
    d.xb = (const int32_t*)(T + (uintptr_t)d.xb); d.xk = (const int32_t*)(T + (uintptr_t)d.xk);
    d.yb = (const int32_t*)(T + (uintptr_t)d.yb); d.yk = (const int32_t*)(T + (uintptr_t)d.yk);
  }
  ResampleArgs a; memset(&a, 0, sizeof(a));
  a.frames = desc.data(); a.nframes = n; a.kind = 0; a.channels = channels; a.pix_step = step;
  for (int c = 0; c < 3; ++c) a.bg[c] = fl.background[c];
  if (step == 4) launch<kPacked, true>(a, plan.tiles); else if (channels == 1) launch<kPlanes, false>(a, plan.tiles); else launch<kPacked, false>(a, plan.tiles);
  std::vector<sjpeg_hip_ragged_frame> made(n);
  resample_plan_frames(plan, frames.data(), dst.get(), made.data());
  long long samples = 0;
  for (int f = 0; f < n; ++f) {
    const Case& c = cases[f];
    Source flat = make_source(c.w, c.h, channels, 1);
    if (step == 4) {
      for (int i = 0; i < c.w * c.h; ++i) for (int ch = 0; ch < 3; ++ch)
        flat.buf[i * 3 + ch] = (uint8_t)flatten_byte(srcs[f].buf[i * 4 + 3], srcs[f].buf[i * 4 + ch], fl.background[ch], false);
    }
    const std::vector<uint8_t> want = expect(step == 4 ? flat : srcs[f], channels, c.w2, c.h2, c.filter);
    const uint8_t* p = (const uint8_t*)made[f].plane[0];
    for (int y = 0; y < c.h2; ++y) for (int x = 0; x < c.w2; ++x) {
      uint32_t ux, uy;
      orient_upright(x, y, c.w2, c.h2, c.orient, &ux, &uy);
      for (int ch = 0; ch < channels; ++ch) {
        const uint8_t got = p[(size_t)uy * made[f].row_stride[0] + (size_t)ux * channels + ch];
        if (got != want[((size_t)y * c.w2 + x) * channels + ch]) { printf("MISMATCH format %d frame %d (%d,%d,%d): %d want %d\n", format, f, x, y, ch, got, want[((size_t)y * c.w2 + x) * channels + ch]); return 1; }
        ++samples;
      }
    }
  }
  printf("format %d: %lld samples equal, %u tiles\n", format, samples, plan.tiles);
  return 0;
}

int main() {
  std::vector<Case> cases;
  const int widths[] = {31, 32, 33, 34, 63, 64, 65}, heights[] = {15, 16, 17, 18, 31, 32, 33};
  for (int k = 0; k < 7; ++k) cases.push_back({48, 24, widths[k], heights[k], k % 5, 1});
  const Case more[] = {{1, 1, 1, 1, 4, 1}, {1, 1, 3, 3, 3, 1}, {2, 1, 1, 2, 2, 1}, {1, 2, 2, 1, 1, 1}, {3, 3, 1, 1, 0, 1}, {3, 3, 3, 3, 4, 5},
                       {50, 40, 50, 17, 4, 1}, {50, 40, 23, 40, 3, 1}, {50, 40, 75, 13, 2, 1}, {50, 40, 20, 90, 1, 1}, {20, 12, 30, 18, 0, 1},
                       {9, 7, 63, 49, 4, 1}, {100, 60, 37, 23, 3, 1}, {700, 5, 3, 2, 0, 1}, {192, 192, 3, 3, 4, 1}, {12000, 2, 33, 40, 0, 3}};
  for (const Case& c : more) cases.push_back(c);
  for (int o = 1; o <= 8; ++o) cases.push_back({40, 23, 57, 11, o % 5, o});
  for (int format : {SJPEG_HIP_SRC_RGB, SJPEG_HIP_SRC_GRAY, SJPEG_HIP_SRC_RGBA}) if (run(format, cases) != 0) return 1;
  printf("resample kernel emulation ok\n");
  return 0;
}
