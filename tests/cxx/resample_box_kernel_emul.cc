// resample_box.hip's kernel ITSELF on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer, as
// resample_kernel_emul.cc runs resample.hip's: tests/test_resample_box_cxx.py cuts the kernel's source out of
// sjpeg_amd/csrc/resample_box.hip (everything in front of the launch function, the address space attributes and the HIP
// include taken out) into resample_box_kernel_body.inc, and this file gives it 256 std::threads a workgroup with a
// std::barrier as __syncthreads.  The plan, the sources and the expectation -- Pillow's reduce and the two passes from
// resample_math.h -- are resample_box_plan_test.cc's.  Packed RGB, BGRA with its fourth byte dropped, gray planes and
// flattened RGBA and BGRA run over frames
// that are reduced -- factors that divide no side, a safe box whose origin is no multiple of the factor, a factor of 50
// -- and frames of the same batch that are not, interior boxes, boxes on the edge, more than one tile on both axes and the
// eight orientations; every byte must equal the definition, and no access may leave its buffer: the sources lie in heap
// buffers of exactly their bytes, so a dword read past a run's last byte at a picture's end is caught.
#define RESAMPLE_BOX_NO_MAIN
#include "resample_box_plan_test.cc"
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
#include "resample_box_kernel_body.inc"

template <int kCls, bool kFlat>
static void launch(const ResampleBoxArgs& a, unsigned tiles) {
  for (unsigned b = 0; b < tiles; ++b) {
    std::barrier<> bar(256);
    g_bar = &bar;
    std::vector<std::thread> ts;
    for (unsigned t = 0; t < 256; ++t) ts.emplace_back([&, t] { threadIdx_ = {t, 0, 0}; blockIdx_ = {b, 0, 0}; resample_box_kernel<kCls, kFlat>(a); });
    for (auto& t : ts) t.join();
  }
}

// flat: the four-byte formats flattened over a background; else their fourth byte is dropped
static int run(int format, bool flat, const std::vector<BoxCase>& cases) {
  const int channels = format == SJPEG_HIP_SRC_GRAY ? 1 : 3;
  const int step = format == SJPEG_HIP_SRC_RGBA || format == SJPEG_HIP_SRC_BGRA ? 4 : channels;
  const bool bgr = format == SJPEG_HIP_SRC_BGRA;
  std::vector<Source> srcs; std::vector<sjpeg_hip_ragged_frame> frames; std::vector<int32_t> sizes; std::vector<uint8_t> orients;
  std::vector<sjpeg_hip_resample> rs; std::vector<sjpeg_hip_resample_box> boxes;
  for (size_t k = 0; k < cases.size(); ++k) {
    srcs.push_back(make_source(cases[k].w, cases[k].h, step, 277u + k));
    frames.push_back(srcs.back().frame);
    sizes.push_back(cases[k].w2); sizes.push_back(cases[k].h2);
    orients.push_back(cases[k].orient); rs.push_back(sjpeg_hip_resample{(uint8_t)cases[k].filter, {0, 0, 0}});
    sjpeg_hip_resample_box b; memcpy(b.box, cases[k].box, sizeof(b.box)); b.reducing_gap = cases[k].gap;
    boxes.push_back(b);
  }
  const int n = cases.size();
  const sjpeg_hip_flatten fl = {{17, 128, 250}, 0, 255.0f, 0.0f};
  ResamplePlan plan;
  CHECK(resample_box_plan("t", format, n, frames.data(), (const int32_t (*)[2])sizes.data(), orients.data(), rs.data(), 1, boxes.data(), 1,
                          flat ? &fl : nullptr, &plan) == 0);
  CHECK(plan.stages.size() == (size_t)n);
  std::unique_ptr<uint8_t[]> dst(new uint8_t[plan.bytes]);
  memset(dst.get(), 0xcd, plan.bytes);
  std::vector<ResampleBoxFrame> desc(n);
  const uint8_t* T = (const uint8_t*)plan.tables.data();
  for (int f = 0; f < n; ++f) {
    ResampleFrame d = plan.frames[f];
    d.dst = dst.get() + (uintptr_t)d.dst;
    d.xb = (const int32_t*)(T + (uintptr_t)d.xb); d.xk = (const int32_t*)(T + (uintptr_t)d.xk);
    d.yb = (const int32_t*)(T + (uintptr_t)d.yb); d.yk = (const int32_t*)(T + (uintptr_t)d.yk);
    desc[f].r = d; desc[f].s = plan.stages[f];
  }
  ResampleBoxArgs a; memset(&a, 0, sizeof(a));
  a.frames = desc.data(); a.nframes = n; a.kind = 0; a.channels = channels; a.pix_step = step;
  for (int c = 0; c < 3; ++c) a.bg[c] = fl.background[c];
  if (flat) launch<kPacked, true>(a, plan.tiles); else if (channels == 1) launch<kPlanes, false>(a, plan.tiles); else launch<kPacked, false>(a, plan.tiles);
  std::vector<sjpeg_hip_ragged_frame> made(n);
  resample_plan_frames(plan, frames.data(), dst.get(), made.data());
  long long samples = 0;
  int reduced = 0;
  for (int f = 0; f < n; ++f) {
    const BoxCase& c = cases[f];
    reduced += plan.stages[f].fx > 1 || plan.stages[f].fy > 1;
    // what the encoder sees of the source: R, G, B of every pixel, flattened where there is alpha
    std::vector<uint8_t> seen((size_t)c.w * c.h * channels);
    for (int i = 0; i < c.w * c.h; ++i) for (int ch = 0; ch < channels; ++ch) {
      const uint8_t* px = srcs[f].buf.get() + (size_t)i * step;
      const uint8_t b = px[bgr ? 2 - ch : ch];
      seen[(size_t)i * channels + ch] = flat ? (uint8_t)flatten_byte(px[3], b, fl.background[ch], false) : b;
    }
    std::vector<uint8_t> want;
    BoxCase whole = c;
    if (c.box[0] == 0 && c.box[1] == 0 && c.box[2] == 0 && c.box[3] == 0) { whole.box[2] = c.w; whole.box[3] = c.h; }
    CHECK(expect_box(seen.data(), c.w, c.h, channels, whole, &want));
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
  printf("format %d flat %d: %lld samples equal, %u tiles, %d of %d frames reduced\n", format, (int)flat, samples, plan.tiles, reduced, n);
  return 0;
}

int main() {
  // {w, h, w2, h2, filter, orient, box, gap}
  std::vector<BoxCase> cases = {
      {37, 29, 6, 7, 3, 1, {0, 0, 0, 0}, 2.0},                    // factors 3 x 2, neither side a multiple: all four multipliers
      {40, 30, 11, 9, 3, 1, {0.1, 0.2, 30.7, 20.3}, 0},           // not reduced, beside reduced ones: a box whose float32 tables differ
      {64, 48, 8, 6, 1, 1, {5.5, 3.25, 60.0, 44.75}, 1.0},        // an interior box, factors 6 x 6, the safe box's origin no multiple
      {90, 20, 6, 9, 2, 1, {11, 2, 83, 19}, 3.0},                 // one axis reduced, the other enlarged
      {45, 45, 5, 5, 0, 1, {0.3, 0.3, 44.6, 44.6}, 1.5},          // a box on the picture's edge: windows clamp
      {300, 160, 70, 37, 3, 1, {0, 0, 0, 0}, 2.0},                // more than one tile on both axes, partial last tiles
      {300, 160, 70, 37, 4, 1, {20.5, 10.5, 290.25, 150.75}, 1.0},
      {4000, 8, 40, 4, 4, 1, {0, 0, 0, 0}, 2.0},                  // a factor of 50: refused without the reduce
      {1, 1, 1, 1, 3, 1, {0, 0, 0, 0}, 2.0}, {2, 9, 1, 2, 4, 1, {0, 0, 0, 0}, 1.0}, {9, 2, 2, 1, 0, 1, {0.5, 0, 9, 2}, 1.0},
      {31, 29, 40, 35, 3, 1, {2.3, 4.1, 17.9, 19.6}, 2.0},        // enlarging from a box: a gap whose factors are 1
  };
  for (int o = 1; o <= 8; ++o) cases.push_back({57, 41, 9, 6, o % 5, o, {1.25, 0.5, 56.0, 40.5}, 2.0});
  for (int format : {SJPEG_HIP_SRC_RGB, SJPEG_HIP_SRC_BGRA, SJPEG_HIP_SRC_GRAY}) if (run(format, false, cases) != 0) return 1;
  for (int format : {SJPEG_HIP_SRC_RGBA, SJPEG_HIP_SRC_BGRA}) if (run(format, true, cases) != 0) return 1;
  printf("resample box kernel emulation ok\n");
  return 0;
}
