// pillow_filter.hip's kernel ITSELF on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer, as
// resample_box_kernel_emul.cc runs resample_box.hip's: tests/test_pillow_filter_cxx.py cuts the kernel's source out of
// sjpeg_amd/csrc/pillow_filter.hip (everything in front of the launch function, the address space attributes and the HIP
// include taken out) into pillow_filter_kernel_body.inc, and this file gives it 256 std::threads with a std::barrier as
// __syncthreads.  The plan, the pictures and the expectation -- the closed form with clamped indices --
// are pillow_filter_plan_test.cc's.  The made pictures, the scratch between the two launches and the output lie in heap
// buffers of exactly their bytes, so the tile, halo and ping-pong indexing is held to every buffer's ends: 1 x 1, both
// clamps at once, a partial last tile, seams on both axes, a halo wider than the tile along rows and along columns
// (sigma 64: r = 63 three times, 192 positions on both sides of an interior tile, which fills the staging buffers),
// kinds mixed in one batch with kind 0 and skipped axes among them.  Every byte of every picture must equal the
// expectation, and the bytes between the pictures must stay as they were.
#define PILLOW_FILTER_NO_MAIN
#include "pillow_filter_plan_test.cc"
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
#include "pillow_filter_kernel_body.inc"

// 256 threads for the whole launch: each runs its lane of workgroup after workgroup, a barrier between two workgroups
// (the staging buffers are one static array, as LDS is one per workgroup at a time)
template <int kAxis>
static void launch(const PillowFilterArgs& a, unsigned tiles) {
  std::barrier<> bar(256);
  g_bar = &bar;
  std::vector<std::thread> ts;
  for (unsigned t = 0; t < 256; ++t) ts.emplace_back([&, t] {
    for (unsigned b = 0; b < tiles; ++b) {
      threadIdx_ = {t, 0, 0}; blockIdx_ = {b, 0, 0};
      pillow_filter_kernel<kAxis>(a);
      g_bar->arrive_and_wait();
    }
  });
  for (auto& t : ts) t.join();
}

struct Case { Picture pic; sjpeg_hip_pillow_filter f; };

static int run(int format, const std::vector<Case>& cases) {
  const int c = format == SJPEG_HIP_SRC_RGB ? 3 : 1, n = (int)cases.size();
  std::vector<Picture> pics; std::vector<sjpeg_hip_pillow_filter> fs;
  for (const Case& k : cases) { pics.push_back(k.pic); fs.push_back(k.f); }
  Batch made = make_batch(format, pics, 31u + format);
  PillowFilterPlan plan;
  CHECK(pillow_filter_plan("t", format, n, made.frames.data(), made.buf.get(), fs.data(), 1, &plan) == 0);
  std::unique_ptr<uint8_t[]> mid(new uint8_t[made.bytes]), dst(new uint8_t[made.bytes]);
  memset(mid.get(), 0xcd, made.bytes); memset(dst.get(), 0xcd, made.bytes);
  std::vector<PillowFilterPlane> desc = plan.planes;
  for (PillowFilterPlane& d : desc) { d.made = made.buf.get() + (uintptr_t)d.made; d.mid = mid.get() + (uintptr_t)d.mid; d.dst = dst.get() + (uintptr_t)d.dst; }
  PillowFilterArgs a; a.planes = desc.data(); a.nplanes = n;
  launch<0>(a, plan.tiles[0]);
  launch<1>(a, plan.tiles[1]);
  long long samples = 0;
  std::vector<uint8_t> touched(made.bytes, 0);
  for (int k = 0; k < n; ++k) {
    const int w = pics[k].w, h = pics[k].h;
    const size_t stride = (size_t)made.frames[k].row_stride[0], off = (uintptr_t)plan.planes[k].made;
    std::vector<uint8_t> src((size_t)w * h * c);
    for (int y = 0; y < h; ++y) memcpy(&src[(size_t)y * w * c], made.buf.get() + off + y * stride, (size_t)w * c);
    const std::vector<uint8_t> want = expect_filter(src, w, h, c, fs[k]);
    for (int y = 0; y < h; ++y) {
      for (size_t i = 0; i < stride; ++i) touched[off + y * stride + i] = 1;     // (a row's padding up to its last dword may be written)
      for (int i = 0; i < w * c; ++i) {
        const uint8_t got = dst[off + y * stride + i];
        if (got != want[(size_t)y * w * c + i]) { printf("MISMATCH format %d frame %d (%dx%d kind %d) row %d byte %d: %d want %d\n", format, k, w, h, fs[k].kind, y, i, got, want[(size_t)y * w * c + i]); return 1; }
        ++samples;
      }
    }
  }
  for (size_t i = 0; i < made.bytes; ++i) if (!touched[i]) CHECK(dst[i] == 0xcd && mid[i] == 0xcd);
  printf("format %d: %lld samples equal, %u + %u tiles\n", format, samples, plan.tiles[0], plan.tiles[1]);
  return 0;
}

int main() {
  if (plan_tests() != 0) return 1;
  const std::vector<Case> cases = {
      {{1, 1}, filter_of(2, 2.0f, 2.0f)},                          // a degenerate line
      {{5, 7}, filter_of(1, 5.0f, 5.0f)},                          // both clamps at once
      {{5, 7}, filter_of(2, 5.0f, 3.0f)},                          // ... three passes of them
      {{70, 37}, filter_of(2, 2.0f, 2.0f)},                        // a partial last tile
      {{300, 160}, filter_of(2, 1.5f, 4.0f)},                      // more than one tile on both axes: seams
      {{300, 20}, filter_of(1, 63.0f, 0.0f)},                      // one pass of r = 63: a halo of 64; the columns skipped
      {{20, 300}, filter_of(1, 0.0f, 63.9f)},                      // the same, for columns (a halo as wide as the tile); the rows skipped
      {{640, 6}, filter_of(2, 64.0f, 0.0f)},                       // sigma 64: three passes of r = 63, a halo of 192 on both sides of
      {{6, 600}, filter_of(3, 64.0f, 64.0f, 150, 3)},              // interior tiles -- wider than the tile, the LDS filled to its last dword
      {{150, 70}, filter_of(2, 40.0f, 40.0f)},                     // three passes of r = 39: halos the line's ends cut off
      {{33, 9}, filter_of(0, 9.0f, 9.0f)},                         // kind 0 in a mixed batch: a copy
      {{131, 67}, filter_of(3, 2.0f, 2.0f, 150, 3)},               // unsharp masks: the made picture read beside the blurred one
      {{17, 9}, filter_of(3, 0.6f, 0.6f, 500, 1)},
      {{17, 9}, filter_of(3, 2.0f, 2.0f, 150, 255)}, {{2, 3}, filter_of(3, 0.0f, 0.0f, 150, 0)},
      {{129, 5}, filter_of(1, 0.3f, 2.7f)}, {{128, 65}, filter_of(2, 1.0f, 3.3f)}, {{2, 3}, filter_of(1, 0.5f, 1.0f)},
  };
  for (int format : {SJPEG_HIP_SRC_RGB, SJPEG_HIP_SRC_GRAY}) if (run(format, cases) != 0) return 1;
  printf("pillow filter kernel emulation ok\n");
  return 0;
}
