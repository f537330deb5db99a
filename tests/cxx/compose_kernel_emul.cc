// compose.hip's kernel ITSELF on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer, as
// pillow_filter_kernel_emul.cc runs pillow_filter.hip's: tests/test_compose_cxx.py cuts the kernel's source out of
// sjpeg_amd/csrc/compose.hip (everything in front of the launch function, the address space attributes and the HIP
// include taken out) into compose_kernel_body.inc, and this file runs it lane by lane, workgroup by workgroup -- the
// kernel has no barrier and no LDS, so the lanes need no threads.  The plan, the pictures, the overlays and the
// expectation are compose_plan_test.cc's.  The made pictures, the overlays and the canvases lie in heap buffers of
// exactly their bytes; beyond that EVERY load and store of the kernel goes through SJPEG_COMPOSE_ACCESS and is held
// to be an aligned dword inside a row of what it says it touches: a made picture's row, a canvas row, an overlay's row
// of 4 * width bytes.  The geometries are the GPU test's: 1 x 1 at (1, 1); every byte phase of 3 * px beside a canvas
// whose last dword holds padding; a picture touching the right and bottom edge; 300 x 20 and 20 x 300 canvases; a frame
// without compose; overlays over each edge, wholly outside, over the whole canvas, overlapping, eight on one frame, one
// used by three frames, one with a stride above 4 * width; alphas of 0, 255 and random.  Every sample of every canvas
// must equal the expectation, and the bytes between the canvases must stay as they were.
#define COMPOSE_NO_MAIN
#include "compose_plan_test.cc"

#include <algorithm>

#undef __global__
#undef __device__
#undef __host__
#undef __forceinline__
#undef __launch_bounds__
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
struct Idx { unsigned x, y, z; };
static Idx threadIdx_, blockIdx_;
#define threadIdx threadIdx_
#define blockIdx blockIdx_

// ---- the rows an access may touch
struct Row { uintptr_t lo, hi; int what; };
static std::vector<Row> g_rows;
static long long g_accesses[3] = {0, 0, 0};
static bool g_bad = false;
static void add_rows(const uint8_t* first, size_t stride, int rows, size_t row_bytes, int what) {
  for (int y = 0; y < rows; ++y) g_rows.push_back({(uintptr_t)(first + y * stride), (uintptr_t)(first + y * stride + row_bytes), what});
}
static void access(const void* p, int what) {
  const uintptr_t a = (uintptr_t)p;
  ++g_accesses[what];
  if (g_bad) return;
  if (a & 3u) { printf("an access of kind %d at %p is not aligned\n", what, p); g_bad = true; return; }
  auto it = std::upper_bound(g_rows.begin(), g_rows.end(), a, [](uintptr_t v, const Row& r) { return v < r.lo; });
  if (it == g_rows.begin()) { printf("an access of kind %d at %p is in front of every row\n", what, p); g_bad = true; return; }
  --it;
  if (a + 4 > it->hi || it->what != what) { printf("an access of kind %d at %p is outside its row (kind %d, %zu bytes)\n", what, p, it->what, (size_t)(it->hi - it->lo)); g_bad = true; }
}
#define SJPEG_COMPOSE_ACCESS(p, what) access((p), (what))
#include "compose_kernel_body.inc"

static int run(int format) {
  const int c = format == SJPEG_HIP_SRC_RGB ? 3 : 1;
  // the overlays: 0 small random, 1 a stride above 4 * width, 2 all alpha 0, 3 all alpha 255, 4 larger than every canvas
  // but the long ones, 5 and 6 half white and half black
  std::vector<OverlayBuf> ob;
  ob.push_back(make_overlay(4, 3, 0, 2, 11u)); ob.push_back(make_overlay(5, 4, 44, 2, 12u)); ob.push_back(make_overlay(3, 3, 0, 0, 13u));
  ob.push_back(make_overlay(3, 2, 0, 1, 14u)); ob.push_back(make_overlay(40, 30, 0, 2, 15u));
  ob.push_back(make_overlay(6, 6, 0, 2, 16u)); ob.push_back(make_overlay(6, 6, 0, 2, 17u));
  for (int k = 5; k <= 6; ++k) {
    uint8_t* p = const_cast<uint8_t*>(static_cast<const uint8_t*>(ob[k].o.rgba));
    for (int i = 0; i < 36; ++i) { p[4 * i] = p[4 * i + 1] = p[4 * i + 2] = k == 5 ? 255 : 0; p[4 * i + 3] = 128; }
  }
  std::vector<sjpeg_hip_overlay> overlays;
  for (const OverlayBuf& v : ob) overlays.push_back(v.o);
  std::vector<Picture> pics;
  std::vector<sjpeg_hip_compose> cs;
  std::vector<sjpeg_hip_overlay_place> pl;
  auto frame = [&](Picture p, sjpeg_hip_compose s, std::vector<sjpeg_hip_overlay_place> places) {
    s.first_place = (int)pl.size(); s.nplaces = (int)places.size();
    pl.insert(pl.end(), places.begin(), places.end());
    pics.push_back(p); cs.push_back(s);
  };
  frame({1, 1}, compose_at(2, 2, 1, 1), {});
  for (int px = 1; px <= 3; ++px) frame({5, 3}, compose_at(10, 5, px, 1), {});          // 30 bytes a row: the last dword holds padding
  frame({5, 3}, compose_at(9, 6, 4, 3), {});                                             // touches the right and the bottom edge
  frame({250, 11}, compose_at(300, 20, 37, 5), {place_of(0, 60, 14, 0), place_of(1, 2, 2, 3)});
  frame({13, 270}, compose_at(20, 300, 3, 17), {place_of(1, 1, 150, 1), place_of(3, 0, 15, 0)});
  frame({7, 4}, compose_at(0, 0, 0, 0), {});                                             // no compose
  frame({70, 33}, compose_centred(90, 35, 0.5, 0.5), {});                                // a canvas and no place
  frame({9, 8}, compose_at(12, 10, 1, 1), {place_of(0, -2, 3, 0), place_of(0, -2, 3, 1), place_of(0, 3, -1, 0), place_of(0, 3, -1, 2),
                                            place_of(0, 50, 50, 0), place_of(0, -20, 0, 0)});   // over each edge, and wholly outside
  frame({9, 8}, compose_at(12, 10, 2, 1), {place_of(4, 0, 0, 4)});                       // over the whole canvas, padding included
  frame({9, 8}, compose_at(12, 10, 2, 1), {place_of(5, 2, 2, 0), place_of(6, 4, 3, 0)}); // two that overlap: white, then black
  frame({9, 8}, compose_at(12, 10, 2, 1), {place_of(6, 4, 3, 0), place_of(5, 2, 2, 0)}); // ... black, then white
  frame({30, 20}, compose_at(33, 22, 1, 1), {place_of(0, 0, 0, 0), place_of(1, 0, 0, 1), place_of(2, 0, 0, 2), place_of(3, 0, 0, 3), place_of(0, 0, 0, 4),
                                             place_of(5, 1, 1, 0), place_of(6, 2, 2, 4), place_of(1, 3, 3, 3)});   // eight
  frame({200, 40}, compose_centred(256, 256, 0.5, 0.5), {place_of(0, 8, 8, 3)});         // the tile: padded to a square, a logo at the corner
  frame({130, 35}, compose_at(130, 35, 0, 0), {place_of(2, 5, 5, 0), place_of(3, 64, 15, 0)});   // at its own size, under overlays on a seam
  const int n = (int)pics.size();
  Batch made = make_batch(format, pics, 5u + format);
  ComposePlan plan;
  CHECK(compose_plan("t", format, n, made.frames.data(), made.buf.get(), cs.data(), 1, overlays.data(), (int)overlays.size(), pl.data(), (int)pl.size(), &plan) == 0);
  std::unique_ptr<uint8_t[]> dst(new uint8_t[plan.bytes]);
  memset(dst.get(), 0xcd, plan.bytes);
  std::vector<ComposeFrame> desc = plan.frames;
  g_rows.clear();
  for (int k = 0; k < n; ++k) {
    ComposeFrame& d = desc[k];
    d.made = made.buf.get() + (uintptr_t)d.made; d.dst = dst.get() + (uintptr_t)d.dst;
    add_rows(d.made, d.src_stride, (int)d.h, align_up((size_t)d.w * c, 4), 0);
    add_rows(d.dst, d.dst_stride, (int)d.ch, d.dst_stride, 1);
  }
  for (const sjpeg_hip_overlay& v : overlays) add_rows(static_cast<const uint8_t*>(v.rgba), (size_t)v.stride, v.height, (size_t)4 * v.width, 2);
  std::sort(g_rows.begin(), g_rows.end(), [](const Row& a, const Row& b) { return a.lo < b.lo; });
  ComposeArgs a; a.frames = desc.data(); a.nframes = n;
  for (unsigned b = 0; b < plan.tiles + 3; ++b) {                    // (a grid larger than the plan's writes nothing more)
    for (unsigned t = 0; t < 256; ++t) {
      threadIdx_ = {t, 0, 0}; blockIdx_ = {b, 0, 0};
      if (b < plan.tiles) compose_kernel(a);
    }
  }
  CHECK(!g_bad);
  long long samples = 0;
  std::vector<uint8_t> touched(plan.bytes, 0);
  for (int k = 0; k < n; ++k) {
    int cw, ch;
    const std::vector<uint8_t> want = expect_compose(desc[k].made, desc[k].src_stride, pics[k].w, pics[k].h, c, cs[k], overlays.data(), pl.data(), &cw, &ch);
    CHECK(cw == (int)desc[k].cw && ch == (int)desc[k].ch);
    const size_t off = (uintptr_t)plan.frames[k].dst, stride = desc[k].dst_stride;
    for (int y = 0; y < ch; ++y) {
      for (size_t i = 0; i < stride; ++i) touched[off + y * stride + i] = 1;     // (a row's padding up to its last dword may be written)
      for (int i = 0; i < cw * c; ++i) {
        const uint8_t got = dst[off + y * stride + i];
        if (got != want[(size_t)y * cw * c + i]) { printf("MISMATCH format %d frame %d (%dx%d) row %d byte %d: %d want %d\n", format, k, cw, ch, y, i, got, want[(size_t)y * cw * c + i]); return 1; }
        ++samples;
      }
    }
  }
  for (size_t i = 0; i < plan.bytes; ++i) if (!touched[i]) CHECK(dst[i] == 0xcd);
  // the two orders of the overlapping overlays differ where both lie
  CHECK(memcmp(dst.get() + (uintptr_t)plan.frames[11].dst, dst.get() + (uintptr_t)plan.frames[12].dst, desc[11].dst_stride * desc[11].ch) != 0);
  printf("format %d: %lld samples equal, %u tiles, %lld + %lld + %lld aligned dwords inside their rows\n", format, samples, plan.tiles, g_accesses[0], g_accesses[1], g_accesses[2]);
  return 0;
}

int main() {
  if (plan_tests() != 0) return 1;
  for (int format : {SJPEG_HIP_SRC_RGB, SJPEG_HIP_SRC_GRAY}) if (run(format) != 0) return 1;
  printf("compose kernel emulation ok\n");
  return 0;
}
