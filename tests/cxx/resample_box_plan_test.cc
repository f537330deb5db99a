// The host half of the box entries (sjpeg_amd/csrc/resample_plan.cc: resample_box_plan, and the arithmetic of
// sjpeg_amd/csrc/resample_math.h behind it) alone, under AddressSanitizer and UndefinedBehaviorSanitizer:
// tests/test_resample_box_cxx.py builds this file with the plan by the host compiler and hands it two files written from
// tests/resample_box_model.py and tests/golden/resample_pillow_box.npz.  argv[1], decisions: what the model decides for
// random frames -- factors, safe box, reduced size, inner box, multipliers, or the refusal -- which resample_box_decide
// must repeat.  argv[2], pictures: what Pillow 12.2.0 made with Image.resize(box=, reducing_gap=), which expect_box --
// the reduce and the two passes written here from resample_math.h -- must repeat byte for byte.  Then the plan: the fixed
// points, the stages, the tables' keys, what the kernel relies on, the refusals by their words.
// resample_plan_test.cc gives the sources, the checks and the words.
#define main resample_plan_test_main
#include "resample_plan_test.cc"
#undef main

struct BoxCase { int w, h, w2, h2, filter, orient; double box[4]; double gap; };

// Image.reduce of one channel layout: src [h][w][channels] to the safe box's blocks
static std::vector<uint8_t> reduce_picture(const uint8_t* src, int w, int channels, const ResampleBoxDecision& d) {
  std::vector<uint8_t> out(static_cast<size_t>(d.W) * d.H * channels);
  for (int Y = 0; Y < d.H; ++Y) for (int X = 0; X < d.W; ++X) for (int c = 0; c < channels; ++c) {
    const int x0 = d.safe[0] + X * d.fx, y0 = d.safe[1] + Y * d.fy;
    const int x1 = std::min(x0 + d.fx, d.safe[2]), y1 = std::min(y0 + d.fy, d.safe[3]);
    uint32_t S = 0;
    for (int y = y0; y < y1; ++y) for (int x = x0; x < x1; ++x) S += src[(static_cast<size_t>(y) * w + x) * channels + c];
    const uint32_t n = static_cast<uint32_t>((x1 - x0) * (y1 - y0));
    out[(static_cast<size_t>(Y) * d.W + X) * channels + c] = static_cast<uint8_t>(resample_reduce_sample(S, n, resample_reduce_multiplier(n)));
  }
  return out;
}

// the five steps: [h2][w2][channels]; false: refused
static bool expect_box(const uint8_t* src, int w, int h, int channels, const BoxCase& c, std::vector<uint8_t>* out) {
  ResampleBoxDecision d;
  if (resample_box_decide(c.filter, w, h, c.w2, c.h2, c.box, c.gap, &d) != kBoxOk) return false;
  const std::vector<uint8_t> P = reduce_picture(src, w, channels, d);
  const float bf[4] = {static_cast<float>(d.box[0]), static_cast<float>(d.box[1]), static_cast<float>(d.box[2]), static_cast<float>(d.box[3])};
  std::vector<int32_t> xb, xk, yb, yk;
  int ksx = 1, ksy = 1;
  if (resample_box_pass_runs(d.W, c.w2, bf[0], bf[2])) {
    resample_box_table(c.filter, d.W, c.w2, bf[0], bf[2], &xb, &xk); ksx = static_cast<int>(resample_box_ksize(c.filter, bf[0], bf[2], c.w2));
  } else resample_identity_table(d.W, &xb, &xk);
  if (resample_box_pass_runs(d.H, c.h2, bf[1], bf[3])) {
    resample_box_table(c.filter, d.H, c.h2, bf[1], bf[3], &yb, &yk); ksy = static_cast<int>(resample_box_ksize(c.filter, bf[1], bf[3], c.h2));
  } else resample_identity_table(d.H, &yb, &yk);
  std::vector<uint8_t> mid(static_cast<size_t>(d.H) * c.w2 * channels);
  out->assign(static_cast<size_t>(c.h2) * c.w2 * channels, 0);
  for (int y = 0; y < d.H; ++y) for (int x = 0; x < c.w2; ++x) for (int ch = 0; ch < channels; ++ch) {
    mid[(static_cast<size_t>(y) * c.w2 + x) * channels + ch] = static_cast<uint8_t>(resample_sample(
        &xk[static_cast<size_t>(x) * ksx], P.data() + (static_cast<size_t>(y) * d.W + xb[2 * x]) * channels + ch, xb[2 * x + 1], channels));
  }
  for (int y = 0; y < c.h2; ++y) for (int x = 0; x < c.w2; ++x) for (int ch = 0; ch < channels; ++ch) {
    (*out)[(static_cast<size_t>(y) * c.w2 + x) * channels + ch] = static_cast<uint8_t>(resample_sample(
        &yk[static_cast<size_t>(y) * ksy], &mid[(static_cast<size_t>(yb[2 * y]) * c.w2 + x) * channels + ch], yb[2 * y + 1], static_cast<long long>(c.w2) * channels));
  }
  return true;
}

template <class T> static bool get(FILE* f, T* v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }

static int decisions(const char* path, int* count) {
  FILE* f = fopen(path, "rb");
  CHECK(f != nullptr);
  int32_t n = 0;
  CHECK(get(f, &n));
  for (int k = 0; k < n; ++k) {
    int32_t in[5], code, want_i[8]; uint32_t want_m[4]; double box[4], gap, want_box[4];
    CHECK(get(f, in, 5) && get(f, box, 4) && get(f, &gap) && get(f, &code) && get(f, want_i, 8) && get(f, want_m, 4) && get(f, want_box, 4));
    ResampleBoxDecision d;
    const int got = resample_box_decide(in[0], in[1], in[2], in[3], in[4], box, gap, &d);
    if (got != code) printf("case %d: %d want %d\n", k, got, code);
    CHECK(got == code);
    if (code != kBoxOk) continue;
    CHECK(d.fx == want_i[0] && d.fy == want_i[1] && d.W == want_i[6] && d.H == want_i[7]);
    for (int i = 0; i < 4; ++i) CHECK(d.safe[i] == want_i[2 + i] && d.m[i] == want_m[i] && d.box[i] == want_box[i]);
    // what the kernel relies on: the safe box inside the picture, every block inside the safe box and not empty
    CHECK(0 <= d.safe[0] && d.safe[0] < d.safe[2] && d.safe[2] <= in[1] && 0 <= d.safe[1] && d.safe[1] < d.safe[3] && d.safe[3] <= in[2]);
    CHECK(d.safe[0] + (d.W - 1) * d.fx < d.safe[2] && d.safe[0] + d.W * d.fx >= d.safe[2]);
    CHECK(d.safe[1] + (d.H - 1) * d.fy < d.safe[3] && d.safe[1] + d.H * d.fy >= d.safe[3]);
  }
  fclose(f);
  *count = n;
  return 0;
}

static int pictures(const char* path, int* count) {
  FILE* f = fopen(path, "rb");
  CHECK(f != nullptr);
  int32_t n = 0;
  CHECK(get(f, &n));
  for (int k = 0; k < n; ++k) {
    int32_t in[6];
    BoxCase c;
    CHECK(get(f, in, 6) && get(f, c.box, 4) && get(f, &c.gap));
    c.filter = in[0]; c.w = in[1]; c.h = in[2]; c.w2 = in[4]; c.h2 = in[5]; c.orient = 1;
    std::vector<uint8_t> src(static_cast<size_t>(c.w) * c.h * in[3]), want(static_cast<size_t>(c.w2) * c.h2 * in[3]), got;
    CHECK(get(f, src.data(), src.size()) && get(f, want.data(), want.size()));
    CHECK(expect_box(src.data(), c.w, c.h, in[3], c, &got));
    if (got != want) printf("picture %d differs from Pillow's\n", k);
    CHECK(got == want);
  }
  fclose(f);
  *count = n;
  return 0;
}

static int plan_checks() {
  Source s = make_source(400, 200, 3, 5);
  const sjpeg_hip_resample bicubic = {SJPEG_HIP_RESAMPLE_BICUBIC, {0, 0, 0}}, lanczos = {SJPEG_HIP_RESAMPLE_LANCZOS, {0, 0, 0}};
  const int32_t size[1][2] = {{100, 50}};
  ResamplePlan plain, plan;
  CHECK(resample_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, size, nullptr, &bicubic, 0, nullptr, &plain) == 0);
  // ---- the fixed points: the whole box without a gap, the all-zero box, a gap whose factors are 1: the parent's plan
  const sjpeg_hip_resample_box same[] = {{{0, 0, 0, 0}, 0}, {{0, 0, 400, 200}, 0}, {{0, 0, 0, 0}, 2.5}, {{0, 0, 400, 200}, 4.0}};
  for (const sjpeg_hip_resample_box& b : same) {
    CHECK(resample_box_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, size, nullptr, &bicubic, 0, &b, 0, nullptr, &plan) == 0);
    CHECK(plan.stages.empty() && plan.tables == plain.tables && plan.ntables == plain.ntables && plan.tiles == plain.tiles && plan.bytes == plain.bytes);
    CHECK(memcmp(&plan.frames[0], &plain.frames[0], sizeof(ResampleFrame)) == 0);
  }
  // ---- a gap that reduces: factors 2 x 2 of 400 x 200 to 100 x 50, the tables those of the reduced picture
  const sjpeg_hip_resample_box two = {{0, 0, 0, 0}, 2.0};
  CHECK(resample_box_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, size, nullptr, &bicubic, 0, &two, 0, nullptr, &plan) == 0);
  CHECK(plan.stages.size() == 1 && plan.stages[0].fx == 2 && plan.stages[0].fy == 2 && plan.stages[0].w == 400 && plan.stages[0].h == 200);
  CHECK(plan.frames[0].W == 200 && plan.frames[0].H == 100 && plan.frames[0].ksx == 9 && plan.bytes == plain.bytes && plan.stages[0].m[0] == (1u << 22));
  // ---- a mixed batch: the frames in front of the first reduced one get the stage of a picture that is not reduced
  {
    Source a = make_source(64, 48, 3, 1), b = make_source(37, 29, 3, 2), c = make_source(20, 20, 3, 3);
    const sjpeg_hip_ragged_frame frames[3] = {a.frame, b.frame, c.frame};
    const int32_t sizes[3][2] = {{30, 30}, {6, 7}, {25, 9}};
    const sjpeg_hip_resample_box boxes[3] = {{{1.5, 2.5, 60, 40}, 0}, {{0, 0, 0, 0}, 2.0}, {{0, 0, 20, 20}, 2.0}};
    CHECK(resample_box_plan("t", SJPEG_HIP_SRC_RGB, 3, frames, sizes, nullptr, &bicubic, 0, boxes, 1, nullptr, &plan) == 0);
    CHECK(plan.stages.size() == 3 && plan.stages[0].fx == 1 && plan.stages[0].w == 64 && plan.stages[0].h == 48 && plan.stages[0].m[3] == (1u << 24));
    CHECK(plan.stages[1].fx == 3 && plan.stages[1].fy == 2 && plan.stages[2].fx == 1 && plan.stages[2].fy == 1 && plan.stages[2].w == 20);
    CHECK(plan.frames[1].W == 13 && plan.frames[1].H == 15);
    // (9, 6, 3 and 2 samples a block: all four multipliers are in play)
    CHECK(plan.stages[1].m[0] == resample_reduce_multiplier(6) && plan.stages[1].m[1] == resample_reduce_multiplier(2) &&
          plan.stages[1].m[2] == resample_reduce_multiplier(3) && plan.stages[1].m[3] == resample_reduce_multiplier(1));
    // no frame reduced: no stages, and a box is a table of its own
    const sjpeg_hip_resample_box none[3] = {{{1.5, 2.5, 60, 40}, 0}, {{0, 0, 0, 0}, 0}, {{0.5, 0, 20, 20}, 0}};
    CHECK(resample_box_plan("t", SJPEG_HIP_SRC_RGB, 3, frames, sizes, nullptr, &bicubic, 0, none, 1, nullptr, &plan) == 0 && plan.stages.empty());
    CHECK(plan.ntables == 6);
    // (a box with the target's own size still runs the pass: 20 -> 20 from 0.5 is no identity)
    const int32_t own[3][2] = {{64, 48}, {37, 29}, {20, 20}};
    CHECK(resample_box_plan("t", SJPEG_HIP_SRC_RGB, 3, frames, own, nullptr, &bicubic, 0, none, 1, nullptr, &plan) == 0);
    CHECK(plan.frames[1].ksx == 1 && plan.frames[1].ksy == 1 && plan.frames[2].ksx == 5 && plan.frames[2].ksy == 1 && plan.frames[0].ksx == 5);
  }
  // ---- the limit the reduce lifts: 4000 -> 40 with Lanczos is refused by the plain entry and a factor of 50 here
  {
    Source g = make_source(4000, 8, 1, 9);
    const int32_t small[1][2] = {{40, 4}};
    CHECK(resample_plan("t", SJPEG_HIP_SRC_GRAY, 1, &g.frame, small, nullptr, &lanczos, 0, nullptr, &plan) == SJPEG_HIP_EINVAL && said("above the cap of 385"));
    CHECK(resample_box_plan("t", SJPEG_HIP_SRC_GRAY, 1, &g.frame, small, nullptr, &lanczos, 0, &two, 0, nullptr, &plan) == 0);
    CHECK(plan.stages[0].fx == 50 && plan.stages[0].fy == 1 && plan.frames[0].W == 80 && plan.frames[0].ksx == 13);
    CHECK(sjpeg_hip_resample_box_ragged_bytes(SJPEG_HIP_SRC_GRAY, 1, &g.frame, small, nullptr, &two, 0) == plan.bytes && plan.bytes == 40 * 4);
    const sjpeg_hip_resample_box nogap = {{0, 0, 0, 0}, 0};
    CHECK(resample_box_plan("t", SJPEG_HIP_SRC_GRAY, 1, &g.frame, small, nullptr, &lanczos, 0, &nogap, 0, nullptr, &plan) == SJPEG_HIP_EINVAL && said("above the cap of 385"));
  }
  // ---- the refusals, by name
  const struct { sjpeg_hip_resample_box b; const char* words; } bad[] = {
      {{{0, 0, 400.5, 200}, 0}, "frame 0: box (0.000000, 0.000000, 400.500000, 200.000000) is empty or leaves the 400x200 picture"},
      {{{-1, 0, 400, 200}, 0}, "is empty or leaves"}, {{{5, 5, 5, 9}, 0}, "is empty or leaves"}, {{{5, 9, 50, 9}, 0}, "is empty or leaves"},
      {{{0, 0, 0, 0}, 0.99}, "frame 0: reducing_gap 0.990000 is not 0 (none) or 1.0 .. 65536.0"}, {{{0, 0, 0, 0}, -2}, "reducing_gap"}};
  for (const auto& c : bad) {
    CHECK(resample_box_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, size, nullptr, &bicubic, 0, &c.b, 0, nullptr, &plan) == SJPEG_HIP_EINVAL && said(c.words));
    CHECK(plan.frames.empty() && plan.stages.empty());
  }
  CHECK(resample_box_plan("t", SJPEG_HIP_SRC_RGB, 1, &s.frame, size, nullptr, &bicubic, 0, nullptr, 0, nullptr, &plan) == SJPEG_HIP_EINVAL && said("t: box == NULL"));
  {
    Source wide = make_source(60000, 2, 1, 3), tall = make_source(2, 300, 1, 4);
    const int32_t tiny[1][2] = {{40, 1}}, shorter[1][2] = {{2, 299}}, taller[1][2] = {{2, 301}}, as_is[1][2] = {{1, 300}};
    const sjpeg_hip_resample_box one = {{0, 0, 0, 0}, 1.0}, nogap = {{0, 0, 0, 0}, 0};
    CHECK(resample_box_plan("t", SJPEG_HIP_SRC_GRAY, 1, &wide.frame, tiny, nullptr, &bicubic, 0, &one, 0, nullptr, &plan) == SJPEG_HIP_EINVAL);
    CHECK(said("frame 0: reduce factors 1500x2 are above the cap of 255"));
    CHECK(resample_box_plan("t", SJPEG_HIP_SRC_GRAY, 1, &tall.frame, shorter, nullptr, &bicubic, 0, &nogap, 0, nullptr, &plan) == SJPEG_HIP_EINVAL);
    CHECK(said("frame 0: a picture of 2x300 samples, more than 100 times as tall as wide, brought to fewer rows is not made"));
    CHECK(resample_box_plan("t", SJPEG_HIP_SRC_GRAY, 1, &tall.frame, taller, nullptr, &bicubic, 0, &nogap, 0, nullptr, &plan) == 0);
    CHECK(resample_box_plan("t", SJPEG_HIP_SRC_GRAY, 1, &tall.frame, as_is, nullptr, &bicubic, 0, &nogap, 0, nullptr, &plan) == 0);
    // (the plain entry does not refuse it: its behaviour is unchanged)
    CHECK(resample_plan("t", SJPEG_HIP_SRC_GRAY, 1, &tall.frame, shorter, nullptr, &bicubic, 0, nullptr, &plan) == 0);
  }
  // ---- the host entries
  int32_t size2[2]; double crop[4]; int32_t b[4][2], K[4 * 7];
  CHECK(sjpeg_hip_thumbnail_size(1920, 1080, 256, 256, size2) == 0 && size2[0] == 256 && size2[1] == 144);
  CHECK(sjpeg_hip_thumbnail_size(100, 50, 256, 256, size2) == 0 && size2[0] == 100 && size2[1] == 50);
  CHECK(sjpeg_hip_thumbnail_size(100, 50, 0.5, 256, size2) == SJPEG_HIP_EINVAL && said("below 1x1"));
  CHECK(sjpeg_hip_fit_crop(1920, 1080, 256, 256, 0, 0.5, 0.5, crop) == 0 && crop[0] == 420 && crop[1] == 0 && crop[2] == 1500 && crop[3] == 1080);
  CHECK(sjpeg_hip_fit_crop(1920, 1080, 0, 256, 0, 0.5, 0.5, crop) == SJPEG_HIP_EINVAL);
  CHECK(sjpeg_hip_resample_box_ksize(SJPEG_HIP_RESAMPLE_LANCZOS, 2, 4, 0.0f, 2.0f) == 7 && sjpeg_hip_resample_box_ksize(4, 2, 4, 1.0f, 1.0f) == 0 && said("leaves the axis"));
  CHECK(sjpeg_hip_resample_box_table(SJPEG_HIP_RESAMPLE_LANCZOS, 2, 4, 0.0f, 2.0f, b, K, 27) == SJPEG_HIP_EINVAL && said("K_capacity 27 is below the 28"));
  CHECK(sjpeg_hip_resample_box_table(SJPEG_HIP_RESAMPLE_LANCZOS, 2, 4, 0.5f, 2.0f, b, K, 28) == 0 && b[3][0] + b[3][1] == 2);
  sjpeg_hip_resample_box_decision dec;
  CHECK(sjpeg_hip_resample_box_decide(SJPEG_HIP_RESAMPLE_BICUBIC, 37, 29, 6, 7, &two, &dec) == 0 && dec.factor[0] == 3 && dec.factor[1] == 2);
  CHECK(dec.reduced_size[0] == 13 && dec.reduced_size[1] == 15 && dec.safe_box[2] == 37 && dec.inner_box[2] == 37.0 / 3);
  return 0;
}

#ifndef RESAMPLE_BOX_NO_MAIN
int main(int argc, char** argv) {
  CHECK(argc == 3);
  int nd = 0, np = 0;
  if (decisions(argv[1], &nd) != 0 || pictures(argv[2], &np) != 0 || plan_checks() != 0) return 1;
  // every block size the entries take: the product stays inside a uint32; a block of zeros is 0; a block of 255s is 255
  // for every block of up to 64 x 64 samples, and 255 or 254 beyond -- the truncated multiplier's answer, and Pillow's
  int dim = 0;
  for (uint32_t fx = 1; fx <= 255; ++fx) for (uint32_t fy = 1; fy <= 255; ++fy) {
    const uint32_t n = fx * fy, m = resample_reduce_multiplier(n), white = resample_reduce_sample(255u * n, n, m);
    CHECK(resample_reduce_fits(n) && resample_reduce_sample(0u, n, m) == 0u);
    CHECK(white == 255u || (white == 254u && n > 64u * 64u));
    dim += white == 254u;
  }
  printf("resample box plan ok: %d decisions, %d pictures equal to Pillow's (%d of 65025 block shapes bring 255s to 254)\n", nd, np, dim);
  return 0;
}
#endif
