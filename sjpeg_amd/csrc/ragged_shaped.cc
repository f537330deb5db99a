// ragged_shaped.cc -- the ragged entries on pictures that are SHAPED inside the call: reduced by a factor (reduce.hip),
// resized to a size, turned upright by an EXIF orientation and flattened over a background (resize.hip), the same for
// the YUV-plane formats (yuv_resize_plan.cc), their samples bytes or 16-bit words, and placed into contact sheets
// (sheet_plan.cc), sharpened by the unsharp mask behind any of it but a sheet (unsharp_plan.cc, unsharp.hip), and
// resampled with Pillow's filters, enlarging too (resample_plan.cc, resample.hip), and filtered by Pillow's BoxBlur,
// GaussianBlur or UnsharpMask behind that (pillow_filter_plan.cc, pillow_filter.hip), and composed behind that: onto a
// canvas, under overlays (compose_plan.cc, compose.hip).  Per family a shape entry -- the made pictures into the
// caller's buffer -- and an encode entry with its packed twin: the pictures into the engine's memory and ONE _full_ call
// (ragged_full.cc) over them.  Host code only.
//
// Every entry fills a Shape by name -- what it asks for beyond its frames --, makes its call (Make: a shape entry's,
// Encode: an encode entry's, around ragged_aux.h's RaggedCall) and hands both to its family's RULE.  A rule states the
// family's decisions once, for both kinds of call: its mandatory pointers, when there is nothing for it to do and which
// family's rule the call then goes to -- under that family's name, which its messages then carry --, and the plan KIND
// it runs.  The bodies -- shape_body, planned_flow, sheet_flow -- are written once against the kinds.  Every check comes
// before the engine is touched; their order and texts are pinned by tests/golden/c_messages.json.  DESIGN.md, "The C
// layer's call description".
#include <stdint.h>

#include <string>
#include <vector>

#include "ragged_aux.h"
#include "sjpeg_hip.h"

namespace {

using namespace sjpeg_internal;
using Frame = sjpeg_hip_ragged_frame;

// ---- what an entry asks for beyond its frames (NULL: not that).  An array that is one for the call or one per frame
// travels with its flag, the overlays and places with their counts
template <class T> struct PerFrame { const T* p = nullptr; int per_frame = 0; };
template <class T> struct Counted { const T* p = nullptr; int n = 0; };
struct Shape {
  const uint8_t* factors = nullptr;
  const int32_t (*sizes)[2] = nullptr;
  const uint8_t* orientations = nullptr;
  const sjpeg_hip_flatten* flatten = nullptr;
  const sjpeg_hip_sheet* sheet = nullptr;
  const sjpeg_hip_yuv_depth* depth = nullptr;
  int light = SJPEG_HIP_LIGHT_CODED;
  PerFrame<sjpeg_hip_yuv_colour> colour;
  PerFrame<sjpeg_hip_unsharp> unsharp;
  PerFrame<sjpeg_hip_resample> resample;
  PerFrame<sjpeg_hip_resample_box> box;
  PerFrame<sjpeg_hip_pillow_filter> filter;
  PerFrame<sjpeg_hip_compose> compose;
  Counted<sjpeg_hip_overlay> overlays;
  Counted<sjpeg_hip_overlay_place> places;
};

// where made pictures stand while a call is checked: there is no memory for them yet, and the checks read no sample
uint8_t* const kNoMemoryYet = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(16));

// ---- the plan kinds: the plan function, the format of what it makes, the made pictures as frames at `base` and how
// many they are, the engine's half, and the hint behind a refused yuv_mode
struct PerFrameKind {                            // (one made picture per frame; the format is any the plan takes)
  static constexpr bool yuv_only = false, sheets = false;
  static constexpr int esz = 0;                  // (the size of a sample where it is not the format's own: ragged_check)
  template <class P> static int count(const P&, int nframes) { return nframes; }
  template <class P> static const char* mode_hint(const P&) { return " (gray pictures are coded 4:0:0 only)"; }
};
struct ReduceKind : PerFrameKind {
  using Plan = ReducePlan;
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    return reduce_plan(who, format, n, fr, s.factors, p);
  }
  static int format(const Plan& p) { return p.reduced_format; }
  static void frames(const Plan& p, const Frame* fr, uint8_t* base, Frame* out) { reduce_plan_frames(p, fr, base, out); }
  static constexpr auto run = engine_reduce;
};
struct ResizeKind : PerFrameKind {               // (with optional orientations and flatten)
  using Plan = ResizePlan;
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    return resize_plan(who, format, n, fr, s.sizes, s.orientations, p, s.flatten);
  }
  static int format(const Plan& p) { return p.resized_format; }
  static void frames(const Plan& p, const Frame* fr, uint8_t* base, Frame* out) { resize_plan_frames(p, fr, base, out); }
  static constexpr auto run = engine_resize;
};
struct YuvResizeKind : PerFrameKind {
  using Plan = YuvResizePlan;
  static constexpr bool yuv_only = true;         // (the format is checked by name, in front of nframes)
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    return yuv_resize_plan(who, format, n, fr, s.sizes, s.orientations, p);
  }
  static int format(const Plan& p) { return p.resized_format; }
  static void frames(const Plan& p, const Frame* fr, uint8_t* base, Frame* out) { yuv_resize_plan_frames(p, fr, base, out); }
  static constexpr auto run = engine_yuv_resize;
  static const char* mode_hint(const Plan&) { return ""; }
};
struct SheetKind : PerFrameKind {                // (its frames count sheets: out_offset and out_capacity 0)
  using Plan = SheetPlan;
  static constexpr bool sheets = true;
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    return sheet_plan(who, format, n, fr, s.sheet, s.sizes, s.orientations, p, s.flatten);
  }
  static int format(const Plan& p) { return p.out_format; }
  static int count(const Plan& p, int) { return p.nsheets; }
  static const char* mode_hint(const Plan& p) { return p.yuv ? "" : PerFrameKind::mode_hint(p); }
  static void frames(const Plan& p, const Frame*, uint8_t* base, Frame* out) { sheet_plan_frames(p, base, out); }
  static constexpr auto run = engine_sheet;
};

// ... and the two whose planes are converted to JFIF's colour behind the resize launch (yuv_colour_plan.cc): the plan of
// the kind they extend plus the colour launch's, the engine's half of the one and then of the other
struct YuvColourKind : YuvResizeKind {
  struct Plan : YuvResizePlan { YuvColourPlan colour; };
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    if (int rc = YuvResizeKind::plan(who, format, n, fr, s, p)) return rc;
    return yuv_colour_plan(who, *p, s.colour.p, s.colour.per_frame, &p->colour);
  }
  static int run(sjpeg_hip_engine* e, const std::string& who, const Plan& p, uint8_t* d_out, uint8_t** base, void* stream) {
    uint8_t* at = nullptr;
    if (int rc = engine_yuv_resize(e, who, p, d_out, &at, stream)) return rc;
    if (base != nullptr) *base = at;
    return engine_yuv_colour(e, who, p.colour, at, stream);
  }
};
struct SheetColourKind : SheetKind {             // (the thumbnails' rectangles alone: the background stays as given)
  struct Plan : SheetPlan { YuvColourPlan colour; };
  static constexpr bool yuv_only = true;
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    if (int rc = yuv_format_check(who, format)) return rc;
    if (int rc = SheetKind::plan(who, format, n, fr, s, p)) return rc;
    return yuv_colour_plan(who, p->planes, s.colour.p, s.colour.per_frame, &p->colour);
  }
  static int run(sjpeg_hip_engine* e, const std::string& who, const Plan& p, uint8_t* d_out, uint8_t** base, void* stream) {
    uint8_t* at = nullptr;
    if (int rc = engine_sheet(e, who, p, d_out, &at, stream)) return rc;
    if (base != nullptr) *base = at;
    return engine_yuv_colour(e, who, p.colour, at, stream);
  }
};

// ... and the two on planes of 16-bit samples (sjpeg_hip_yuv_depth): the same plans marked deep, so the engine's half
// runs the kernel's deep instantiations; the made planes are bytes, and everything behind them is the colour kinds'
struct YuvDeepKind : YuvColourKind {
  static constexpr int esz = 2;
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    if (int rc = yuv_depth_check(who, s.depth)) return rc;
    if (int rc = yuv_resize_plan(who, format, n, fr, s.sizes, s.orientations, p, s.depth)) return rc;
    return yuv_colour_plan(who, *p, s.colour.p, s.colour.per_frame, &p->colour);
  }
};
struct SheetDeepKind : SheetColourKind {
  static constexpr int esz = 2;
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    if (int rc = yuv_format_check(who, format)) return rc;
    if (int rc = yuv_depth_check(who, s.depth)) return rc;
    if (int rc = sheet_plan(who, format, n, fr, s.sheet, s.sizes, s.orientations, p, nullptr, s.depth)) return rc;
    return yuv_colour_plan(who, p->planes, s.colour.p, s.colour.per_frame, &p->colour);
  }
};

// ... and the two in linear light (sjpeg_hip_linear_ragged_src): the resize and sheet plans marked with the light, so
// the engine's half runs the kernel's linear instantiations; a YUV-plane format is refused by name in front of the plan
struct LinearKind : ResizeKind {
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    if (int rc = light_check(who, s.light, format)) return rc;
    if (int rc = ResizeKind::plan(who, format, n, fr, s, p)) return rc;
    p->light = s.light;
    return 0;
  }
};
struct SheetLinearKind : SheetKind {
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    if (int rc = light_check(who, s.light, format)) return rc;
    if (int rc = SheetKind::plan(who, format, n, fr, s, p)) return rc;
    p->rgb.light = s.light;
    return 0;
  }
};

// ... and the one that resamples with Pillow's filters (sjpeg_hip_resample_ragged_src; resample_plan.cc, resample.hip):
// a kernel and tables of its own, the resize kind's layout -- sizes may exceed the source, there is no light
struct ResampleKind : PerFrameKind {
  using Plan = ResamplePlan;
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    return resample_plan(who, format, n, fr, s.sizes, s.orientations, s.resample.p, s.resample.per_frame, s.flatten, p);
  }
  static int format(const Plan& p) { return p.resized_format; }
  static void frames(const Plan& p, const Frame* fr, uint8_t* base, Frame* out) { resample_plan_frames(p, fr, base, out); }
  static constexpr auto run = engine_resample;
};
// ... from a source box and behind a reduce (sjpeg_hip_resample_box_ragged_src; resample_box.hip where a frame is reduced)
struct ResampleBoxKind : ResampleKind {
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    return resample_box_plan(who, format, n, fr, s.sizes, s.orientations, s.resample.p, s.resample.per_frame, s.box.p, s.box.per_frame, s.flatten, p);
  }
};

// the pictures a per-frame kind K makes, read off its plan before there is memory for them: what a stage behind K plans on
template <class K>
std::vector<Frame> made_pictures(const typename K::Plan& p, const Frame* fr, int n) {
  std::vector<Frame> made(static_cast<size_t>(n));
  K::frames(p, fr, kNoMemoryYet, made.data());
  return made;
}

// ... and any per-frame kind K with ONE STAGE behind it on K's own layout: K's plan, then the stage's plan of the
// pictures K makes; K's pictures into the engine's memory, then the stage's launches from there to the caller's buffer
// or the engine's final pictures.  Frames and format are K's.  A stage states its plan function with its argument pair
// in Shape, and the engine's half:
struct UnsharpStage {                            // (the unsharp mask: unsharp_plan.cc, unsharp.hip -- one launch)
  using Plan = UnsharpPlan;
  static int plan(const std::string& who, int format, int n, const Frame* made, const Shape& s, Plan* p) {
    return unsharp_plan(who, format, n, made, kNoMemoryYet, s.unsharp.p, s.unsharp.per_frame, p);
  }
  static constexpr auto run = engine_unsharp;
};
struct FilterStage {                             // (Pillow's filters: pillow_filter_plan.cc, pillow_filter.hip -- two launches)
  using Plan = PillowFilterPlan;
  static int plan(const std::string& who, int format, int n, const Frame* made, const Shape& s, Plan* p) {
    return pillow_filter_plan(who, format, n, made, kNoMemoryYet, s.filter.p, s.filter.per_frame, p);
  }
  static constexpr auto run = engine_pillow_filter;
};
template <class K, class Stage>
struct Behind : K {
  struct Plan : K::Plan { typename Stage::Plan stage; };
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    if (int rc = K::plan(who, format, n, fr, s, p)) return rc;
    if (int rc = Stage::plan(who, K::format(*p), n, made_pictures<K>(*p, fr, n).data(), s, &p->stage)) return rc;
    p->stage.bytes = p->bytes;
    return 0;
  }
  static int run(sjpeg_hip_engine* e, const std::string& who, const Plan& p, uint8_t* d_out, uint8_t** base, void* stream) {
    uint8_t* staged = nullptr;
    if (int rc = K::run(e, who, p, nullptr, &staged, stream)) return rc;
    return Stage::run(e, who, p.stage, staged, d_out, base, stream);
  }
};
template <class K> using UnsharpKind = Behind<K, UnsharpStage>;
template <class K> using FilterKind = Behind<K, FilterStage>;

// ... and any per-frame kind K with the compose stage behind it (compose_plan.cc, compose.hip): K's plan, then the
// compose plan over the pictures K makes; K's pictures into the engine's memory, then the one compose launch from there
// to the caller's buffer or the engine's composed pictures.  Unlike Behind it OWNS frames(), bytes and the sizes: the
// canvases are not K's layout
template <class K>
struct ComposeKind : PerFrameKind {
  struct Plan {
    typename K::Plan made;
    ComposePlan compose;
    size_t bytes = 0;
  };
  static constexpr bool yuv_only = K::yuv_only;
  static constexpr int esz = K::esz;
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    if (int rc = K::plan(who, format, n, fr, s, &p->made)) return rc;
    if (int rc = compose_plan(who, K::format(p->made), n, made_pictures<K>(p->made, fr, n).data(), kNoMemoryYet, s.compose.p, s.compose.per_frame,
                              s.overlays.p, s.overlays.n, s.places.p, s.places.n, &p->compose)) {
      return rc;
    }
    p->bytes = p->compose.bytes;
    return 0;
  }
  static int format(const Plan& p) { return K::format(p.made); }
  static void frames(const Plan& p, const Frame* fr, uint8_t* base, Frame* out) { compose_plan_frames(p.compose, fr, base, out); }
  static int run(sjpeg_hip_engine* e, const std::string& who, const Plan& p, uint8_t* d_out, uint8_t** base, void* stream) {
    uint8_t* staged = nullptr;
    if (int rc = K::run(e, who, p.made, nullptr, &staged, stream)) return rc;
    return engine_compose(e, who, p.compose, staged, d_out, base, stream);
  }
};

int source_mode(const SourceLayout* L) { return L->implied != 0 ? L->implied : SJPEG_HIP_YUV444; }

// ---- the families: the names of the encode entry ([0]) and its packed twin ([1]) and of the shape entry, and the words
// of the shape entry's messages -- its mandatory pointers, its buffer, its size argument, what it makes and the _bytes
// function that says how much that takes
struct ShapeWords { const char *pointers, *buffer, *bytes, *made, *bytes_fn; };
struct Family {
  std::string encode[2], make;
  ShapeWords words;
};
constexpr ShapeWords picture_words(const char* made, const char* bytes_fn) {
  return {"frames, d_out, out_frames or out_format", "d_out", "bytes", made, bytes_fn};
}
constexpr ShapeWords kOrientWords = picture_words("oriented pictures", "sjpeg_hip_orient_ragged_bytes");
constexpr ShapeWords kSheetWords = {"frames, sheet, d_out, sheet_frames, nsheets or out_format", "d_out", "bytes", "sheets",
                                    "sjpeg_hip_sheet_ragged_bytes"};
constexpr ShapeWords kYuvWords = picture_words("converted planes", "sjpeg_hip_resize_ragged_yuv_bytes");
#define SJPEG_ENCODERS(stem) {"sjpeg_hip_encode_ragged_" stem "_src", "sjpeg_hip_encode_ragged_" stem "_packed_src"}
const Family
    kReduced = {SJPEG_ENCODERS("reduced"), "sjpeg_hip_reduce_ragged_src",
                {"frames, factors, d_reduced, reduced_frames or reduced_format", "d_reduced", "reduced_bytes", "reduced pictures",
                 "sjpeg_hip_reduce_ragged_bytes"}},
    kResized = {SJPEG_ENCODERS("resized"), "sjpeg_hip_resize_ragged_src",
                {"frames, sizes, d_resized, resized_frames or resized_format", "d_resized", "resized_bytes", "resized pictures",
                 "sjpeg_hip_resize_ragged_bytes"}},
    kOriented = {SJPEG_ENCODERS("oriented"), "sjpeg_hip_orient_ragged_src", kOrientWords},
    kFlattened = {SJPEG_ENCODERS("flattened"), "sjpeg_hip_flatten_ragged_src", kOrientWords},
    kYuvResized = {SJPEG_ENCODERS("yuv_resized"), "sjpeg_hip_resize_ragged_yuv_src", picture_words("resized planes", kYuvWords.bytes_fn)},
    kSheet = {SJPEG_ENCODERS("sheet"), "sjpeg_hip_sheet_ragged_src", kSheetWords},
    kSheetFlat = {SJPEG_ENCODERS("sheet_flat"), "sjpeg_hip_sheet_ragged_flat_src", kSheetWords},
    kYuvConverted = {SJPEG_ENCODERS("yuv_converted"), "sjpeg_hip_convert_ragged_yuv_src", kYuvWords},
    kSheetColour = {SJPEG_ENCODERS("sheet_yuv_colour"), "sjpeg_hip_sheet_ragged_yuv_colour_src", kSheetWords},
    kYuv16 = {SJPEG_ENCODERS("yuv16"), "sjpeg_hip_convert_ragged_yuv16_src", kYuvWords},
    kSheetYuv16 = {SJPEG_ENCODERS("sheet_yuv16"), "sjpeg_hip_sheet_ragged_yuv16_src", kSheetWords},
    kLinear = {SJPEG_ENCODERS("linear"), "sjpeg_hip_linear_ragged_src", kOrientWords},
    kSheetLinear = {SJPEG_ENCODERS("sheet_linear"), "sjpeg_hip_sheet_ragged_linear_src", kSheetWords},
    kUnsharp = {SJPEG_ENCODERS("unsharp"), "sjpeg_hip_unsharp_ragged_src", kOrientWords},
    kYuvUnsharp = {SJPEG_ENCODERS("yuv_unsharp"), "sjpeg_hip_unsharp_ragged_yuv_src", picture_words("sharpened planes", kYuvWords.bytes_fn)},
    kResampled = {SJPEG_ENCODERS("resampled"), "sjpeg_hip_resample_ragged_src",
                  picture_words("resampled pictures", "sjpeg_hip_resample_ragged_bytes")},
    kResampledBox = {SJPEG_ENCODERS("resampled_box"), "sjpeg_hip_resample_box_ragged_src",
                     picture_words("resampled pictures", "sjpeg_hip_resample_box_ragged_bytes")},
    kFiltered = {SJPEG_ENCODERS("filtered"), "sjpeg_hip_filter_ragged_src",
                 picture_words("filtered pictures", "sjpeg_hip_resample_box_ragged_bytes")},
    kComposed = {SJPEG_ENCODERS("composed"), "sjpeg_hip_compose_ragged_src", picture_words("composed pictures", "sjpeg_hip_compose_ragged_bytes")};
#undef SJPEG_ENCODERS

// ---- a shape entry's call: the made pictures into the caller's buffer
struct Pictures {                                // what every entry starts with
  sjpeg_hip_engine* e;
  int format, nframes;
  const Frame* frames;
};
struct MadeOut {                                 // where a shape entry's pictures and answers go
  void* d_out;
  size_t bytes;
  Frame* out_frames;
  int* count;                                    // where the number of made pictures goes (NULL: it is nframes)
  int* out_format;
  void* stream;
};
MadeOut pictures_into(void* d_out, size_t bytes, Frame* out_frames, int* out_format, void* stream) {
  return {d_out, bytes, out_frames, nullptr, out_format, stream};
}
struct Make;
template <class K> int shape_body(const Make& m, const Shape& s, bool missing);
template <class K> int planned_flow(const RaggedCall& c, const Shape& s);
template <class K> int sheet_flow(const RaggedCall& c, const Shape& s);

// ---- the two FINISHERS a rule is written against: whose name the call goes by, how its checks begin and what runs the
// kind the rule ends in.  enter(): the call now goes by this family's name
struct Make {                                    // (a shape entry's call: ends in shape_body<K>)
  static constexpr bool encodes = false;
  Pictures p;
  MadeOut out;
  const Family* family = nullptr;
  void enter(const Family& f) { family = &f; }
  const std::string& who() const { return family->make; }
  int format() const { return p.format; }
  int nframes() const { return p.nframes; }
  const Frame* frames() const { return p.frames; }
  // (the engine alone, in front of a rule's own checks: the rest of a shape entry's are shape_body's)
  int begin(bool = false, const void* = nullptr, bool = false) const {
    return p.e == nullptr ? set_error(SJPEG_HIP_EINVAL, who() + ": engine == NULL") : 0;
  }
  // (missing: a pointer that only this entry refuses as NULL; a sheet kind wants its sheet and nsheets)
  template <class K> int run(const Shape& s, bool missing = false) const {
    return shape_body<K>(*this, s, missing || (K::sheets && (s.sheet == nullptr || out.count == nullptr)));
  }
};
struct Encode {                                  // (an encode entry's call: ends in planned_flow<K>, a sheet kind in sheet_flow<K>)
  static constexpr bool encodes = true;
  RaggedCall c;
  void enter(const Family& f) { c.who = &f.encode[c.out.packed]; }
  const std::string& who() const { return *c.who; }
  int format() const { return c.format; }
  int nframes() const { return c.nframes; }
  const Frame* frames() const { return c.frames; }
  int begin(bool has_sheet = false, const void* sheet = nullptr, bool yuv_only = false) const {
    return encode_prologue(c, has_sheet, sheet, yuv_only);
  }
  template <class K> int run(const Shape& s, bool = false) const {
    if constexpr (K::sheets) return sheet_flow<K>(c, s); else return planned_flow<K>(c, s);
  }
};
struct Meta { const sjpeg_hip_metadata* meta; int per_frame; };
Encode encode(const Pictures& p, const sjpeg_hip_ragged_params* params, const Meta& m, const RaggedOut& out) {
  return {{nullptr, p.e, p.format, p.nframes, p.frames, params, m.meta, m.per_frame, out}};
}
// the tail of an unpacked encode entry; its packed twin: .packed_into(), the unpacked sheet encodes: .strided_by()
RaggedOut answers(void* d_out, uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return {d_out, d_sizes, modes, q_out, value_out, stream};
}

template <class K>
int shape_body(const Make& m, const Shape& s, bool missing) {
  const std::string& who = m.who();
  const ShapeWords& w = m.family->words;
  const MadeOut& o = m.out;
  if (m.p.e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (missing || m.p.frames == nullptr || o.d_out == nullptr || o.out_frames == nullptr || o.out_format == nullptr) {
    return set_error(SJPEG_HIP_EINVAL, who + ": " + w.pointers + " == NULL");
  }
  if ((reinterpret_cast<uintptr_t>(o.d_out) & 15u) != 0) return set_error(SJPEG_HIP_EINVAL, who + ": " + w.buffer + " must be a multiple of 16");
  try {
    typename K::Plan plan;
    if (K::yuv_only) { if (int rc = yuv_format_check(who, m.p.format)) return rc; }
    const SourceLayout* const L = source_layout(m.p.format);
    if (L == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": unknown source format");
    if (m.p.nframes < 1 || m.p.nframes > 65535) return set_error(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
    if (int rc = ragged_check(who, m.p.format, source_mode(L), m.p.nframes, m.p.frames, K::esz)) return rc;
    if (int rc = K::plan(who, m.p.format, m.p.nframes, m.p.frames, s, &plan)) return rc;
    if (o.bytes < plan.bytes) {
      return set_error(SJPEG_HIP_EINVAL, who + ": " + w.bytes + " " + std::to_string(o.bytes) + " is below the " + std::to_string(plan.bytes) +
                                             " bytes the " + w.made + " take (" + w.bytes_fn + ")");
    }
    if (int rc = K::run(m.p.e, who, plan, static_cast<uint8_t*>(o.d_out), nullptr, o.stream)) return rc;
    K::frames(plan, m.p.frames, static_cast<uint8_t*>(o.d_out), o.out_frames);
    if (o.count != nullptr) *o.count = K::count(plan, m.p.nframes);
    *o.out_format = K::format(plan);
    return 0;
  } catch (...) {
    return set_error(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

// ---- the encode entries' flows
// a packed call's frames go where the placement kernel says: their out_offset is not read
void unplace(const RaggedOut& o, std::vector<sjpeg_hip_ragged_frame>* made) {
  if (o.packed) for (sjpeg_hip_ragged_frame& f : *made) f.out_offset = 0;
}

// The rest of a call whose pictures are planned (prologue done): the remaining checks -- the plan's, the yuv_mode, the
// caller's frames, the inner flow's own on the made pictures (standing at kNoMemoryYet), the metadata --, then the
// kernel into the engine's memory for made pictures and ONE inner flow over them, read as the plan's format: frame
// order, packed layout, modes, q_out, value_out, the host waits and the search counters are that flow's.
template <class K>
int planned_flow(const RaggedCall& c, const Shape& s) {
  const std::string& who = *c.who;
  try {
    const SourceLayout* const L = source_layout(c.format);
    if (L == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": unknown source format");
    typename K::Plan plan;
    if (int rc = K::plan(who, c.format, c.nframes, c.frames, s, &plan)) return rc;
    if (L->implied != 0 && c.params->yuv_mode != L->implied) {
      return set_error(SJPEG_HIP_EINVAL, who + ": yuv_mode does not match the source format" + K::mode_hint(plan));
    }
    if (int rc = ragged_check(who, c.format, source_mode(L), c.nframes, c.frames, K::esz)) return rc;
    std::vector<sjpeg_hip_ragged_frame> made = made_pictures<K>(plan, c.frames, c.nframes);
    unplace(c.out, &made);
    if (int rc = full_checks(who, K::format(plan), c.nframes, made.data(), *c.params)) return rc;
    MetaCtx ctx;
    if (c.meta != nullptr) { if (int rc = check_metadata(who, c.nframes, c.meta, c.meta_per_frame, &ctx)) return rc; }
    // ---- device work
    uint8_t* base = nullptr;
    if (int rc = K::run(c.e, who, plan, nullptr, &base, c.out.stream)) return rc;
    K::frames(plan, c.frames, base, made.data());
    unplace(c.out, &made);
    RaggedCall inner = c;
    inner.format = K::format(plan); inner.frames = made.data();
    const MetaScope scope(c.e, c.meta != nullptr ? &ctx : nullptr);
    return full_flow(inner);
  } catch (...) {
    return set_error(SJPEG_HIP_ENOMEM, who + ": out of host memory");
  }
}

// The contact sheets' flow differs: params, meta, modes, q_out and value_out count SHEETS, whose output ranges the flow
// makes itself -- sheet s at d_out + s * out_stride with capacity out_stride, or packed with what is always enough.
template <class K>
int sheet_flow(const RaggedCall& c, const Shape& s) {
  const std::string& who = *c.who;
  const RaggedOut& o = c.out;
  try {
    typename K::Plan plan;
    if (int rc = K::plan(who, c.format, c.nframes, c.frames, s, &plan)) return rc;
    const SourceLayout* const L = source_layout(c.format);
    if (L->implied != 0 && c.params->yuv_mode != L->implied) {
      return set_error(SJPEG_HIP_EINVAL, who + ": yuv_mode does not match the source format" + SheetKind::mode_hint(plan));
    }
    // (the source frames' output ranges are not read: the sheets' are the call's)
    std::vector<sjpeg_hip_ragged_frame> src(c.frames, c.frames + c.nframes);
    for (sjpeg_hip_ragged_frame& f : src) { f.out_offset = 0; f.out_capacity = 0; }
    if (int rc = ragged_check(who, c.format, source_mode(L), c.nframes, src.data(), K::esz)) return rc;
    const int ns = plan.nsheets;
    if (!o.packed && o.out_stride > UINT64_MAX / static_cast<uint64_t>(ns)) {
      return set_error(SJPEG_HIP_EINVAL, who + ": out_stride * nsheets overflows");
    }
    MetaCtx ctx;
    if (c.meta != nullptr) { if (int rc = check_metadata(who, ns, c.meta, c.meta_per_frame, &ctx)) return rc; }
    std::vector<sjpeg_hip_ragged_frame> made(static_cast<size_t>(ns));
    auto made_sheets = [&](uint8_t* base) {
      sheet_plan_frames(plan, base, made.data());
      for (int k = 0; k < ns; ++k) {
        made[k].out_offset = o.packed ? 0 : static_cast<uint64_t>(k) * o.out_stride;
        // (packed: a sheet may take what is always enough for it)
        const size_t header = 2048 + (c.meta != nullptr && !ctx.entries.empty() ? ctx.of(k).block.size() : 0);
        made[k].out_capacity = o.packed ? sjpeg_hip_frame_bound(plan.width, plan.height, SJPEG_HIP_YUV444, header) : o.out_stride;
      }
    };
    // (the inner flow's own checks on the sheets, standing at kNoMemoryYet)
    made_sheets(kNoMemoryYet);
    if (int rc = full_checks(who, plan.out_format, ns, made.data(), *c.params)) return rc;
    // ---- device work
    uint8_t* base = nullptr;
    if (int rc = K::run(c.e, who, plan, nullptr, &base, o.stream)) return rc;
    made_sheets(base);
    RaggedCall inner = c;
    inner.format = plan.out_format; inner.nframes = ns; inner.frames = made.data();
    const MetaScope scope(c.e, c.meta != nullptr ? &ctx : nullptr);
    return full_flow(inner);
  } catch (...) {
    return set_error(SJPEG_HIP_ENOMEM, who + ": out of host memory");
  }
}

// ---- what the rules ask
bool all_ones(const uint8_t* v, int nframes) {
  for (int f = 0; v != nullptr && f < nframes; ++f) if (v[f] != 1) return false;
  return true;
}
bool all_own_size(const int32_t (*sizes)[2], int nframes, const sjpeg_hip_ragged_frame* frames) {
  for (int f = 0; sizes != nullptr && f < nframes; ++f) {
    if (sizes[f][0] != frames[f].width || sizes[f][1] != frames[f].height) return false;
  }
  return true;
}
// 0 where every value is lo..hi (NULL: none to check), else the message names the first frame whose is not
int per_frame_range(const std::string& who, const uint8_t* v, int nframes, const char* what, int hi, const char* tail) {
  for (int f = 0; v != nullptr && f < nframes; ++f) {
    if (v[f] < 1 || v[f] > hi) {
      return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": " + what + " " + std::to_string(v[f]) + " is not one of 1.." +
                                             std::to_string(hi) + tail);
    }
  }
  return 0;
}
int orientations_check(const std::string& who, const uint8_t* orientations, int nframes) {
  return per_frame_range(who, orientations, nframes, "orientation", 8, " (EXIF tag 0x0112)");
}
// "nothing to do" of a per-frame array: NULL, or -- where nframes is a count: only then is the array [nframes] -- the
// family's all-identity test
template <class T, class Test>
bool nothing_to(Test all_identity, int nframes, const PerFrame<T>& a, bool one_needs_count = false) {
  const bool counted = nframes >= 1 && nframes <= 65535;
  return a.p == nullptr || (((a.per_frame == 0 && !one_needs_count) || counted) && all_identity(nframes, a.p, a.per_frame));
}
bool nothing_to_convert(int nframes, const Shape& s) { return nothing_to(yuv_colour_all_identity, nframes, s.colour, true); }
bool nothing_to_sharpen(int nframes, const Shape& s) { return nothing_to(unsharp_all_zero, nframes, s.unsharp); }
bool nothing_to_filter(int nframes, const Shape& s) { return nothing_to(pillow_filter_all_none, nframes, s.filter); }
// whether every frame's compose is an identity; a call with a canvas that the box plan refuses is not: the entry says why
bool nothing_to_compose(int format, int nframes, const Frame* frames, const Shape& s) {
  const PerFrame<sjpeg_hip_compose>& a = s.compose;
  if (a.p == nullptr) return true;
  if (a.per_frame != 0 && (nframes < 1 || nframes > 65535)) return false;      // (compose is [nframes] only where nframes is a count)
  if (compose_all_none(nframes, a.p, a.per_frame)) return true;
  // a frame with a canvas: an identity where the canvas is the made picture's size -- which the plan knows
  const int n = a.per_frame != 0 ? nframes : 1;
  for (int f = 0; f < n; ++f) if (a.p[f].nplaces != 0) return false;
  if (frames == nullptr || s.resample.p == nullptr || s.box.p == nullptr || nframes < 1 || nframes > 65535) return false;
  if (source_layout(format) == nullptr) return false;
  static const std::string quiet = "sjpeg_hip_compose_ragged_src";
  if (compose_check(quiet, nframes, a.p, a.per_frame, s.overlays.p, s.overlays.n, s.places.p, s.places.n) != 0) return false;
  try {
    ResamplePlan made;
    if (ResampleBoxKind::plan(quiet, format, nframes, frames, s, &made) != 0) return false;
    const std::vector<Frame> pictures = made_pictures<ResampleBoxKind>(made, frames, nframes);
    for (int f = 0; f < nframes; ++f) {
      const sjpeg_hip_compose& c = a.p[a.per_frame != 0 ? f : 0];
      const bool own = c.canvas_width == 0 && c.canvas_height == 0;
      if (!own && (c.canvas_width != pictures[f].width || c.canvas_height != pictures[f].height)) return false;
      if (c.mode == 0 && (c.px != 0 || c.py != 0)) return false;
    }
    return true;
  } catch (...) {
    return false;
  }
}
// a format of the other family is refused by name and pointed at the entries that take it
int unsharp_family_check(const std::string& who, int format, bool yuv) {
  const SourceLayout* const L = source_layout(format);
  if (L == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": unknown source format");
  const bool planes = L->cls == kSrcPlanes && L->planes >= 2;
  if (planes == yuv) return 0;
  if (yuv) {
    return set_error(SJPEG_HIP_EINVAL, who + ": " + source_format_name(format) + " is not a YUV-plane format (RGB-like and gray pictures are "
                                           "sharpened by sjpeg_hip_unsharp_ragged_src and sjpeg_hip_encode_ragged_unsharp_src)");
  }
  return set_error(SJPEG_HIP_EINVAL, who + ": " + source_format_name(format) + " is a YUV-plane format (decoded video is sharpened by "
                                         "sjpeg_hip_unsharp_ragged_yuv_src and sjpeg_hip_encode_ragged_yuv_unsharp_src)");
}

// ---- THE RULES, one per family, against either finisher F.  Only an encode entry passes through to the _resized_ and
// _full_meta_ calls -- a shape entry has no route of fewer arguments there: it refuses the NULL that the encode entry
// passes through on, and always makes its pictures --, so the rules of reduced, resized, flattened and yuv_resized are
// two overloads side by side.  The others are one template.  Where the recorded order of an encode entry's checks and
// its shape entry's differ, the rule says so on the line (`F::encodes`): an encode entry checks its values in front of
// its plan, a shape entry leaves them to its plan, behind its buffer's checks.

// factors NULL or all 1: exactly the _full_meta_ call on the caller's frames
int reduced_rule(Encode f, const Shape& s) {
  f.enter(kReduced);
  if (int rc = f.begin()) return rc;
  if (int rc = per_frame_range(f.who(), s.factors, f.nframes(), "factor", SJPEG_HIP_REDUCE_MAX, "")) return rc;
  if (all_ones(s.factors, f.nframes())) return full_entry(f.c);
  return f.run<ReduceKind>(s);
}
int reduced_rule(Make f, const Shape& s) {
  f.enter(kReduced);
  return f.run<ReduceKind>(s, s.factors == nullptr);
}
// sizes NULL or every size its frame's own: the _full_meta_ call again
int resized_rule(Encode f, const Shape& s) {
  f.enter(kResized);
  if (int rc = f.begin()) return rc;
  if (all_own_size(s.sizes, f.nframes(), f.frames())) return full_entry(f.c);
  return f.run<ResizeKind>(s);
}
int resized_rule(Make f, const Shape& s) {
  f.enter(kResized);
  return f.run<ResizeKind>(s, s.sizes == nullptr);
}
// flatten NULL: the oriented call.  Then orientations NULL or all 1 and no flatten: exactly the resized call on the same
// arguments (so any format at its own sizes still passes through to the _full_meta_ call).  With a flatten every frame
// goes through the kernel: the inner call never sees the alpha format.
int flattened_rule(Encode f, const Shape& s) {
  f.enter(s.flatten != nullptr ? kFlattened : kOriented);
  if (int rc = f.begin()) return rc;
  if (int rc = orientations_check(f.who(), s.orientations, f.nframes())) return rc;
  if (s.flatten == nullptr && all_ones(s.orientations, f.nframes())) return resized_rule(f, s);
  return f.run<ResizeKind>(s);
}
int flattened_rule(Make f, const Shape& s) {
  f.enter(s.flatten != nullptr ? kFlattened : kOriented);
  return f.run<ResizeKind>(s);
}
// every size the frame's own and every orientation 1 (or both NULL): the _full_meta_ call on the caller's planes
int yuv_resized_rule(Encode f, const Shape& s) {
  f.enter(kYuvResized);
  if (int rc = f.begin(false, nullptr, true)) return rc;
  if (int rc = orientations_check(f.who(), s.orientations, f.nframes())) return rc;
  if (all_ones(s.orientations, f.nframes()) && all_own_size(s.sizes, f.nframes(), f.frames())) return full_entry(f.c);
  return f.run<YuvResizeKind>(s);
}
int yuv_resized_rule(Make f, const Shape& s) {
  f.enter(kYuvResized);
  return f.run<YuvResizeKind>(s);
}
// no pass-through; flatten NULL: the sheet entry under its own name
template <class F>
int sheet_rule(F f, const Shape& s) {
  f.enter(s.flatten != nullptr ? kSheetFlat : kSheet);
  if (int rc = f.begin(true, s.sheet)) return rc;
  return f.template run<SheetKind>(s);
}

// Video colour.  colour NULL or the identity for every frame: exactly the yuv_resized call on the same arguments.
// Otherwise every frame goes through the resize kernel, at its own size and orientation 1 too: the colour launch works
// in place, and the caller's planes are not its to write.
template <class F>
int yuv_converted_rule(F f, const Shape& s) {
  f.enter(kYuvConverted);
  // (not the shape entry: it has nothing to say before it knows whose name the call goes by)
  if constexpr (F::encodes) { if (int rc = f.begin(false, nullptr, true)) return rc; }
  if (nothing_to_convert(f.nframes(), s)) return yuv_resized_rule(f, s);
  if constexpr (F::encodes) { if (int rc = orientations_check(f.who(), s.orientations, f.nframes())) return rc; }
  return f.template run<YuvColourKind>(s);
}
// ... the sheet call, for the YUV-plane formats
template <class F>
int sheet_colour_rule(F f, const Shape& s) {
  f.enter(kSheetColour);
  if (int rc = f.begin(true, s.sheet, true)) return rc;
  // (the shape entry: the format by name in front of the route, as the prologue has it for the encode entries)
  if constexpr (!F::encodes) { if (int rc = yuv_format_check(f.who(), f.format())) return rc; }
  if (nothing_to_convert(f.nframes(), s)) return sheet_rule(f, s);
  return f.template run<SheetColourKind>(s);
}

// 16-bit samples: no pass-through -- the inner flow cannot read words, so every frame goes through the kernel, at its
// own size and orientation 1 too.  colour NULL: none.
template <class F>
int yuv16_rule(F f, const Shape& s) {
  f.enter(kYuv16);
  if (int rc = f.begin(false, nullptr, true)) return rc;
  if (int rc = yuv_depth_check(f.who(), s.depth)) return rc;
  if constexpr (F::encodes) { if (int rc = orientations_check(f.who(), s.orientations, f.nframes())) return rc; }
  return f.template run<YuvDeepKind>(s);
}
template <class F>
int sheet_yuv16_rule(F f, const Shape& s) {
  f.enter(kSheetYuv16);
  if (int rc = f.begin(true, s.sheet, true)) return rc;
  if constexpr (!F::encodes) { if (int rc = yuv_format_check(f.who(), f.format())) return rc; }      // (as sheet_colour_rule)
  if (int rc = yuv_depth_check(f.who(), s.depth)) return rc;
  return f.template run<SheetDeepKind>(s);
}

// Linear light.  light == SJPEG_HIP_LIGHT_CODED: exactly the flattened call (which hands on to the oriented one without
// a flatten) on the same arguments.  Otherwise no pass-through: every frame goes through the kernel, at its own size
// and orientation 1 too -- a copy, because the inverse is exact.
template <class F>
int linear_rule(F f, const Shape& s) {
  if (s.light == SJPEG_HIP_LIGHT_CODED) return flattened_rule(f, s);
  f.enter(kLinear);
  if (int rc = f.begin()) return rc;
  if (int rc = light_check(f.who(), s.light, f.format())) return rc;
  if constexpr (F::encodes) { if (int rc = orientations_check(f.who(), s.orientations, f.nframes())) return rc; }
  return f.template run<LinearKind>(s);
}
template <class F>
int sheet_linear_rule(F f, const Shape& s) {
  if (s.light == SJPEG_HIP_LIGHT_CODED) return sheet_rule(f, s);
  f.enter(kSheetLinear);
  if (int rc = f.begin(true, s.sheet)) return rc;
  if (int rc = light_check(f.who(), s.light, f.format())) return rc;
  return f.template run<SheetLinearKind>(s);
}

// The unsharp mask.  unsharp NULL or amount 0 for every frame: exactly the linear call (which hands on to the flattened
// one in coded light) or, for the YUV-plane formats, the yuv16 call or without a depth the yuv_converted one, on the
// same arguments.  Otherwise no pass-through: every frame goes through the resize kernel, at its own size and
// orientation 1 too -- the unsharp launch reads the made pictures, whatever the source format.
template <class F>
int unsharp_rule(F f, const Shape& s) {
  if (nothing_to_sharpen(f.nframes(), s)) return linear_rule(f, s);
  f.enter(kUnsharp);
  if (int rc = f.begin()) return rc;
  if (int rc = unsharp_family_check(f.who(), f.format(), false)) return rc;
  if (int rc = light_check(f.who(), s.light, f.format())) return rc;
  if constexpr (F::encodes) {
    if (int rc = unsharp_check(f.who(), f.nframes(), s.unsharp.p, s.unsharp.per_frame)) return rc;
    if (int rc = orientations_check(f.who(), s.orientations, f.nframes())) return rc;
  }
  return f.template run<UnsharpKind<LinearKind>>(s);
}
template <class F>
int yuv_unsharp_rule(F f, const Shape& s) {
  if (nothing_to_sharpen(f.nframes(), s)) return s.depth == nullptr ? yuv_converted_rule(f, s) : yuv16_rule(f, s);
  f.enter(kYuvUnsharp);
  if (int rc = f.begin()) return rc;
  if (int rc = unsharp_family_check(f.who(), f.format(), true)) return rc;
  if (s.depth != nullptr) { if (int rc = yuv_depth_check(f.who(), s.depth)) return rc; }
  if constexpr (F::encodes) {
    if (int rc = unsharp_check(f.who(), f.nframes(), s.unsharp.p, s.unsharp.per_frame)) return rc;
    if (int rc = orientations_check(f.who(), s.orientations, f.nframes())) return rc;
  }
  return s.depth == nullptr ? f.template run<UnsharpKind<YuvColourKind>>(s) : f.template run<UnsharpKind<YuvDeepKind>>(s);
}

// Resampling with Pillow's filters.  No pass-through: every frame goes through the resample kernel, at its own size too
// (a copy: the identity tables).  The resample families' mandatory pointers, resample and with_box box -- between them
// an encode entry checks resample's values, and behind them the later stages' (`values`) and the orientations:
template <class F, class Values>
int resample_checks(const F& f, const Shape& s, bool with_box, Values values) {
  if (s.resample.p == nullptr) return set_error(SJPEG_HIP_EINVAL, f.who() + ": resample == NULL");
  if constexpr (F::encodes) { if (int rc = resample_check(f.who(), f.nframes(), s.resample.p, s.resample.per_frame)) return rc; }
  if (with_box && s.box.p == nullptr) return set_error(SJPEG_HIP_EINVAL, f.who() + ": box == NULL");
  if constexpr (F::encodes) {
    if (int rc = values()) return rc;
    if (int rc = orientations_check(f.who(), s.orientations, f.nframes())) return rc;
  }
  return 0;
}
// unsharp NULL or amount 0 for every frame: the made pictures are the call's; otherwise the unsharp launch runs behind
// the resample launch, unchanged.
template <class F>
int resampled_rule(F f, const Shape& s) {
  f.enter(kResampled);
  if (int rc = f.begin()) return rc;
  if (int rc = resample_checks(f, s, false, [] { return 0; })) return rc;
  return nothing_to_sharpen(f.nframes(), s) ? f.template run<ResampleKind>(s) : f.template run<UnsharpKind<ResampleKind>>(s);
}
// ... from a source box and behind a reduce: the same, the plan the box kind's
template <class F>
int resampled_box_rule(F f, const Shape& s) {
  f.enter(kResampledBox);
  if (int rc = f.begin()) return rc;
  if (int rc = resample_checks(f, s, true, [] { return 0; })) return rc;
  return nothing_to_sharpen(f.nframes(), s) ? f.template run<ResampleBoxKind>(s) : f.template run<UnsharpKind<ResampleBoxKind>>(s);
}
// Pillow's filters behind the box entries.  filter NULL or kind 0 for every frame: exactly the resampled_box call
// without unsharp on the same arguments, under its name.  Otherwise the two filter launches run behind the resample
// launch over every frame, those of kind 0 copied.
template <class F>
int filtered_rule(F f, const Shape& s) {
  if (nothing_to_filter(f.nframes(), s)) return resampled_box_rule(f, s);
  f.enter(kFiltered);
  if (int rc = f.begin()) return rc;
  if (int rc = resample_checks(f, s, true, [&] { return pillow_filter_check(f.who(), f.nframes(), s.filter.p, s.filter.per_frame); })) return rc;
  return f.template run<FilterKind<ResampleBoxKind>>(s);
}
// The compose stage behind the filtered entries.  compose NULL, or every frame an identity -- a canvas of 0 x 0, or of
// the made picture's own size with the picture at (0, 0), and no place --: exactly the filtered call on the same
// arguments, under its name.  Otherwise one compose launch runs behind the launches that made the pictures; a call
// none of whose frames has a filter runs no filter launch.
template <class F>
int composed_rule(F f, const Shape& s) {
  if (nothing_to_compose(f.format(), f.nframes(), f.frames(), s)) return filtered_rule(f, s);
  f.enter(kComposed);
  if (int rc = f.begin()) return rc;
  const auto values = [&] {
    if (int rc = pillow_filter_check(f.who(), f.nframes(), s.filter.p, s.filter.per_frame)) return rc;
    return compose_check(f.who(), f.nframes(), s.compose.p, s.compose.per_frame, s.overlays.p, s.overlays.n, s.places.p, s.places.n);
  };
  if (int rc = resample_checks(f, s, true, values)) return rc;
  if (nothing_to_filter(f.nframes(), s)) return f.template run<ComposeKind<ResampleBoxKind>>(s);
  return f.template run<ComposeKind<FilterKind<ResampleBoxKind>>>(s);
}

}  // namespace

extern "C" {

// ---- pictures reduced by their factors: thumbnails and pyramid levels
int sjpeg_hip_reduce_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const uint8_t* factors,
                                void* d_reduced, size_t reduced_bytes, sjpeg_hip_ragged_frame* reduced_frames, int* reduced_format, void* stream) {
  Shape s; s.factors = factors;
  return reduced_rule(Make{{e, format, nframes, frames}, pictures_into(d_reduced, reduced_bytes, reduced_frames, reduced_format, stream)}, s);
}

int sjpeg_hip_encode_ragged_reduced_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                        const sjpeg_hip_ragged_params* params, const uint8_t* factors, const sjpeg_hip_metadata* meta,
                                        int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                        void* stream) {
  Shape s; s.factors = factors;
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream);
  return reduced_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_reduced_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                               const sjpeg_hip_ragged_params* params, const uint8_t* factors, const sjpeg_hip_metadata* meta,
                                               int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes,
                                               int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.factors = factors;
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return reduced_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

// ---- ... resized to their sizes: thumbnails that fit a box
int sjpeg_hip_resize_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                                void* d_resized, size_t resized_bytes, sjpeg_hip_ragged_frame* resized_frames, int* resized_format, void* stream) {
  Shape s; s.sizes = sizes;
  return resized_rule(Make{{e, format, nframes, frames}, pictures_into(d_resized, resized_bytes, resized_frames, resized_format, stream)}, s);
}

int sjpeg_hip_encode_ragged_resized_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                        const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const sjpeg_hip_metadata* meta,
                                        int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                        void* stream) {
  Shape s; s.sizes = sizes;
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream);
  return resized_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_resized_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                               const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const sjpeg_hip_metadata* meta,
                                               int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes,
                                               int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.sizes = sizes;
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return resized_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

// ---- ... and turned upright by their EXIF orientations in the same ONE launch (orient_math.h): the kernel stores every
// tile where it lands in the upright picture
int sjpeg_hip_orient_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                                const uint8_t* orientations, void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* out_frames, int* out_format,
                                void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations;
  return flattened_rule(Make{{e, format, nframes, frames}, pictures_into(d_out, out_bytes, out_frames, out_format, stream)}, s);
}

int sjpeg_hip_encode_ragged_oriented_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                         const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                         const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes, float* q_out,
                                         float* value_out, void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations;
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream);
  return flattened_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_oriented_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                                const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed, size_t packed_capacity,
                                                uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations;
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return flattened_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

// ---- ... and flattened over a background as they are staged (flatten_math.h), still ONE launch: RGBA pictures.  The
// shape entry wants its flatten (`flatten` goes into the plan, whose checks of it come with its others).
int sjpeg_hip_flatten_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_flatten* flatten,
                                 const int32_t (*sizes)[2], const uint8_t* orientations, void* d_out, size_t out_bytes,
                                 sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations;
  Make f = Make{{e, format, nframes, frames}, pictures_into(d_out, out_bytes, out_frames, out_format, stream)};
  f.enter(kFlattened);
  if (int rc = f.begin()) return rc;
  if (flatten == nullptr) return set_error(SJPEG_HIP_EINVAL, f.who() + ": flatten == NULL");      // (this entry wants its flatten)
  return flattened_rule(f, s);
}

int sjpeg_hip_encode_ragged_flattened_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                          const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                          const uint8_t* orientations, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out,
                                          uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations;
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream);
  return flattened_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_flattened_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                 const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                                 const uint8_t* orientations, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed,
                                                 size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out,
                                                 float* value_out, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations;
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return flattened_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

// ---- ... and decoded video: NV12, NV21 and planar YUV resized and turned plane by plane, every plane a picture of its
// own, still ONE launch; the inner flow codes the planes as planar 4:2:0 or 4:4:4
int sjpeg_hip_resize_ragged_yuv_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                                    const uint8_t* orientations, void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* out_frames, int* out_format,
                                    void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations;
  return yuv_resized_rule(Make{{e, format, nframes, frames}, pictures_into(d_out, out_bytes, out_frames, out_format, stream)}, s);
}

int sjpeg_hip_encode_ragged_yuv_resized_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                            const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                            const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes,
                                            float* q_out, float* value_out, void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations;
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream);
  return yuv_resized_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_yuv_resized_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                   const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                                   const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed, size_t packed_capacity,
                                                   uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations;
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return yuv_resized_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

// ---- ... and contact sheets: the batch resized, turned and placed into grid pictures; one set of entries for both
// families of formats
int sjpeg_hip_sheet_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_sheet* sheet,
                               const int32_t (*sizes)[2], const uint8_t* orientations, void* d_out, size_t out_bytes,
                               sjpeg_hip_ragged_frame* sheet_frames, int* nsheets, int* out_format, void* stream) {
  Shape s; s.sheet = sheet; s.sizes = sizes; s.orientations = orientations;
  return sheet_rule(Make{{e, format, nframes, frames}, {d_out, out_bytes, sheet_frames, nsheets, out_format, stream}}, s);
}

int sjpeg_hip_sheet_ragged_flat_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_sheet* sheet,
                                    const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations, void* d_out,
                                    size_t out_bytes, sjpeg_hip_ragged_frame* sheet_frames, int* nsheets, int* out_format, void* stream) {
  Shape s; s.sheet = sheet; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations;
  Make f = Make{{e, format, nframes, frames}, {d_out, out_bytes, sheet_frames, nsheets, out_format, stream}};
  f.enter(kSheetFlat);
  if (int rc = f.begin()) return rc;
  if (flatten == nullptr) return set_error(SJPEG_HIP_EINVAL, f.who() + ": flatten == NULL");      // (this entry wants its flatten)
  return sheet_rule(f, s);
}

int sjpeg_hip_encode_ragged_sheet_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                      const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2],
                                      const uint8_t* orientations, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, size_t out_stride,
                                      uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.sheet = sheet; s.sizes = sizes; s.orientations = orientations;
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream).strided_by(out_stride);
  return sheet_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_sheet_flat_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                           const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet, const sjpeg_hip_flatten* flatten,
                                           const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_metadata* meta, int meta_per_frame,
                                           void* d_out, size_t out_stride, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                           void* stream) {
  Shape s; s.sheet = sheet; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations;
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream).strided_by(out_stride);
  return sheet_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_sheet_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                             const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2],
                                             const uint8_t* orientations, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed,
                                             size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out,
                                             float* value_out, void* stream) {
  Shape s; s.sheet = sheet; s.sizes = sizes; s.orientations = orientations;
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return sheet_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_sheet_flat_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                  const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                                  const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations,
                                                  const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed, size_t packed_capacity,
                                                  uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.sheet = sheet; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations;
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return sheet_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

// ---- ... and video colour: the made planes, or the thumbnails' rectangles of a sheet, converted to JFIF's full-range
// BT.601 by ONE more launch behind the resize launch (yuv_colour.hip)
int sjpeg_hip_convert_ragged_yuv_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                                     const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour, int colour_per_frame, void* d_out,
                                     size_t out_bytes, sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame};
  return yuv_converted_rule(Make{{e, format, nframes, frames}, pictures_into(d_out, out_bytes, out_frames, out_format, stream)}, s);
}

int sjpeg_hip_encode_ragged_yuv_converted_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                              const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                              const sjpeg_hip_yuv_colour* colour, int colour_per_frame, const sjpeg_hip_metadata* meta,
                                              int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                              void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame};
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream);
  return yuv_converted_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_yuv_converted_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                     const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                                     const sjpeg_hip_yuv_colour* colour, int colour_per_frame, const sjpeg_hip_metadata* meta,
                                                     int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets,
                                                     uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame};
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return yuv_converted_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_sheet_ragged_yuv_colour_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                          const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2], const uint8_t* orientations,
                                          const sjpeg_hip_yuv_colour* colour, int colour_per_frame, void* d_out, size_t out_bytes,
                                          sjpeg_hip_ragged_frame* sheet_frames, int* nsheets, int* out_format, void* stream) {
  Shape s; s.sheet = sheet; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame};
  return sheet_colour_rule(Make{{e, format, nframes, frames}, {d_out, out_bytes, sheet_frames, nsheets, out_format, stream}}, s);
}

int sjpeg_hip_encode_ragged_sheet_yuv_colour_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                 const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2],
                                                 const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                                                 const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, size_t out_stride,
                                                 uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.sheet = sheet; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame};
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream).strided_by(out_stride);
  return sheet_colour_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_sheet_yuv_colour_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                        const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                                        const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour,
                                                        int colour_per_frame, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed,
                                                        size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out,
                                                        float* value_out, void* stream) {
  Shape s; s.sheet = sheet; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame};
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return sheet_colour_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

// ---- ... and 10-bit video: the YUV-plane formats with 16-bit samples (P010 and its kin, yuv420p10le / 12le) through the
// kernel's deep instantiations; each entry its colour counterpart plus the depth
int sjpeg_hip_convert_ragged_yuv16_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                                       const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                                       const sjpeg_hip_yuv_depth* depth, void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* out_frames,
                                       int* out_format, void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame}; s.depth = depth;
  return yuv16_rule(Make{{e, format, nframes, frames}, pictures_into(d_out, out_bytes, out_frames, out_format, stream)}, s);
}

int sjpeg_hip_encode_ragged_yuv16_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                      const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                      const sjpeg_hip_yuv_colour* colour, int colour_per_frame, const sjpeg_hip_yuv_depth* depth,
                                      const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes, float* q_out,
                                      float* value_out, void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame}; s.depth = depth;
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream);
  return yuv16_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_yuv16_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                             const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                             const sjpeg_hip_yuv_colour* colour, int colour_per_frame, const sjpeg_hip_yuv_depth* depth,
                                             const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed, size_t packed_capacity,
                                             uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame}; s.depth = depth;
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return yuv16_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_sheet_ragged_yuv16_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_sheet* sheet,
                                     const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                                     const sjpeg_hip_yuv_depth* depth, void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* sheet_frames,
                                     int* nsheets, int* out_format, void* stream) {
  Shape s; s.sheet = sheet; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame}; s.depth = depth;
  return sheet_yuv16_rule(Make{{e, format, nframes, frames}, {d_out, out_bytes, sheet_frames, nsheets, out_format, stream}}, s);
}

int sjpeg_hip_encode_ragged_sheet_yuv16_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                            const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2],
                                            const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                                            const sjpeg_hip_yuv_depth* depth, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out,
                                            size_t out_stride, uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.sheet = sheet; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame}; s.depth = depth;
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream).strided_by(out_stride);
  return sheet_yuv16_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_sheet_yuv16_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                   const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2],
                                                   const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                                                   const sjpeg_hip_yuv_depth* depth, const sjpeg_hip_metadata* meta, int meta_per_frame,
                                                   void* d_packed, size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes, int* modes,
                                                   float* q_out, float* value_out, void* stream) {
  Shape s; s.sheet = sheet; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame}; s.depth = depth;
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return sheet_yuv16_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

// ---- ... and the resize in linear light: the flattened and sheet entries plus `light` (light_math.h), through the
// kernel's linear instantiations; flatten may be NULL
int sjpeg_hip_linear_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_flatten* flatten,
                                int light, const int32_t (*sizes)[2], const uint8_t* orientations, void* d_out, size_t out_bytes,
                                sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  Shape s; s.flatten = flatten; s.light = light; s.sizes = sizes; s.orientations = orientations;
  return linear_rule(Make{{e, format, nframes, frames}, pictures_into(d_out, out_bytes, out_frames, out_format, stream)}, s);
}

int sjpeg_hip_encode_ragged_linear_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                       const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, int light, const int32_t (*sizes)[2],
                                       const uint8_t* orientations, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out,
                                       uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.flatten = flatten; s.light = light; s.sizes = sizes; s.orientations = orientations;
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream);
  return linear_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_linear_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                              const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, int light,
                                              const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_metadata* meta,
                                              int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes,
                                              int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.flatten = flatten; s.light = light; s.sizes = sizes; s.orientations = orientations;
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return linear_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_sheet_ragged_linear_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                      const sjpeg_hip_sheet* sheet, const sjpeg_hip_flatten* flatten, int light, const int32_t (*sizes)[2],
                                      const uint8_t* orientations, void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* sheet_frames, int* nsheets,
                                      int* out_format, void* stream) {
  Shape s; s.sheet = sheet; s.flatten = flatten; s.light = light; s.sizes = sizes; s.orientations = orientations;
  return sheet_linear_rule(Make{{e, format, nframes, frames}, {d_out, out_bytes, sheet_frames, nsheets, out_format, stream}}, s);
}

int sjpeg_hip_encode_ragged_sheet_linear_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                             const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet, const sjpeg_hip_flatten* flatten,
                                             int light, const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_metadata* meta,
                                             int meta_per_frame, void* d_out, size_t out_stride, uint64_t* d_sizes, int* modes, float* q_out,
                                             float* value_out, void* stream) {
  Shape s; s.sheet = sheet; s.flatten = flatten; s.light = light; s.sizes = sizes; s.orientations = orientations;
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream).strided_by(out_stride);
  return sheet_linear_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_sheet_linear_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                    const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                                    const sjpeg_hip_flatten* flatten, int light, const int32_t (*sizes)[2],
                                                    const uint8_t* orientations, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed,
                                                    size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out,
                                                    float* value_out, void* stream) {
  Shape s; s.sheet = sheet; s.flatten = flatten; s.light = light; s.sizes = sizes; s.orientations = orientations;
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return sheet_linear_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

// ---- ... and the unsharp mask behind any of it: the linear entries and the yuv16 entries plus `unsharp`; ONE more
// launch over the made pictures (unsharp.hip), out of place
int sjpeg_hip_unsharp_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_flatten* flatten,
                                 int light, const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_unsharp* unsharp,
                                 int unsharp_per_frame, void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* out_frames, int* out_format,
                                 void* stream) {
  Shape s; s.flatten = flatten; s.light = light; s.sizes = sizes; s.orientations = orientations; s.unsharp = {unsharp, unsharp_per_frame};
  return unsharp_rule(Make{{e, format, nframes, frames}, pictures_into(d_out, out_bytes, out_frames, out_format, stream)}, s);
}

int sjpeg_hip_encode_ragged_unsharp_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                        const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, int light, const int32_t (*sizes)[2],
                                        const uint8_t* orientations, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame,
                                        const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes, float* q_out,
                                        float* value_out, void* stream) {
  Shape s; s.flatten = flatten; s.light = light; s.sizes = sizes; s.orientations = orientations; s.unsharp = {unsharp, unsharp_per_frame};
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream);
  return unsharp_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_unsharp_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                               const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, int light,
                                               const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_unsharp* unsharp,
                                               int unsharp_per_frame, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed,
                                               size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out,
                                               float* value_out, void* stream) {
  Shape s; s.flatten = flatten; s.light = light; s.sizes = sizes; s.orientations = orientations; s.unsharp = {unsharp, unsharp_per_frame};
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return unsharp_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_unsharp_ragged_yuv_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                                     const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                                     const sjpeg_hip_yuv_depth* depth, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, void* d_out,
                                     size_t out_bytes, sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame}; s.depth = depth;
  s.unsharp = {unsharp, unsharp_per_frame};
  return yuv_unsharp_rule(Make{{e, format, nframes, frames}, pictures_into(d_out, out_bytes, out_frames, out_format, stream)}, s);
}

int sjpeg_hip_encode_ragged_yuv_unsharp_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                            const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                            const sjpeg_hip_yuv_colour* colour, int colour_per_frame, const sjpeg_hip_yuv_depth* depth,
                                            const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, const sjpeg_hip_metadata* meta,
                                            int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                            void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame}; s.depth = depth;
  s.unsharp = {unsharp, unsharp_per_frame};
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream);
  return yuv_unsharp_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_yuv_unsharp_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                   const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                                   const sjpeg_hip_yuv_colour* colour, int colour_per_frame, const sjpeg_hip_yuv_depth* depth,
                                                   const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, const sjpeg_hip_metadata* meta,
                                                   int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes,
                                                   int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.sizes = sizes; s.orientations = orientations; s.colour = {colour, colour_per_frame}; s.depth = depth;
  s.unsharp = {unsharp, unsharp_per_frame};
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return yuv_unsharp_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

// ---- ... and resampling with Pillow's filters: box, bilinear, Hamming, bicubic and Lanczos windows, enlarging too; ONE
// launch of a kernel of its own (resample.hip), optionally the unsharp launch behind it
int sjpeg_hip_resample_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                  const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations,
                                  const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame,
                                  void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations; s.resample = {resample, resample_per_frame};
  s.unsharp = {unsharp, unsharp_per_frame};
  return resampled_rule(Make{{e, format, nframes, frames}, pictures_into(d_out, out_bytes, out_frames, out_format, stream)}, s);
}

int sjpeg_hip_encode_ragged_resampled_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                          const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                          const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame,
                                          const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, const sjpeg_hip_metadata* meta, int meta_per_frame,
                                          void* d_out, uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations; s.resample = {resample, resample_per_frame};
  s.unsharp = {unsharp, unsharp_per_frame};
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream);
  return resampled_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_resampled_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                 const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                                 const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame,
                                                 const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, const sjpeg_hip_metadata* meta,
                                                 int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes,
                                                 int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations; s.resample = {resample, resample_per_frame};
  s.unsharp = {unsharp, unsharp_per_frame};
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return resampled_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

// ---- ... from a source box and behind a reduce: Image.thumbnail and ImageOps.fit
int sjpeg_hip_resample_box_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                      const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations,
                                      const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_resample_box* box,
                                      int box_per_frame, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, void* d_out, size_t out_bytes,
                                      sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations; s.resample = {resample, resample_per_frame};
  s.box = {box, box_per_frame}; s.unsharp = {unsharp, unsharp_per_frame};
  return resampled_box_rule(Make{{e, format, nframes, frames}, pictures_into(d_out, out_bytes, out_frames, out_format, stream)}, s);
}

int sjpeg_hip_encode_ragged_resampled_box_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                              const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                              const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame,
                                              const sjpeg_hip_resample_box* box, int box_per_frame, const sjpeg_hip_unsharp* unsharp,
                                              int unsharp_per_frame, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out,
                                              uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations; s.resample = {resample, resample_per_frame};
  s.box = {box, box_per_frame}; s.unsharp = {unsharp, unsharp_per_frame};
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream);
  return resampled_box_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_resampled_box_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                     const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten,
                                                     const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_resample* resample,
                                                     int resample_per_frame, const sjpeg_hip_resample_box* box, int box_per_frame,
                                                     const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, const sjpeg_hip_metadata* meta,
                                                     int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets,
                                                     uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations; s.resample = {resample, resample_per_frame};
  s.box = {box, box_per_frame}; s.unsharp = {unsharp, unsharp_per_frame};
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return resampled_box_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

// ---- ... and filtered by Pillow's BoxBlur, GaussianBlur or UnsharpMask behind it: two launches (pillow_filter.hip)
int sjpeg_hip_filter_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_flatten* flatten,
                                const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame,
                                const sjpeg_hip_resample_box* box, int box_per_frame, const sjpeg_hip_pillow_filter* filter, int filter_per_frame,
                                void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations; s.resample = {resample, resample_per_frame};
  s.box = {box, box_per_frame}; s.filter = {filter, filter_per_frame};
  return filtered_rule(Make{{e, format, nframes, frames}, pictures_into(d_out, out_bytes, out_frames, out_format, stream)}, s);
}

int sjpeg_hip_encode_ragged_filtered_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                         const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                         const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame,
                                         const sjpeg_hip_resample_box* box, int box_per_frame, const sjpeg_hip_pillow_filter* filter,
                                         int filter_per_frame, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, uint64_t* d_sizes,
                                         int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations; s.resample = {resample, resample_per_frame};
  s.box = {box, box_per_frame}; s.filter = {filter, filter_per_frame};
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream);
  return filtered_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_filtered_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                                const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame,
                                                const sjpeg_hip_resample_box* box, int box_per_frame, const sjpeg_hip_pillow_filter* filter,
                                                int filter_per_frame, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed,
                                                size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out,
                                                float* value_out, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations; s.resample = {resample, resample_per_frame};
  s.box = {box, box_per_frame}; s.filter = {filter, filter_per_frame};
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return filtered_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

// ---- ... and composed behind that: a canvas and overlays by one launch (compose.hip)
size_t sjpeg_hip_compose_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                                      const uint8_t* orientations, const sjpeg_hip_resample_box* box, int box_per_frame,
                                      const sjpeg_hip_compose* compose, int compose_per_frame) {
  if (frames == nullptr || box == nullptr || nframes < 1 || nframes > 65535) return 0;
  try {
    // (the layout depends on neither the filter nor the overlays: the places are counted, not read)
    const sjpeg_hip_resample filter = {SJPEG_HIP_RESAMPLE_BOX, {0, 0, 0}};
    std::vector<sjpeg_hip_compose> bare;
    if (compose != nullptr) {
      bare.assign(compose, compose + (compose_per_frame != 0 ? nframes : 1));
      for (sjpeg_hip_compose& c : bare) {
        if (c.nplaces < 0 || c.nplaces > kComposePlacesMax || c.first_place < 0) return 0;
        c.first_place = 0; c.nplaces = 0;
      }
    }
    Shape s;
    s.sizes = sizes; s.orientations = orientations; s.resample = {&filter, 0}; s.box = {box, box_per_frame};
    if (compose != nullptr) s.compose = {bare.data(), compose_per_frame};
    ComposeKind<ResampleBoxKind>::Plan plan;
    if (ComposeKind<ResampleBoxKind>::plan("sjpeg_hip_compose_ragged_bytes", format, nframes, frames, s, &plan) != 0) return 0;
    return plan.bytes;
  } catch (...) {
    return 0;
  }
}

int sjpeg_hip_compose_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_flatten* flatten,
                                 const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame,
                                 const sjpeg_hip_resample_box* box, int box_per_frame, const sjpeg_hip_pillow_filter* filter, int filter_per_frame,
                                 const sjpeg_hip_compose* compose, int compose_per_frame, const sjpeg_hip_overlay* overlays, int noverlays,
                                 const sjpeg_hip_overlay_place* places, int nplaces, void* d_out, size_t out_bytes,
                                 sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations; s.resample = {resample, resample_per_frame};
  s.box = {box, box_per_frame}; s.filter = {filter, filter_per_frame}; s.compose = {compose, compose_per_frame};
  s.overlays = {overlays, noverlays}; s.places = {places, nplaces};
  return composed_rule(Make{{e, format, nframes, frames}, pictures_into(d_out, out_bytes, out_frames, out_format, stream)}, s);
}

int sjpeg_hip_encode_ragged_composed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                         const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                         const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame,
                                         const sjpeg_hip_resample_box* box, int box_per_frame, const sjpeg_hip_pillow_filter* filter,
                                         int filter_per_frame, const sjpeg_hip_compose* compose, int compose_per_frame,
                                         const sjpeg_hip_overlay* overlays, int noverlays, const sjpeg_hip_overlay_place* places, int nplaces,
                                         const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes, float* q_out,
                                         float* value_out, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations; s.resample = {resample, resample_per_frame};
  s.box = {box, box_per_frame}; s.filter = {filter, filter_per_frame}; s.compose = {compose, compose_per_frame};
  s.overlays = {overlays, noverlays}; s.places = {places, nplaces};
  const RaggedOut out = answers(d_out, d_sizes, modes, q_out, value_out, stream);
  return composed_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

int sjpeg_hip_encode_ragged_composed_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                                const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame,
                                                const sjpeg_hip_resample_box* box, int box_per_frame, const sjpeg_hip_pillow_filter* filter,
                                                int filter_per_frame, const sjpeg_hip_compose* compose, int compose_per_frame,
                                                const sjpeg_hip_overlay* overlays, int noverlays, const sjpeg_hip_overlay_place* places, int nplaces,
                                                const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed, size_t packed_capacity,
                                                uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  Shape s; s.flatten = flatten; s.sizes = sizes; s.orientations = orientations; s.resample = {resample, resample_per_frame};
  s.box = {box, box_per_frame}; s.filter = {filter, filter_per_frame}; s.compose = {compose, compose_per_frame};
  s.overlays = {overlays, noverlays}; s.places = {places, nplaces};
  const RaggedOut out = answers(d_packed, d_sizes, modes, q_out, value_out, stream).packed_into(packed_capacity, d_offsets);
  return composed_rule(encode({e, format, nframes, frames}, params, {meta, meta_per_frame}, out), s);
}

}  // extern "C"
