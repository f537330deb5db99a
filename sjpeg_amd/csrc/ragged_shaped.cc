// ragged_shaped.cc -- the ragged entries on pictures that are SHAPED inside the call: reduced by a factor (reduce.hip),
// resized to a size, turned upright by an EXIF orientation and flattened over a background (resize.hip), the same for
// the YUV-plane formats (yuv_resize_plan.cc), their samples bytes or 16-bit words, and placed into contact sheets
// (sheet_plan.cc), sharpened by the unsharp mask behind any of it but a sheet (unsharp_plan.cc, unsharp.hip), and
// resampled with Pillow's filters, enlarging too (resample_plan.cc, resample.hip), and filtered by Pillow's BoxBlur,
// GaussianBlur or UnsharpMask behind that (pillow_filter_plan.cc, pillow_filter.hip), and composed behind that: onto a
// canvas, under overlays (compose_plan.cc, compose.hip).  Per
// family a shape entry -- the made pictures into the caller's buffer -- and an encode entry with
// its packed twin: the pictures into the engine's memory and ONE _full_ call (ragged_full.cc) over them.  Host code only.
//
// Every entry fills a call description (ragged_aux.h: RaggedCall, RaggedOut) and names a plan KIND below; the bodies
// -- shape_body, planned_flow, sheet_flow -- are written once against those.  A route that needs no kernel (factors all
// 1, sizes the frames' own, orientations all 1, no flatten) renames the call and hands the same description to the entry
// of fewer arguments: the messages then carry that entry's name.  Every check comes before the engine is touched; their
// order and texts are pinned by tests/golden/c_messages.json.  DESIGN.md, "The C layer's call description".
#include <stdint.h>

#include <string>
#include <vector>

#include "ragged_aux.h"
#include "sjpeg_hip.h"

namespace {

using namespace sjpeg_internal;

// what an entry asks for beyond its frames (NULL: not that), in this order
struct Shape {
  const uint8_t* factors = nullptr;
  const int32_t (*sizes)[2] = nullptr;
  const uint8_t* orientations = nullptr;
  const sjpeg_hip_flatten* flatten = nullptr;
  const sjpeg_hip_sheet* sheet = nullptr;
  const sjpeg_hip_yuv_colour* colour = nullptr;
  int colour_per_frame = 0;
  const sjpeg_hip_yuv_depth* depth = nullptr;
  int light = SJPEG_HIP_LIGHT_CODED;
  const sjpeg_hip_unsharp* unsharp = nullptr;
  int unsharp_per_frame = 0;
  const sjpeg_hip_resample* resample = nullptr;
  int resample_per_frame = 0;
  const sjpeg_hip_resample_box* box = nullptr;
  int box_per_frame = 0;
  const sjpeg_hip_pillow_filter* filter = nullptr;
  int filter_per_frame = 0;
  const sjpeg_hip_compose* compose = nullptr;
  int compose_per_frame = 0;
  const sjpeg_hip_overlay* overlays = nullptr;
  int noverlays = 0;
  const sjpeg_hip_overlay_place* places = nullptr;
  int nplaces = 0;
};
Shape linear_shape(const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_flatten* flatten, const sjpeg_hip_sheet* sheet, int light) {
  Shape s{nullptr, sizes, orientations, flatten, sheet};
  s.light = light;
  return s;
}

// ---- the plan kinds: the plan function, the format of what it makes, the made pictures as frames at `base` and how
// many they are, the engine's half, and the hint behind a refused yuv_mode
using Frame = sjpeg_hip_ragged_frame;
struct PerFrameKind {                            // (one made picture per frame; the format is any the plan takes)
  static constexpr bool yuv_only = false;
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
    return yuv_colour_plan(who, *p, s.colour, s.colour_per_frame, &p->colour);
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
    return yuv_colour_plan(who, p->planes, s.colour, s.colour_per_frame, &p->colour);
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
    return yuv_colour_plan(who, *p, s.colour, s.colour_per_frame, &p->colour);
  }
};
struct SheetDeepKind : SheetColourKind {
  static constexpr int esz = 2;
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    if (int rc = yuv_format_check(who, format)) return rc;
    if (int rc = yuv_depth_check(who, s.depth)) return rc;
    if (int rc = sheet_plan(who, format, n, fr, s.sheet, s.sizes, s.orientations, p, nullptr, s.depth)) return rc;
    return yuv_colour_plan(who, p->planes, s.colour, s.colour_per_frame, &p->colour);
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
    return resample_plan(who, format, n, fr, s.sizes, s.orientations, s.resample, s.resample_per_frame, s.flatten, p);
  }
  static int format(const Plan& p) { return p.resized_format; }
  static void frames(const Plan& p, const Frame* fr, uint8_t* base, Frame* out) { resample_plan_frames(p, fr, base, out); }
  static constexpr auto run = engine_resample;
};
// ... from a source box and behind a reduce (sjpeg_hip_resample_box_ragged_src; resample_box.hip where a frame is reduced)
struct ResampleBoxKind : ResampleKind {
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    return resample_box_plan(who, format, n, fr, s.sizes, s.orientations, s.resample, s.resample_per_frame, s.box, s.box_per_frame, s.flatten, p);
  }
};

// ... and any per-frame kind K with the unsharp mask behind it (unsharp_plan.cc, unsharp.hip): K's plan, then the
// unsharp plan of the pictures K makes -- read off K's own frames, standing at a placeholder address --; K's pictures
// into the engine's memory, then the unsharp launch from there to the caller's buffer or the engine's final pictures.
// The layout is K's: frames and format are K's
template <class K>
struct UnsharpKind : K {
  struct Plan : K::Plan { UnsharpPlan unsharp; };
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    if (int rc = K::plan(who, format, n, fr, s, p)) return rc;
    uint8_t* const at = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(16));
    std::vector<Frame> made(static_cast<size_t>(n));
    K::frames(*p, fr, at, made.data());
    if (int rc = unsharp_plan(who, K::format(*p), n, made.data(), at, s.unsharp, s.unsharp_per_frame, &p->unsharp)) return rc;
    p->unsharp.bytes = p->bytes;
    return 0;
  }
  static int run(sjpeg_hip_engine* e, const std::string& who, const Plan& p, uint8_t* d_out, uint8_t** base, void* stream) {
    uint8_t* staged = nullptr;
    if (int rc = K::run(e, who, p, nullptr, &staged, stream)) return rc;
    return engine_unsharp(e, who, p.unsharp, staged, d_out, base, stream);
  }
};

// ... and any per-frame kind K with Pillow's filters behind it (pillow_filter_plan.cc, pillow_filter.hip): as
// UnsharpKind, the plan read off K's own frames at a placeholder address; K's pictures into the engine's memory, then
// the two filter launches from there to the caller's buffer or the engine's final pictures
template <class K>
struct FilterKind : K {
  struct Plan : K::Plan { PillowFilterPlan filter; };
  static int plan(const std::string& who, int format, int n, const Frame* fr, const Shape& s, Plan* p) {
    if (int rc = K::plan(who, format, n, fr, s, p)) return rc;
    uint8_t* const at = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(16));
    std::vector<Frame> made(static_cast<size_t>(n));
    K::frames(*p, fr, at, made.data());
    if (int rc = pillow_filter_plan(who, K::format(*p), n, made.data(), at, s.filter, s.filter_per_frame, &p->filter)) return rc;
    p->filter.bytes = p->bytes;
    return 0;
  }
  static int run(sjpeg_hip_engine* e, const std::string& who, const Plan& p, uint8_t* d_out, uint8_t** base, void* stream) {
    uint8_t* staged = nullptr;
    if (int rc = K::run(e, who, p, nullptr, &staged, stream)) return rc;
    return engine_pillow_filter(e, who, p.filter, staged, d_out, base, stream);
  }
};

// ... and any per-frame kind K with the compose stage behind it (compose_plan.cc, compose.hip): K's plan, then the
// compose plan over the pictures K makes, read off K's own frames at a placeholder address; K's pictures into the
// engine's memory, then the one compose launch from there to the caller's buffer or the engine's composed pictures.
// Unlike UnsharpKind and FilterKind it OWNS frames(), bytes and the sizes: the canvases are not K's layout
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
    uint8_t* const at = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(16));
    std::vector<Frame> made(static_cast<size_t>(n));
    K::frames(p->made, fr, at, made.data());
    if (int rc = compose_plan(who, K::format(p->made), n, made.data(), at, s.compose, s.compose_per_frame, s.overlays, s.noverlays, s.places,
                              s.nplaces, &p->compose)) {
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

// ---- the shape entries: the made pictures into the caller's buffer
// the words of an entry's messages: its mandatory pointers, its buffer, its size argument, what it makes and the _bytes
// function that says how much that takes
struct ShapeWords { const char *pointers, *buffer, *bytes, *made, *bytes_fn; };
constexpr ShapeWords kOrientWords = {"frames, d_out, out_frames or out_format", "d_out", "bytes", "oriented pictures",
                                     "sjpeg_hip_orient_ragged_bytes"};
constexpr ShapeWords kSheetWords = {"frames, sheet, d_out, sheet_frames, nsheets or out_format", "d_out", "bytes", "sheets",
                                    "sjpeg_hip_sheet_ragged_bytes"};

// `missing`: one of the entry's mandatory pointers is NULL (the entry knows which it has); count: where the number of
// made pictures goes (NULL: it is nframes)
template <class K>
int shape_body(const std::string& who, const ShapeWords& w, sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
               const Shape& s, bool missing, void* d_out, size_t bytes, sjpeg_hip_ragged_frame* out_frames, int* count, int* out_format,
               void* stream) {
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (missing || frames == nullptr || d_out == nullptr || out_frames == nullptr || out_format == nullptr) {
    return set_error(SJPEG_HIP_EINVAL, who + ": " + w.pointers + " == NULL");
  }
  if ((reinterpret_cast<uintptr_t>(d_out) & 15u) != 0) return set_error(SJPEG_HIP_EINVAL, who + ": " + w.buffer + " must be a multiple of 16");
  try {
    typename K::Plan plan;
    if (K::yuv_only) { if (int rc = yuv_format_check(who, format)) return rc; }
    const SourceLayout* const L = source_layout(format);
    if (L == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": unknown source format");
    if (nframes < 1 || nframes > 65535) return set_error(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
    if (int rc = ragged_check(who, format, source_mode(L), nframes, frames, K::esz)) return rc;
    if (int rc = K::plan(who, format, nframes, frames, s, &plan)) return rc;
    if (bytes < plan.bytes) {
      return set_error(SJPEG_HIP_EINVAL, who + ": " + w.bytes + " " + std::to_string(bytes) + " is below the " + std::to_string(plan.bytes) +
                                             " bytes the " + w.made + " take (" + w.bytes_fn + ")");
    }
    if (int rc = K::run(e, who, plan, static_cast<uint8_t*>(d_out), nullptr, stream)) return rc;
    K::frames(plan, frames, static_cast<uint8_t*>(d_out), out_frames);
    if (count != nullptr) *count = K::count(plan, nframes);
    *out_format = K::format(plan);
    return 0;
  } catch (...) {
    return set_error(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

// ---- the encode entries.  Their names by family: [0] the entry, [1] its packed twin
#define SJPEG_ENTRY_NAMES(stem) {"sjpeg_hip_encode_ragged_" stem "_src", "sjpeg_hip_encode_ragged_" stem "_packed_src"}
const std::string kReduced[2] = SJPEG_ENTRY_NAMES("reduced"), kResized[2] = SJPEG_ENTRY_NAMES("resized"),
                  kOriented[2] = SJPEG_ENTRY_NAMES("oriented"), kFlattened[2] = SJPEG_ENTRY_NAMES("flattened"),
                  kYuvResized[2] = SJPEG_ENTRY_NAMES("yuv_resized"), kSheet[2] = SJPEG_ENTRY_NAMES("sheet"),
                  kSheetFlat[2] = SJPEG_ENTRY_NAMES("sheet_flat"), kYuvConverted[2] = SJPEG_ENTRY_NAMES("yuv_converted"),
                  kSheetColour[2] = SJPEG_ENTRY_NAMES("sheet_yuv_colour"), kYuv16[2] = SJPEG_ENTRY_NAMES("yuv16"),
                  kSheetYuv16[2] = SJPEG_ENTRY_NAMES("sheet_yuv16"), kLinear[2] = SJPEG_ENTRY_NAMES("linear"),
                  kSheetLinear[2] = SJPEG_ENTRY_NAMES("sheet_linear"), kUnsharp[2] = SJPEG_ENTRY_NAMES("unsharp"),
                  kYuvUnsharp[2] = SJPEG_ENTRY_NAMES("yuv_unsharp"), kResampled[2] = SJPEG_ENTRY_NAMES("resampled"),
                  kResampledBox[2] = SJPEG_ENTRY_NAMES("resampled_box"), kFiltered[2] = SJPEG_ENTRY_NAMES("filtered"),
                  kComposed[2] = SJPEG_ENTRY_NAMES("composed");
#undef SJPEG_ENTRY_NAMES

// a packed call's frames go where the placement kernel says: their out_offset is not read
void unplace(const RaggedOut& o, std::vector<sjpeg_hip_ragged_frame>* made) {
  if (o.packed) for (sjpeg_hip_ragged_frame& f : *made) f.out_offset = 0;
}

// The rest of a call whose pictures are planned (prologue done): the remaining checks -- the plan's, the yuv_mode, the
// caller's frames, the inner flow's own on the made pictures (standing at a placeholder address until there is
// memory), the metadata --, then the kernel into the engine's memory for made pictures and ONE inner flow over them,
// read as the plan's format: frame order, packed layout, modes, q_out, value_out, the host waits and the search counters
// are that flow's.
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
    std::vector<sjpeg_hip_ragged_frame> made(static_cast<size_t>(c.nframes));
    K::frames(plan, c.frames, reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(16)), made.data());
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
template <class K = SheetKind>
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
    // (the inner flow's own checks on the sheets, standing at a placeholder address until there is memory)
    made_sheets(reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(16)));
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

// The route rules.  factors NULL or all 1: exactly the _full_meta_ call on the caller's frames.
int reduced_entry(const RaggedCall& c, const uint8_t* factors) {
  if (int rc = encode_prologue(c)) return rc;
  if (int rc = per_frame_range(*c.who, factors, c.nframes, "factor", SJPEG_HIP_REDUCE_MAX, "")) return rc;
  if (all_ones(factors, c.nframes)) return full_entry(c);
  return planned_flow<ReduceKind>(c, Shape{factors});
}
// sizes NULL or every size its frame's own: the _full_meta_ call again
int resized_entry(const RaggedCall& c, const int32_t (*sizes)[2]) {
  if (int rc = encode_prologue(c)) return rc;
  if (all_own_size(sizes, c.nframes, c.frames)) return full_entry(c);
  return planned_flow<ResizeKind>(c, Shape{nullptr, sizes});
}
// orientations NULL or all 1 and no flatten: exactly the resized call on the same arguments (so any format at its own
// sizes still passes through to the _full_meta_ call).  With a flatten every frame goes through the kernel: the inner
// call never sees the alpha format.
int oriented_entry(RaggedCall c, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations) {
  if (int rc = encode_prologue(c)) return rc;
  if (int rc = orientations_check(*c.who, orientations, c.nframes)) return rc;
  if (flatten == nullptr && all_ones(orientations, c.nframes)) {
    c.who = &kResized[c.out.packed];
    return resized_entry(c, sizes);
  }
  return planned_flow<ResizeKind>(c, Shape{nullptr, sizes, orientations, flatten});
}
// flatten NULL: exactly the oriented call
int flattened_entry(RaggedCall c, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations) {
  c.who = flatten != nullptr ? &kFlattened[c.out.packed] : &kOriented[c.out.packed];
  return oriented_entry(c, flatten, sizes, orientations);
}
// every size the frame's own and every orientation 1 (or both NULL): the _full_meta_ call on the caller's planes
int yuv_resized_entry(const RaggedCall& c, const int32_t (*sizes)[2], const uint8_t* orientations) {
  if (int rc = encode_prologue(c, false, nullptr, true)) return rc;
  if (int rc = orientations_check(*c.who, orientations, c.nframes)) return rc;
  if (all_ones(orientations, c.nframes) && all_own_size(sizes, c.nframes, c.frames)) return full_entry(c);
  return planned_flow<YuvResizeKind>(c, Shape{nullptr, sizes, orientations});
}
// no pass-through; flatten NULL: the sheet entry under its own name
int sheet_entry(RaggedCall c, const sjpeg_hip_sheet* sheet, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                const uint8_t* orientations) {
  c.who = flatten != nullptr ? &kSheetFlat[c.out.packed] : &kSheet[c.out.packed];
  if (int rc = encode_prologue(c, true, sheet)) return rc;
  return sheet_flow(c, Shape{nullptr, sizes, orientations, flatten, sheet});
}
// colour NULL or the identity for every frame: exactly the yuv_resized call on the same arguments.  Otherwise every
// frame goes through the resize kernel, at its own size and orientation 1 too: the colour launch works in place, and
// the caller's planes are not its to write.
int yuv_converted_entry(RaggedCall c, const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour,
                        int colour_per_frame) {
  c.who = &kYuvConverted[c.out.packed];
  if (int rc = encode_prologue(c, false, nullptr, true)) return rc;
  if (yuv_colour_all_identity(c.nframes, colour, colour_per_frame)) {
    c.who = &kYuvResized[c.out.packed];
    return yuv_resized_entry(c, sizes, orientations);
  }
  if (int rc = orientations_check(*c.who, orientations, c.nframes)) return rc;
  return planned_flow<YuvColourKind>(c, Shape{nullptr, sizes, orientations, nullptr, nullptr, colour, colour_per_frame});
}
// ... the sheet call, for the YUV-plane formats
int sheet_colour_entry(RaggedCall c, const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2], const uint8_t* orientations,
                       const sjpeg_hip_yuv_colour* colour, int colour_per_frame) {
  c.who = &kSheetColour[c.out.packed];
  if (int rc = encode_prologue(c, true, sheet, true)) return rc;
  if (yuv_colour_all_identity(c.nframes, colour, colour_per_frame)) return sheet_entry(c, sheet, nullptr, sizes, orientations);
  return sheet_flow<SheetColourKind>(c, Shape{nullptr, sizes, orientations, nullptr, sheet, colour, colour_per_frame});
}

// 16-bit samples: no pass-through -- the inner flow cannot read words, so every frame goes through the kernel, at its
// own size and orientation 1 too.  colour NULL: none.
int yuv16_entry(RaggedCall c, const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                const sjpeg_hip_yuv_depth* depth) {
  c.who = &kYuv16[c.out.packed];
  if (int rc = encode_prologue(c, false, nullptr, true)) return rc;
  if (int rc = yuv_depth_check(*c.who, depth)) return rc;
  if (int rc = orientations_check(*c.who, orientations, c.nframes)) return rc;
  return planned_flow<YuvDeepKind>(c, Shape{nullptr, sizes, orientations, nullptr, nullptr, colour, colour_per_frame, depth});
}
int sheet_yuv16_entry(RaggedCall c, const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2], const uint8_t* orientations,
                      const sjpeg_hip_yuv_colour* colour, int colour_per_frame, const sjpeg_hip_yuv_depth* depth) {
  c.who = &kSheetYuv16[c.out.packed];
  if (int rc = encode_prologue(c, true, sheet, true)) return rc;
  if (int rc = yuv_depth_check(*c.who, depth)) return rc;
  return sheet_flow<SheetDeepKind>(c, Shape{nullptr, sizes, orientations, nullptr, sheet, colour, colour_per_frame, depth});
}


// Linear light.  light == SJPEG_HIP_LIGHT_CODED: exactly the flattened call (which hands on to the oriented one without
// a flatten) on the same arguments.  Otherwise no pass-through: every frame goes through the kernel, at its own size
// and orientation 1 too -- a copy, because the inverse is exact.
int linear_entry(RaggedCall c, const sjpeg_hip_flatten* flatten, int light, const int32_t (*sizes)[2], const uint8_t* orientations) {
  if (light == SJPEG_HIP_LIGHT_CODED) return flattened_entry(c, flatten, sizes, orientations);
  c.who = &kLinear[c.out.packed];
  if (int rc = encode_prologue(c)) return rc;
  if (int rc = light_check(*c.who, light, c.format)) return rc;
  if (int rc = orientations_check(*c.who, orientations, c.nframes)) return rc;
  return planned_flow<LinearKind>(c, linear_shape(sizes, orientations, flatten, nullptr, light));
}
int sheet_linear_entry(RaggedCall c, const sjpeg_hip_sheet* sheet, const sjpeg_hip_flatten* flatten, int light, const int32_t (*sizes)[2],
                       const uint8_t* orientations) {
  if (light == SJPEG_HIP_LIGHT_CODED) return sheet_entry(c, sheet, flatten, sizes, orientations);
  c.who = &kSheetLinear[c.out.packed];
  if (int rc = encode_prologue(c, true, sheet)) return rc;
  if (int rc = light_check(*c.who, light, c.format)) return rc;
  return sheet_flow<SheetLinearKind>(c, linear_shape(sizes, orientations, flatten, sheet, light));
}

// The unsharp mask.  unsharp NULL or amount 0 for every frame: exactly the linear call (which hands on to the flattened
// one in coded light) or, for the YUV-plane formats, the yuv16 call or without a depth the yuv_converted one, on the
// same arguments.  Otherwise no pass-through: every frame goes through the resize kernel, at its own size and
// orientation 1 too -- the unsharp launch reads the made pictures, whatever the source format.  A format of the other
// family is refused by name and pointed at the entries that take it.
bool nothing_to_sharpen(int nframes, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame) {
  // (unsharp is [nframes] only where nframes is a count)
  return unsharp == nullptr || ((unsharp_per_frame == 0 || (nframes >= 1 && nframes <= 65535)) && unsharp_all_zero(nframes, unsharp, unsharp_per_frame));
}
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
Shape unsharp_shape(Shape s, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame) {
  s.unsharp = unsharp; s.unsharp_per_frame = unsharp_per_frame;
  return s;
}
int unsharp_entry(RaggedCall c, const sjpeg_hip_flatten* flatten, int light, const int32_t (*sizes)[2], const uint8_t* orientations,
                  const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame) {
  if (nothing_to_sharpen(c.nframes, unsharp, unsharp_per_frame)) return linear_entry(c, flatten, light, sizes, orientations);
  c.who = &kUnsharp[c.out.packed];
  if (int rc = encode_prologue(c)) return rc;
  if (int rc = unsharp_family_check(*c.who, c.format, false)) return rc;
  if (int rc = light_check(*c.who, light, c.format)) return rc;
  if (int rc = unsharp_check(*c.who, c.nframes, unsharp, unsharp_per_frame)) return rc;
  if (int rc = orientations_check(*c.who, orientations, c.nframes)) return rc;
  return planned_flow<UnsharpKind<LinearKind>>(c, unsharp_shape(linear_shape(sizes, orientations, flatten, nullptr, light), unsharp, unsharp_per_frame));
}
int yuv_unsharp_entry(RaggedCall c, const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                      const sjpeg_hip_yuv_depth* depth, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame) {
  if (nothing_to_sharpen(c.nframes, unsharp, unsharp_per_frame)) {
    if (depth == nullptr) return yuv_converted_entry(c, sizes, orientations, colour, colour_per_frame);
    return yuv16_entry(c, sizes, orientations, colour, colour_per_frame, depth);
  }
  c.who = &kYuvUnsharp[c.out.packed];
  if (int rc = encode_prologue(c)) return rc;
  if (int rc = unsharp_family_check(*c.who, c.format, true)) return rc;
  if (depth != nullptr) { if (int rc = yuv_depth_check(*c.who, depth)) return rc; }
  if (int rc = unsharp_check(*c.who, c.nframes, unsharp, unsharp_per_frame)) return rc;
  if (int rc = orientations_check(*c.who, orientations, c.nframes)) return rc;
  const Shape s = unsharp_shape(Shape{nullptr, sizes, orientations, nullptr, nullptr, colour, colour_per_frame, depth}, unsharp, unsharp_per_frame);
  if (depth == nullptr) return planned_flow<UnsharpKind<YuvColourKind>>(c, s);
  return planned_flow<UnsharpKind<YuvDeepKind>>(c, s);
}

// Resampling with Pillow's filters.  No pass-through: every frame goes through the resample kernel, at its own size too
// (a copy: the identity tables).  unsharp NULL or amount 0 for every frame: the made pictures are the call's; otherwise
// the unsharp launch runs behind the resample launch, unchanged.
Shape resample_shape(const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_flatten* flatten, const sjpeg_hip_resample* resample,
                     int resample_per_frame, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame) {
  Shape s{nullptr, sizes, orientations, flatten};
  s.resample = resample; s.resample_per_frame = resample_per_frame;
  s.unsharp = unsharp; s.unsharp_per_frame = unsharp_per_frame;
  return s;
}
int resampled_entry(RaggedCall c, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations,
                    const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame) {
  c.who = &kResampled[c.out.packed];
  if (int rc = encode_prologue(c)) return rc;
  if (int rc = resample_check(*c.who, c.nframes, resample, resample_per_frame)) return rc;
  if (int rc = orientations_check(*c.who, orientations, c.nframes)) return rc;
  const Shape s = resample_shape(sizes, orientations, flatten, resample, resample_per_frame, unsharp, unsharp_per_frame);
  if (nothing_to_sharpen(c.nframes, unsharp, unsharp_per_frame)) return planned_flow<ResampleKind>(c, s);
  return planned_flow<UnsharpKind<ResampleKind>>(c, s);
}
// ... from a source box and behind a reduce: the same, the plan the box kind's
int resampled_box_entry(RaggedCall c, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations,
                        const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_resample_box* box, int box_per_frame,
                        const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame) {
  c.who = &kResampledBox[c.out.packed];
  if (int rc = encode_prologue(c)) return rc;
  if (int rc = resample_check(*c.who, c.nframes, resample, resample_per_frame)) return rc;
  if (box == nullptr) return set_error(SJPEG_HIP_EINVAL, *c.who + ": box == NULL");
  if (int rc = orientations_check(*c.who, orientations, c.nframes)) return rc;
  Shape s = resample_shape(sizes, orientations, flatten, resample, resample_per_frame, unsharp, unsharp_per_frame);
  s.box = box; s.box_per_frame = box_per_frame;
  if (nothing_to_sharpen(c.nframes, unsharp, unsharp_per_frame)) return planned_flow<ResampleBoxKind>(c, s);
  return planned_flow<UnsharpKind<ResampleBoxKind>>(c, s);
}

// Pillow's filters behind the box entries.  filter NULL or kind 0 for every frame: exactly the resampled_box call
// without unsharp on the same arguments, under its name.  Otherwise the two filter launches run behind the resample
// launch over every frame, those of kind 0 copied.
bool nothing_to_filter(int nframes, const sjpeg_hip_pillow_filter* filter, int filter_per_frame) {
  // (filter is [nframes] only where nframes is a count)
  return filter == nullptr || ((filter_per_frame == 0 || (nframes >= 1 && nframes <= 65535)) && pillow_filter_all_none(nframes, filter, filter_per_frame));
}
int filtered_entry(RaggedCall c, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations,
                   const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_resample_box* box, int box_per_frame,
                   const sjpeg_hip_pillow_filter* filter, int filter_per_frame) {
  if (nothing_to_filter(c.nframes, filter, filter_per_frame)) {
    return resampled_box_entry(c, flatten, sizes, orientations, resample, resample_per_frame, box, box_per_frame, nullptr, 0);
  }
  c.who = &kFiltered[c.out.packed];
  if (int rc = encode_prologue(c)) return rc;
  if (int rc = resample_check(*c.who, c.nframes, resample, resample_per_frame)) return rc;
  if (box == nullptr) return set_error(SJPEG_HIP_EINVAL, *c.who + ": box == NULL");
  if (int rc = pillow_filter_check(*c.who, c.nframes, filter, filter_per_frame)) return rc;
  if (int rc = orientations_check(*c.who, orientations, c.nframes)) return rc;
  Shape s = resample_shape(sizes, orientations, flatten, resample, resample_per_frame, nullptr, 0);
  s.box = box; s.box_per_frame = box_per_frame;
  s.filter = filter; s.filter_per_frame = filter_per_frame;
  return planned_flow<FilterKind<ResampleBoxKind>>(c, s);
}

// The compose stage behind the filtered entries.  compose NULL, or every frame an identity -- a canvas of 0 x 0, or of
// the made picture's own size with the picture at (0, 0), and no place --: exactly the filtered call on the same
// arguments, under its name.  Otherwise one compose launch runs behind the launches that made the pictures; a call
// none of whose frames has a filter runs no filter launch.
struct ComposeArgs {
  const sjpeg_hip_compose* compose;
  int compose_per_frame;
  const sjpeg_hip_overlay* overlays;
  int noverlays;
  const sjpeg_hip_overlay_place* places;
  int nplaces;
};
// whether every frame is an identity; a call with a canvas that the box plan refuses is not: this entry says why
bool nothing_to_compose(int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2], const uint8_t* orientations,
                        const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_resample_box* box, int box_per_frame,
                        const sjpeg_hip_flatten* flatten, const ComposeArgs& a) {
  if (a.compose == nullptr) return true;
  if (a.compose_per_frame != 0 && (nframes < 1 || nframes > 65535)) return false;      // (compose is [nframes] only where nframes is a count)
  if (compose_all_none(nframes, a.compose, a.compose_per_frame)) return true;
  // a frame with a canvas: an identity where the canvas is the made picture's size -- which the plan knows
  const int n = a.compose_per_frame != 0 ? nframes : 1;
  for (int f = 0; f < n; ++f) if (a.compose[f].nplaces != 0) return false;
  if (frames == nullptr || resample == nullptr || box == nullptr || nframes < 1 || nframes > 65535 || source_layout(format) == nullptr) return false;
  static const std::string quiet = "sjpeg_hip_compose_ragged_src";
  if (compose_check(quiet, nframes, a.compose, a.compose_per_frame, a.overlays, a.noverlays, a.places, a.nplaces) != 0) return false;
  try {
    ResamplePlan made;
    if (resample_box_plan(quiet, format, nframes, frames, sizes, orientations, resample, resample_per_frame, box, box_per_frame, flatten, &made) != 0) {
      return false;
    }
    std::vector<Frame> pictures(static_cast<size_t>(nframes));
    resample_plan_frames(made, frames, reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(16)), pictures.data());
    for (int f = 0; f < nframes; ++f) {
      const sjpeg_hip_compose& c = a.compose[a.compose_per_frame != 0 ? f : 0];
      const bool own = c.canvas_width == 0 && c.canvas_height == 0;
      if (!own && (c.canvas_width != pictures[f].width || c.canvas_height != pictures[f].height)) return false;
      if (c.mode == 0 && (c.px != 0 || c.py != 0)) return false;
    }
    return true;
  } catch (...) {
    return false;
  }
}
Shape composed_shape(const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_resample* resample,
                     int resample_per_frame, const sjpeg_hip_resample_box* box, int box_per_frame, const sjpeg_hip_pillow_filter* filter,
                     int filter_per_frame, const ComposeArgs& a) {
  Shape s = resample_shape(sizes, orientations, flatten, resample, resample_per_frame, nullptr, 0);
  s.box = box; s.box_per_frame = box_per_frame;
  s.filter = filter; s.filter_per_frame = filter_per_frame;
  s.compose = a.compose; s.compose_per_frame = a.compose_per_frame;
  s.overlays = a.overlays; s.noverlays = a.noverlays;
  s.places = a.places; s.nplaces = a.nplaces;
  return s;
}
int composed_entry(RaggedCall c, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations,
                   const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_resample_box* box, int box_per_frame,
                   const sjpeg_hip_pillow_filter* filter, int filter_per_frame, const ComposeArgs& a) {
  if (nothing_to_compose(c.format, c.nframes, c.frames, sizes, orientations, resample, resample_per_frame, box, box_per_frame, flatten, a)) {
    return filtered_entry(c, flatten, sizes, orientations, resample, resample_per_frame, box, box_per_frame, filter, filter_per_frame);
  }
  c.who = &kComposed[c.out.packed];
  if (int rc = encode_prologue(c)) return rc;
  if (int rc = resample_check(*c.who, c.nframes, resample, resample_per_frame)) return rc;
  if (box == nullptr) return set_error(SJPEG_HIP_EINVAL, *c.who + ": box == NULL");
  if (int rc = pillow_filter_check(*c.who, c.nframes, filter, filter_per_frame)) return rc;
  if (int rc = compose_check(*c.who, c.nframes, a.compose, a.compose_per_frame, a.overlays, a.noverlays, a.places, a.nplaces)) return rc;
  if (int rc = orientations_check(*c.who, orientations, c.nframes)) return rc;
  const Shape s = composed_shape(flatten, sizes, orientations, resample, resample_per_frame, box, box_per_frame, filter, filter_per_frame, a);
  if (nothing_to_filter(c.nframes, filter, filter_per_frame)) return planned_flow<ComposeKind<ResampleBoxKind>>(c, s);
  return planned_flow<ComposeKind<FilterKind<ResampleBoxKind>>>(c, s);
}

}  // namespace

extern "C" {

// ---- pictures reduced by their factors: thumbnails and pyramid levels
int sjpeg_hip_reduce_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                const uint8_t* factors, void* d_reduced, size_t reduced_bytes,
                                sjpeg_hip_ragged_frame* reduced_frames, int* reduced_format, void* stream) {
  static const std::string who = "sjpeg_hip_reduce_ragged_src";
  static constexpr ShapeWords w = {"frames, factors, d_reduced, reduced_frames or reduced_format", "d_reduced", "reduced_bytes",
                                   "reduced pictures", "sjpeg_hip_reduce_ragged_bytes"};
  return shape_body<ReduceKind>(who, w, e, format, nframes, frames, Shape{factors}, factors == nullptr, d_reduced, reduced_bytes,
                                reduced_frames, nullptr, reduced_format, stream);
}

int sjpeg_hip_encode_ragged_reduced_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                        const sjpeg_hip_ragged_params* params, const uint8_t* factors,
                                        const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, uint64_t* d_sizes,
                                        int* modes, float* q_out, float* value_out, void* stream) {
  return reduced_entry({&kReduced[0], e, format, nframes, frames, params, meta, meta_per_frame,
                        {d_out, d_sizes, modes, q_out, value_out, stream}}, factors);
}

int sjpeg_hip_encode_ragged_reduced_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                               const sjpeg_hip_ragged_params* params, const uint8_t* factors,
                                               const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed,
                                               size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes, int* modes,
                                               float* q_out, float* value_out, void* stream) {
  return reduced_entry({&kReduced[1], e, format, nframes, frames, params, meta, meta_per_frame,
                        RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, factors);
}

// ---- ... resized to their sizes: thumbnails that fit a box
int sjpeg_hip_resize_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                const int32_t (*sizes)[2], void* d_resized, size_t resized_bytes,
                                sjpeg_hip_ragged_frame* resized_frames, int* resized_format, void* stream) {
  static const std::string who = "sjpeg_hip_resize_ragged_src";
  static constexpr ShapeWords w = {"frames, sizes, d_resized, resized_frames or resized_format", "d_resized", "resized_bytes",
                                   "resized pictures", "sjpeg_hip_resize_ragged_bytes"};
  return shape_body<ResizeKind>(who, w, e, format, nframes, frames, Shape{nullptr, sizes}, sizes == nullptr, d_resized, resized_bytes,
                                resized_frames, nullptr, resized_format, stream);
}

int sjpeg_hip_encode_ragged_resized_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                        const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2],
                                        const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, uint64_t* d_sizes,
                                        int* modes, float* q_out, float* value_out, void* stream) {
  return resized_entry({&kResized[0], e, format, nframes, frames, params, meta, meta_per_frame,
                        {d_out, d_sizes, modes, q_out, value_out, stream}}, sizes);
}

int sjpeg_hip_encode_ragged_resized_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                               const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2],
                                               const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed,
                                               size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes, int* modes,
                                               float* q_out, float* value_out, void* stream) {
  return resized_entry({&kResized[1], e, format, nframes, frames, params, meta, meta_per_frame,
                        RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, sizes);
}

// ---- ... and turned upright by their EXIF orientations in the same ONE launch (orient_math.h): the kernel stores every
// tile where it lands in the upright picture
int sjpeg_hip_orient_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                const int32_t (*sizes)[2], const uint8_t* orientations, void* d_out, size_t out_bytes,
                                sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_orient_ragged_src";
  return shape_body<ResizeKind>(who, kOrientWords, e, format, nframes, frames, Shape{nullptr, sizes, orientations}, false, d_out,
                                out_bytes, out_frames, nullptr, out_format, stream);
}

int sjpeg_hip_encode_ragged_oriented_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                         const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                         const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, uint64_t* d_sizes,
                                         int* modes, float* q_out, float* value_out, void* stream) {
  return oriented_entry({&kOriented[0], e, format, nframes, frames, params, meta, meta_per_frame,
                         {d_out, d_sizes, modes, q_out, value_out, stream}}, nullptr, sizes, orientations);
}

int sjpeg_hip_encode_ragged_oriented_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2],
                                                const uint8_t* orientations, const sjpeg_hip_metadata* meta, int meta_per_frame,
                                                void* d_packed, size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes,
                                                int* modes, float* q_out, float* value_out, void* stream) {
  return oriented_entry({&kOriented[1], e, format, nframes, frames, params, meta, meta_per_frame,
                         RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, nullptr, sizes,
                        orientations);
}

// ---- ... and flattened over a background as they are staged (flatten_math.h), still ONE launch: RGBA pictures.  The
// shape entry wants its flatten (`flatten` goes into the plan, whose checks of it come with its others).
int sjpeg_hip_flatten_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                 const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations, void* d_out,
                                 size_t out_bytes, sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_flatten_ragged_src";
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (flatten == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": flatten == NULL");
  return shape_body<ResizeKind>(who, kOrientWords, e, format, nframes, frames, Shape{nullptr, sizes, orientations, flatten}, false, d_out,
                                out_bytes, out_frames, nullptr, out_format, stream);
}

int sjpeg_hip_encode_ragged_flattened_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                          const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten,
                                          const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_metadata* meta,
                                          int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                          void* stream) {
  return flattened_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                          {d_out, d_sizes, modes, q_out, value_out, stream}}, flatten, sizes, orientations);
}

int sjpeg_hip_encode_ragged_flattened_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                 const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten,
                                                 const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_metadata* meta,
                                                 int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets,
                                                 uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return flattened_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                          RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, flatten, sizes,
                         orientations);
}

// ---- ... and decoded video: NV12, NV21 and planar YUV resized and turned plane by plane, every plane a picture of its
// own, still ONE launch; the inner flow codes the planes as planar 4:2:0 or 4:4:4
int sjpeg_hip_resize_ragged_yuv_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                    const int32_t (*sizes)[2], const uint8_t* orientations, void* d_out, size_t out_bytes,
                                    sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_resize_ragged_yuv_src";
  static constexpr ShapeWords w = {kOrientWords.pointers, "d_out", "bytes", "resized planes", "sjpeg_hip_resize_ragged_yuv_bytes"};
  return shape_body<YuvResizeKind>(who, w, e, format, nframes, frames, Shape{nullptr, sizes, orientations}, false, d_out, out_bytes,
                                   out_frames, nullptr, out_format, stream);
}

int sjpeg_hip_encode_ragged_yuv_resized_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                            const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                            const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, uint64_t* d_sizes,
                                            int* modes, float* q_out, float* value_out, void* stream) {
  return yuv_resized_entry({&kYuvResized[0], e, format, nframes, frames, params, meta, meta_per_frame,
                            {d_out, d_sizes, modes, q_out, value_out, stream}}, sizes, orientations);
}

int sjpeg_hip_encode_ragged_yuv_resized_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                   const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2],
                                                   const uint8_t* orientations, const sjpeg_hip_metadata* meta, int meta_per_frame,
                                                   void* d_packed, size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes,
                                                   int* modes, float* q_out, float* value_out, void* stream) {
  return yuv_resized_entry({&kYuvResized[1], e, format, nframes, frames, params, meta, meta_per_frame,
                            RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, sizes,
                           orientations);
}

// ---- ... and contact sheets: the batch resized, turned and placed into grid pictures; one set of entries for both
// families of formats
int sjpeg_hip_sheet_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                               const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2], const uint8_t* orientations, void* d_out,
                               size_t out_bytes, sjpeg_hip_ragged_frame* sheet_frames, int* nsheets, int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_sheet_ragged_src";
  return shape_body<SheetKind>(who, kSheetWords, e, format, nframes, frames, Shape{nullptr, sizes, orientations, nullptr, sheet},
                               sheet == nullptr || nsheets == nullptr, d_out, out_bytes, sheet_frames, nsheets, out_format, stream);
}

int sjpeg_hip_sheet_ragged_flat_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                    const sjpeg_hip_sheet* sheet, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                    const uint8_t* orientations, void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* sheet_frames,
                                    int* nsheets, int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_sheet_ragged_flat_src";
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (flatten == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": flatten == NULL");
  return shape_body<SheetKind>(who, kSheetWords, e, format, nframes, frames, Shape{nullptr, sizes, orientations, flatten, sheet},
                               sheet == nullptr || nsheets == nullptr, d_out, out_bytes, sheet_frames, nsheets, out_format, stream);
}

int sjpeg_hip_encode_ragged_sheet_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                      const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2],
                                      const uint8_t* orientations, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out,
                                      size_t out_stride, uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return sheet_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                      RaggedOut{d_out, d_sizes, modes, q_out, value_out, stream}.strided_by(out_stride)}, sheet, nullptr, sizes, orientations);
}

int sjpeg_hip_encode_ragged_sheet_flat_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                           const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                           const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations,
                                           const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, size_t out_stride,
                                           uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return sheet_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                      RaggedOut{d_out, d_sizes, modes, q_out, value_out, stream}.strided_by(out_stride)}, sheet, flatten, sizes, orientations);
}

int sjpeg_hip_encode_ragged_sheet_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                             const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                             const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_metadata* meta,
                                             int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets,
                                             uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return sheet_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                      RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, sheet, nullptr, sizes,
                     orientations);
}

int sjpeg_hip_encode_ragged_sheet_flat_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                  const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                                  const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                                  const uint8_t* orientations, const sjpeg_hip_metadata* meta, int meta_per_frame,
                                                  void* d_packed, size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes,
                                                  int* modes, float* q_out, float* value_out, void* stream) {
  return sheet_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                      RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, sheet, flatten, sizes,
                     orientations);
}

// ---- ... and video colour: the made planes, or the thumbnails' rectangles of a sheet, converted to JFIF's full-range
// BT.601 by ONE more launch behind the resize launch (yuv_colour.hip)
int sjpeg_hip_convert_ragged_yuv_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                     const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour,
                                     int colour_per_frame, void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* out_frames,
                                     int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_convert_ragged_yuv_src";
  static constexpr ShapeWords w = {kOrientWords.pointers, "d_out", "bytes", "converted planes", "sjpeg_hip_resize_ragged_yuv_bytes"};
  // (nothing to convert: the resize entry itself; colour is [nframes] only where nframes is a count)
  if (colour == nullptr || (nframes >= 1 && nframes <= 65535 && yuv_colour_all_identity(nframes, colour, colour_per_frame))) {
    return sjpeg_hip_resize_ragged_yuv_src(e, format, nframes, frames, sizes, orientations, d_out, out_bytes, out_frames, out_format, stream);
  }
  return shape_body<YuvColourKind>(who, w, e, format, nframes, frames, Shape{nullptr, sizes, orientations, nullptr, nullptr, colour, colour_per_frame},
                                   false, d_out, out_bytes, out_frames, nullptr, out_format, stream);
}

int sjpeg_hip_encode_ragged_yuv_converted_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                              const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                              const sjpeg_hip_yuv_colour* colour, int colour_per_frame, const sjpeg_hip_metadata* meta,
                                              int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                              void* stream) {
  return yuv_converted_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                              {d_out, d_sizes, modes, q_out, value_out, stream}}, sizes, orientations, colour, colour_per_frame);
}

int sjpeg_hip_encode_ragged_yuv_converted_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                     const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2],
                                                     const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                                                     const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed,
                                                     size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes, int* modes,
                                                     float* q_out, float* value_out, void* stream) {
  return yuv_converted_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                              RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, sizes,
                             orientations, colour, colour_per_frame);
}

int sjpeg_hip_sheet_ragged_yuv_colour_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                          const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2], const uint8_t* orientations,
                                          const sjpeg_hip_yuv_colour* colour, int colour_per_frame, void* d_out, size_t out_bytes,
                                          sjpeg_hip_ragged_frame* sheet_frames, int* nsheets, int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_sheet_ragged_yuv_colour_src";
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (int rc = yuv_format_check(who, format)) return rc;
  if (colour == nullptr || (nframes >= 1 && nframes <= 65535 && yuv_colour_all_identity(nframes, colour, colour_per_frame))) {
    return sjpeg_hip_sheet_ragged_src(e, format, nframes, frames, sheet, sizes, orientations, d_out, out_bytes, sheet_frames, nsheets, out_format,
                                      stream);
  }
  return shape_body<SheetColourKind>(who, kSheetWords, e, format, nframes, frames,
                                     Shape{nullptr, sizes, orientations, nullptr, sheet, colour, colour_per_frame},
                                     sheet == nullptr || nsheets == nullptr, d_out, out_bytes, sheet_frames, nsheets, out_format, stream);
}

int sjpeg_hip_encode_ragged_sheet_yuv_colour_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                 const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2],
                                                 const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                                                 const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, size_t out_stride,
                                                 uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return sheet_colour_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                             RaggedOut{d_out, d_sizes, modes, q_out, value_out, stream}.strided_by(out_stride)}, sheet, sizes, orientations, colour,
                            colour_per_frame);
}

int sjpeg_hip_encode_ragged_sheet_yuv_colour_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                        const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                                        const int32_t (*sizes)[2], const uint8_t* orientations,
                                                        const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                                                        const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed,
                                                        size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes, int* modes,
                                                        float* q_out, float* value_out, void* stream) {
  return sheet_colour_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                             RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, sheet, sizes,
                            orientations, colour, colour_per_frame);
}

// ---- ... and 10-bit video: the YUV-plane formats with 16-bit samples (P010 and its kin, yuv420p10le / 12le) through the
// kernel's deep instantiations; each entry its colour counterpart plus the depth
int sjpeg_hip_convert_ragged_yuv16_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                       const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour,
                                       int colour_per_frame, const sjpeg_hip_yuv_depth* depth, void* d_out, size_t out_bytes,
                                       sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_convert_ragged_yuv16_src";
  static constexpr ShapeWords w = {kOrientWords.pointers, "d_out", "bytes", "converted planes", "sjpeg_hip_resize_ragged_yuv_bytes"};
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (int rc = yuv_depth_check(who, depth)) return rc;
  return shape_body<YuvDeepKind>(who, w, e, format, nframes, frames,
                                 Shape{nullptr, sizes, orientations, nullptr, nullptr, colour, colour_per_frame, depth}, false, d_out, out_bytes,
                                 out_frames, nullptr, out_format, stream);
}

int sjpeg_hip_encode_ragged_yuv16_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                      const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                      const sjpeg_hip_yuv_colour* colour, int colour_per_frame, const sjpeg_hip_yuv_depth* depth,
                                      const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes,
                                      float* q_out, float* value_out, void* stream) {
  return yuv16_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                      {d_out, d_sizes, modes, q_out, value_out, stream}}, sizes, orientations, colour, colour_per_frame, depth);
}

int sjpeg_hip_encode_ragged_yuv16_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                             const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                             const sjpeg_hip_yuv_colour* colour, int colour_per_frame, const sjpeg_hip_yuv_depth* depth,
                                             const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed, size_t packed_capacity,
                                             uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                             void* stream) {
  return yuv16_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                      RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, sizes,
                     orientations, colour, colour_per_frame, depth);
}

int sjpeg_hip_sheet_ragged_yuv16_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                     const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2], const uint8_t* orientations,
                                     const sjpeg_hip_yuv_colour* colour, int colour_per_frame, const sjpeg_hip_yuv_depth* depth,
                                     void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* sheet_frames, int* nsheets, int* out_format,
                                     void* stream) {
  static const std::string who = "sjpeg_hip_sheet_ragged_yuv16_src";
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (int rc = yuv_format_check(who, format)) return rc;
  if (int rc = yuv_depth_check(who, depth)) return rc;
  return shape_body<SheetDeepKind>(who, kSheetWords, e, format, nframes, frames,
                                   Shape{nullptr, sizes, orientations, nullptr, sheet, colour, colour_per_frame, depth},
                                   sheet == nullptr || nsheets == nullptr, d_out, out_bytes, sheet_frames, nsheets, out_format, stream);
}

int sjpeg_hip_encode_ragged_sheet_yuv16_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                            const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2],
                                            const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                                            const sjpeg_hip_yuv_depth* depth, const sjpeg_hip_metadata* meta, int meta_per_frame,
                                            void* d_out, size_t out_stride, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                            void* stream) {
  return sheet_yuv16_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                            RaggedOut{d_out, d_sizes, modes, q_out, value_out, stream}.strided_by(out_stride)}, sheet, sizes, orientations,
                           colour, colour_per_frame, depth);
}

int sjpeg_hip_encode_ragged_sheet_yuv16_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                   const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                                   const int32_t (*sizes)[2], const uint8_t* orientations,
                                                   const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                                                   const sjpeg_hip_yuv_depth* depth, const sjpeg_hip_metadata* meta, int meta_per_frame,
                                                   void* d_packed, size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes,
                                                   int* modes, float* q_out, float* value_out, void* stream) {
  return sheet_yuv16_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                            RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, sheet,
                           sizes, orientations, colour, colour_per_frame, depth);
}

// ---- ... and the resize in linear light: the flattened and sheet entries plus `light` (light_math.h), through the
// kernel's linear instantiations; flatten may be NULL
int sjpeg_hip_linear_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                const sjpeg_hip_flatten* flatten, int light, const int32_t (*sizes)[2], const uint8_t* orientations,
                                void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_linear_ragged_src";
  if (light == SJPEG_HIP_LIGHT_CODED) {
    if (flatten == nullptr) return sjpeg_hip_orient_ragged_src(e, format, nframes, frames, sizes, orientations, d_out, out_bytes, out_frames, out_format, stream);
    return sjpeg_hip_flatten_ragged_src(e, format, nframes, frames, flatten, sizes, orientations, d_out, out_bytes, out_frames, out_format, stream);
  }
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (int rc = light_check(who, light, format)) return rc;
  return shape_body<LinearKind>(who, kOrientWords, e, format, nframes, frames, linear_shape(sizes, orientations, flatten, nullptr, light), false,
                                d_out, out_bytes, out_frames, nullptr, out_format, stream);
}

int sjpeg_hip_encode_ragged_linear_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                       const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, int light,
                                       const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_metadata* meta,
                                       int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                       void* stream) {
  return linear_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                       {d_out, d_sizes, modes, q_out, value_out, stream}}, flatten, light, sizes, orientations);
}

int sjpeg_hip_encode_ragged_linear_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                              const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, int light,
                                              const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_metadata* meta,
                                              int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets,
                                              uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return linear_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                       RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, flatten, light,
                      sizes, orientations);
}

int sjpeg_hip_sheet_ragged_linear_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                      const sjpeg_hip_sheet* sheet, const sjpeg_hip_flatten* flatten, int light, const int32_t (*sizes)[2],
                                      const uint8_t* orientations, void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* sheet_frames,
                                      int* nsheets, int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_sheet_ragged_linear_src";
  if (light == SJPEG_HIP_LIGHT_CODED) {
    if (flatten == nullptr) {
      return sjpeg_hip_sheet_ragged_src(e, format, nframes, frames, sheet, sizes, orientations, d_out, out_bytes, sheet_frames, nsheets, out_format, stream);
    }
    return sjpeg_hip_sheet_ragged_flat_src(e, format, nframes, frames, sheet, flatten, sizes, orientations, d_out, out_bytes, sheet_frames, nsheets,
                                           out_format, stream);
  }
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (int rc = light_check(who, light, format)) return rc;
  return shape_body<SheetLinearKind>(who, kSheetWords, e, format, nframes, frames, linear_shape(sizes, orientations, flatten, sheet, light),
                                     sheet == nullptr || nsheets == nullptr, d_out, out_bytes, sheet_frames, nsheets, out_format, stream);
}

int sjpeg_hip_encode_ragged_sheet_linear_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                             const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                             const sjpeg_hip_flatten* flatten, int light, const int32_t (*sizes)[2],
                                             const uint8_t* orientations, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out,
                                             size_t out_stride, uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return sheet_linear_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                             RaggedOut{d_out, d_sizes, modes, q_out, value_out, stream}.strided_by(out_stride)}, sheet, flatten, light, sizes,
                            orientations);
}

int sjpeg_hip_encode_ragged_sheet_linear_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                    const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                                    const sjpeg_hip_flatten* flatten, int light, const int32_t (*sizes)[2],
                                                    const uint8_t* orientations, const sjpeg_hip_metadata* meta, int meta_per_frame,
                                                    void* d_packed, size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes,
                                                    int* modes, float* q_out, float* value_out, void* stream) {
  return sheet_linear_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                             RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, sheet,
                            flatten, light, sizes, orientations);
}

// ---- ... and the unsharp mask behind any of it: the linear entries and the yuv16 entries plus `unsharp`; ONE more
// launch over the made pictures (unsharp.hip), out of place
int sjpeg_hip_unsharp_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                 const sjpeg_hip_flatten* flatten, int light, const int32_t (*sizes)[2], const uint8_t* orientations,
                                 const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, void* d_out, size_t out_bytes,
                                 sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_unsharp_ragged_src";
  if (nothing_to_sharpen(nframes, unsharp, unsharp_per_frame)) {
    return sjpeg_hip_linear_ragged_src(e, format, nframes, frames, flatten, light, sizes, orientations, d_out, out_bytes, out_frames, out_format,
                                       stream);
  }
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (int rc = unsharp_family_check(who, format, false)) return rc;
  if (int rc = light_check(who, light, format)) return rc;
  return shape_body<UnsharpKind<LinearKind>>(who, kOrientWords, e, format, nframes, frames,
                                             unsharp_shape(linear_shape(sizes, orientations, flatten, nullptr, light), unsharp, unsharp_per_frame),
                                             false, d_out, out_bytes, out_frames, nullptr, out_format, stream);
}

int sjpeg_hip_encode_ragged_unsharp_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                        const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, int light,
                                        const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_unsharp* unsharp,
                                        int unsharp_per_frame, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out,
                                        uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return unsharp_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                        {d_out, d_sizes, modes, q_out, value_out, stream}}, flatten, light, sizes, orientations, unsharp, unsharp_per_frame);
}

int sjpeg_hip_encode_ragged_unsharp_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                               const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, int light,
                                               const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_unsharp* unsharp,
                                               int unsharp_per_frame, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed,
                                               size_t packed_capacity, uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out,
                                               float* value_out, void* stream) {
  return unsharp_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                        RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, flatten, light,
                       sizes, orientations, unsharp, unsharp_per_frame);
}

int sjpeg_hip_unsharp_ragged_yuv_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                     const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_yuv_colour* colour,
                                     int colour_per_frame, const sjpeg_hip_yuv_depth* depth, const sjpeg_hip_unsharp* unsharp,
                                     int unsharp_per_frame, void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* out_frames,
                                     int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_unsharp_ragged_yuv_src";
  static constexpr ShapeWords w = {kOrientWords.pointers, "d_out", "bytes", "sharpened planes", "sjpeg_hip_resize_ragged_yuv_bytes"};
  if (nothing_to_sharpen(nframes, unsharp, unsharp_per_frame)) {
    if (depth == nullptr) {
      return sjpeg_hip_convert_ragged_yuv_src(e, format, nframes, frames, sizes, orientations, colour, colour_per_frame, d_out, out_bytes,
                                              out_frames, out_format, stream);
    }
    return sjpeg_hip_convert_ragged_yuv16_src(e, format, nframes, frames, sizes, orientations, colour, colour_per_frame, depth, d_out, out_bytes,
                                              out_frames, out_format, stream);
  }
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (int rc = unsharp_family_check(who, format, true)) return rc;
  const Shape s = unsharp_shape(Shape{nullptr, sizes, orientations, nullptr, nullptr, colour, colour_per_frame, depth}, unsharp, unsharp_per_frame);
  if (depth == nullptr) {
    return shape_body<UnsharpKind<YuvColourKind>>(who, w, e, format, nframes, frames, s, false, d_out, out_bytes, out_frames, nullptr, out_format,
                                                  stream);
  }
  if (int rc = yuv_depth_check(who, depth)) return rc;
  return shape_body<UnsharpKind<YuvDeepKind>>(who, w, e, format, nframes, frames, s, false, d_out, out_bytes, out_frames, nullptr, out_format,
                                              stream);
}

int sjpeg_hip_encode_ragged_yuv_unsharp_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                            const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                            const sjpeg_hip_yuv_colour* colour, int colour_per_frame, const sjpeg_hip_yuv_depth* depth,
                                            const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, const sjpeg_hip_metadata* meta,
                                            int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                            void* stream) {
  return yuv_unsharp_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                            {d_out, d_sizes, modes, q_out, value_out, stream}}, sizes, orientations, colour, colour_per_frame, depth, unsharp,
                           unsharp_per_frame);
}

int sjpeg_hip_encode_ragged_yuv_unsharp_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                   const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2], const uint8_t* orientations,
                                                   const sjpeg_hip_yuv_colour* colour, int colour_per_frame, const sjpeg_hip_yuv_depth* depth,
                                                   const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, const sjpeg_hip_metadata* meta,
                                                   int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets,
                                                   uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return yuv_unsharp_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                            RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, sizes,
                           orientations, colour, colour_per_frame, depth, unsharp, unsharp_per_frame);
}

// ---- ... and resampling with Pillow's filters: box, bilinear, Hamming, bicubic and Lanczos windows, enlarging too; ONE
// launch of a kernel of its own (resample.hip), optionally the unsharp launch behind it
int sjpeg_hip_resample_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                  const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations,
                                  const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_unsharp* unsharp,
                                  int unsharp_per_frame, void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* out_frames, int* out_format,
                                  void* stream) {
  static const std::string who = "sjpeg_hip_resample_ragged_src";
  static constexpr ShapeWords w = {kOrientWords.pointers, "d_out", "bytes", "resampled pictures", "sjpeg_hip_resample_ragged_bytes"};
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (resample == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": resample == NULL");
  const Shape s = resample_shape(sizes, orientations, flatten, resample, resample_per_frame, unsharp, unsharp_per_frame);
  if (nothing_to_sharpen(nframes, unsharp, unsharp_per_frame)) {
    return shape_body<ResampleKind>(who, w, e, format, nframes, frames, s, false, d_out, out_bytes, out_frames, nullptr, out_format, stream);
  }
  return shape_body<UnsharpKind<ResampleKind>>(who, w, e, format, nframes, frames, s, false, d_out, out_bytes, out_frames, nullptr, out_format,
                                               stream);
}

int sjpeg_hip_encode_ragged_resampled_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                          const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                          const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame,
                                          const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, const sjpeg_hip_metadata* meta,
                                          int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                          void* stream) {
  return resampled_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                          {d_out, d_sizes, modes, q_out, value_out, stream}}, flatten, sizes, orientations, resample, resample_per_frame, unsharp,
                         unsharp_per_frame);
}

int sjpeg_hip_encode_ragged_resampled_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                 const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten,
                                                 const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_resample* resample,
                                                 int resample_per_frame, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame,
                                                 const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_packed, size_t packed_capacity,
                                                 uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                                 void* stream) {
  return resampled_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                          RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, flatten, sizes,
                         orientations, resample, resample_per_frame, unsharp, unsharp_per_frame);
}

// ---- ... from a source box and behind a reduce: Image.thumbnail and ImageOps.fit
int sjpeg_hip_resample_box_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                      const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations,
                                      const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_resample_box* box,
                                      int box_per_frame, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, void* d_out, size_t out_bytes,
                                      sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_resample_box_ragged_src";
  static constexpr ShapeWords w = {kOrientWords.pointers, "d_out", "bytes", "resampled pictures", "sjpeg_hip_resample_box_ragged_bytes"};
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (resample == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": resample == NULL");
  if (box == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": box == NULL");
  Shape s = resample_shape(sizes, orientations, flatten, resample, resample_per_frame, unsharp, unsharp_per_frame);
  s.box = box; s.box_per_frame = box_per_frame;
  if (nothing_to_sharpen(nframes, unsharp, unsharp_per_frame)) {
    return shape_body<ResampleBoxKind>(who, w, e, format, nframes, frames, s, false, d_out, out_bytes, out_frames, nullptr, out_format, stream);
  }
  return shape_body<UnsharpKind<ResampleBoxKind>>(who, w, e, format, nframes, frames, s, false, d_out, out_bytes, out_frames, nullptr, out_format,
                                                  stream);
}

int sjpeg_hip_encode_ragged_resampled_box_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                              const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                              const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame,
                                              const sjpeg_hip_resample_box* box, int box_per_frame, const sjpeg_hip_unsharp* unsharp,
                                              int unsharp_per_frame, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out,
                                              uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return resampled_box_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                              {d_out, d_sizes, modes, q_out, value_out, stream}}, flatten, sizes, orientations, resample, resample_per_frame, box,
                             box_per_frame, unsharp, unsharp_per_frame);
}

int sjpeg_hip_encode_ragged_resampled_box_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                     const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten,
                                                     const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_resample* resample,
                                                     int resample_per_frame, const sjpeg_hip_resample_box* box, int box_per_frame,
                                                     const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, const sjpeg_hip_metadata* meta,
                                                     int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets,
                                                     uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return resampled_box_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                              RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, flatten,
                             sizes, orientations, resample, resample_per_frame, box, box_per_frame, unsharp, unsharp_per_frame);
}

// ---- ... and filtered by Pillow's BoxBlur, GaussianBlur or UnsharpMask behind it: two launches (pillow_filter.hip)
int sjpeg_hip_filter_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations,
                                const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_resample_box* box, int box_per_frame,
                                const sjpeg_hip_pillow_filter* filter, int filter_per_frame, void* d_out, size_t out_bytes,
                                sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_filter_ragged_src";
  static constexpr ShapeWords w = {kOrientWords.pointers, "d_out", "bytes", "filtered pictures", "sjpeg_hip_resample_box_ragged_bytes"};
  if (nothing_to_filter(nframes, filter, filter_per_frame)) {
    return sjpeg_hip_resample_box_ragged_src(e, format, nframes, frames, flatten, sizes, orientations, resample, resample_per_frame, box,
                                             box_per_frame, nullptr, 0, d_out, out_bytes, out_frames, out_format, stream);
  }
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (resample == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": resample == NULL");
  if (box == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": box == NULL");
  Shape s = resample_shape(sizes, orientations, flatten, resample, resample_per_frame, nullptr, 0);
  s.box = box; s.box_per_frame = box_per_frame;
  s.filter = filter; s.filter_per_frame = filter_per_frame;
  return shape_body<FilterKind<ResampleBoxKind>>(who, w, e, format, nframes, frames, s, false, d_out, out_bytes, out_frames, nullptr, out_format,
                                                 stream);
}

int sjpeg_hip_encode_ragged_filtered_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                         const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                         const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame,
                                         const sjpeg_hip_resample_box* box, int box_per_frame, const sjpeg_hip_pillow_filter* filter,
                                         int filter_per_frame, const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out,
                                         uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return filtered_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                         {d_out, d_sizes, modes, q_out, value_out, stream}}, flatten, sizes, orientations, resample, resample_per_frame, box,
                        box_per_frame, filter, filter_per_frame);
}

int sjpeg_hip_encode_ragged_filtered_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten,
                                                const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_resample* resample,
                                                int resample_per_frame, const sjpeg_hip_resample_box* box, int box_per_frame,
                                                const sjpeg_hip_pillow_filter* filter, int filter_per_frame, const sjpeg_hip_metadata* meta,
                                                int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets,
                                                uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return filtered_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                         RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, flatten,
                        sizes, orientations, resample, resample_per_frame, box, box_per_frame, filter, filter_per_frame);
}

// ---- ... and composed behind that: a canvas and overlays by one launch (compose.hip)
size_t sjpeg_hip_compose_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                                      const uint8_t* orientations, const sjpeg_hip_resample_box* box, int box_per_frame,
                                      const sjpeg_hip_compose* compose, int compose_per_frame) {
  if (frames == nullptr || box == nullptr || nframes < 1 || nframes > 65535) return 0;
  try {
    // (the layout depends on neither the filter nor the overlays: the places are counted, not read)
    const sjpeg_hip_resample filter = {SJPEG_HIP_RESAMPLE_BOX, {0, 0, 0}};
    Shape s = resample_shape(sizes, orientations, nullptr, &filter, 0, nullptr, 0);
    s.box = box; s.box_per_frame = box_per_frame;
    std::vector<sjpeg_hip_compose> bare;
    if (compose != nullptr) {
      bare.assign(compose, compose + (compose_per_frame != 0 ? nframes : 1));
      for (sjpeg_hip_compose& c : bare) {
        if (c.nplaces < 0 || c.nplaces > kComposePlacesMax || c.first_place < 0) return 0;
        c.first_place = 0; c.nplaces = 0;
      }
      s.compose = bare.data(); s.compose_per_frame = compose_per_frame;
    }
    ComposeKind<ResampleBoxKind>::Plan plan;
    if (ComposeKind<ResampleBoxKind>::plan("sjpeg_hip_compose_ragged_bytes", format, nframes, frames, s, &plan) != 0) return 0;
    return plan.bytes;
  } catch (...) {
    return 0;
  }
}

int sjpeg_hip_compose_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                 const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2], const uint8_t* orientations,
                                 const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_resample_box* box, int box_per_frame,
                                 const sjpeg_hip_pillow_filter* filter, int filter_per_frame, const sjpeg_hip_compose* compose,
                                 int compose_per_frame, const sjpeg_hip_overlay* overlays, int noverlays, const sjpeg_hip_overlay_place* places,
                                 int nplaces, void* d_out, size_t out_bytes, sjpeg_hip_ragged_frame* out_frames, int* out_format, void* stream) {
  static const std::string who = "sjpeg_hip_compose_ragged_src";
  static constexpr ShapeWords w = {kOrientWords.pointers, "d_out", "bytes", "composed pictures", "sjpeg_hip_compose_ragged_bytes"};
  const ComposeArgs a = {compose, compose_per_frame, overlays, noverlays, places, nplaces};
  if (nothing_to_compose(format, nframes, frames, sizes, orientations, resample, resample_per_frame, box, box_per_frame, flatten, a)) {
    return sjpeg_hip_filter_ragged_src(e, format, nframes, frames, flatten, sizes, orientations, resample, resample_per_frame, box, box_per_frame,
                                       filter, filter_per_frame, d_out, out_bytes, out_frames, out_format, stream);
  }
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (resample == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": resample == NULL");
  if (box == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": box == NULL");
  const Shape s = composed_shape(flatten, sizes, orientations, resample, resample_per_frame, box, box_per_frame, filter, filter_per_frame, a);
  if (nothing_to_filter(nframes, filter, filter_per_frame)) {
    return shape_body<ComposeKind<ResampleBoxKind>>(who, w, e, format, nframes, frames, s, false, d_out, out_bytes, out_frames, nullptr,
                                                    out_format, stream);
  }
  return shape_body<ComposeKind<FilterKind<ResampleBoxKind>>>(who, w, e, format, nframes, frames, s, false, d_out, out_bytes, out_frames, nullptr,
                                                              out_format, stream);
}

int sjpeg_hip_encode_ragged_composed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                         const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2],
                                         const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame,
                                         const sjpeg_hip_resample_box* box, int box_per_frame, const sjpeg_hip_pillow_filter* filter,
                                         int filter_per_frame, const sjpeg_hip_compose* compose, int compose_per_frame,
                                         const sjpeg_hip_overlay* overlays, int noverlays, const sjpeg_hip_overlay_place* places, int nplaces,
                                         const sjpeg_hip_metadata* meta, int meta_per_frame, void* d_out, uint64_t* d_sizes, int* modes,
                                         float* q_out, float* value_out, void* stream) {
  return composed_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                         {d_out, d_sizes, modes, q_out, value_out, stream}}, flatten, sizes, orientations, resample, resample_per_frame, box,
                        box_per_frame, filter, filter_per_frame, {compose, compose_per_frame, overlays, noverlays, places, nplaces});
}

int sjpeg_hip_encode_ragged_composed_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten,
                                                const int32_t (*sizes)[2], const uint8_t* orientations, const sjpeg_hip_resample* resample,
                                                int resample_per_frame, const sjpeg_hip_resample_box* box, int box_per_frame,
                                                const sjpeg_hip_pillow_filter* filter, int filter_per_frame, const sjpeg_hip_compose* compose,
                                                int compose_per_frame, const sjpeg_hip_overlay* overlays, int noverlays,
                                                const sjpeg_hip_overlay_place* places, int nplaces, const sjpeg_hip_metadata* meta,
                                                int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets,
                                                uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return composed_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                         RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)}, flatten,
                        sizes, orientations, resample, resample_per_frame, box, box_per_frame, filter, filter_per_frame,
                        {compose, compose_per_frame, overlays, noverlays, places, nplaces});
}

}  // extern "C"
