// source_layout.h -- what a source format (SJPEG_HIP_SRC_*, include/sjpeg_hip.h) IS, stated once: one row a format,
// and the few functions that every entry point reads it through -- the engine's uniform and ragged entries
// (scan_engine.hip), the riskiness and the sharp conversion (riskiness.hip, sharp_yuv.hip), the search (ragged_full.cc)
// and the host API (host_api.cc).  Host side, internal: not part of include/sjpeg_hip.h.  DESIGN.md, "adding a source
// format", lists what else a new format touches.
#ifndef SJPEG_AMD_SOURCE_LAYOUT_H_
#define SJPEG_AMD_SOURCE_LAYOUT_H_

#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <string>

#include "pixel_elem.h"
#include "sjpeg_hip.h"

namespace sjpeg_internal {

// source classes the scan kernels' colour phase is specialised for (scan_device.h says what each one reads)
enum { kSrcRgb24 = 0, kSrcRgbx32 = 1, kSrcPlanes = 2, kSrcRgbPlanar = 3, kSrcRgbPlanarF = 4 };

struct SourceLayout {
  int format;                  // SJPEG_HIP_SRC_*: the row's place in the table
  int cls;                     // kSrc*
  int planes;                  // how many of the caller's planes are read (1, 2 or 3)
  int implied;                 // the SJPEG_HIP_YUV* the format implies, or 0: any of the three
  int kind, esz;               // kElem* (pixel_elem.h) and its size in bytes
  // a row of plane i: `step` elements from a pixel to the next, the first `read` of a pixel's elements are read, over
  // the picture's width or (chroma) over (width + 1) / 2 -- row_bytes() below
  struct Plane { int step, read, chroma; } plane[3];
  // the RGB-like formats: bytes from a pixel to the next and where R, G and B lie inside plane[0] (one_pitch: G and B
  // are planes of their own, layout_rgb_offsets)
  int pix_step, r_off, g_off, b_off;
  bool one_pitch;              // planar RGB, bytes or floats: one pitch, three bases (sjpeg_hip.h)
  bool rgb_like;               // taken by SJPEG_YUV_AUTO, SJPEG_YUV_SHARP, the riskiness and the sharp conversion
  // the scan kernels' per-format fields (ScanArgs, scan_device.h)
  int rsh, bsh, cstep, uoff, voff, pstep, pone;
};

namespace layout_rows {
constexpr int k420 = SJPEG_HIP_YUV420, k444 = SJPEG_HIP_YUV444, k400 = SJPEG_HIP_YUV400;
constexpr int elem_size(int kind) { return kind == kElemF32 ? 4 : kind == kElemU8 ? 1 : 2; }
constexpr SourceLayout::Plane kFull = {1, 1, 0}, kHalf = {1, 1, 1}, kNone = {0, 0, 0};
// packed bytes: `step` bytes a pixel, all of them read; R at byte r_off, B at byte b_off
constexpr SourceLayout packed(int format, int cls, int step, int r_off, int b_off, int rsh, int bsh) {
  return {format, cls, 1, 0, kElemU8, 1, {{step, step, 0}, kNone, kNone}, step, r_off, 1, b_off, false, true, rsh, bsh, 0, 0, 0, 0, 0};
}
// Y, U, V (or gray) planes of bytes
constexpr SourceLayout yuv(int format, int planes, int implied, SourceLayout::Plane chroma, int cstep, int uoff, int voff) {
  return {format, kSrcPlanes, planes, implied, kElemU8, 1, {kFull, planes > 1 ? chroma : kNone, planes > 2 ? chroma : kNone},
          0, 0, 0, 0, false, false, 0, 0, cstep, uoff, voff, 0, 0};
}
// R, G, B planes of one pitch
constexpr SourceLayout planar_rgb(int format, int cls, int kind) {
  return {format, cls, 3, 0, kind, elem_size(kind), {kFull, kFull, kFull}, elem_size(kind), 0, 0, 0, true, true,
          0, 0, 0, 0, 0, kind == kElemU8 ? 0 : 1, 0};
}
// one plane of float pixels: `step` elements a pixel, the first `read` of them read (R, G, B or the gray value)
constexpr SourceLayout one_plane_float(int format, int kind, int step, int read) {
  return {format, kSrcRgbPlanarF, 1, read == 1 ? k400 : 0, kind, elem_size(kind), {{step, read, 0}, kNone, kNone},
          step * elem_size(kind), 0, read == 1 ? 0 : elem_size(kind), read == 1 ? 0 : 2 * elem_size(kind), false, read == 3,
          0, 0, 0, 0, 0, step, read == 1 ? 1 : 0};
}
}  // namespace layout_rows

constexpr int kSourceFormats = 21;
constexpr SourceLayout kSourceLayouts[kSourceFormats] = {
    layout_rows::packed(SJPEG_HIP_SRC_RGB, kSrcRgb24, 3, 0, 2, 0, 0),
    layout_rows::packed(SJPEG_HIP_SRC_BGRA, kSrcRgbx32, 4, 2, 0, 16, 0),
    layout_rows::packed(SJPEG_HIP_SRC_RGBA, kSrcRgbx32, 4, 0, 2, 0, 16),
    layout_rows::yuv(SJPEG_HIP_SRC_GRAY, 1, layout_rows::k400, layout_rows::kNone, 0, 0, 0),
    layout_rows::yuv(SJPEG_HIP_SRC_YUV444, 3, layout_rows::k444, layout_rows::kFull, 1, 0, 0),
    layout_rows::yuv(SJPEG_HIP_SRC_YUV420, 3, layout_rows::k420, layout_rows::kHalf, 1, 0, 0),
    layout_rows::yuv(SJPEG_HIP_SRC_NV12, 2, layout_rows::k420, {2, 2, 1}, 2, 0, 1),
    layout_rows::yuv(SJPEG_HIP_SRC_NV21, 2, layout_rows::k420, {2, 2, 1}, 2, 1, 0),
    layout_rows::planar_rgb(SJPEG_HIP_SRC_RGB_PLANAR, kSrcRgbPlanar, kElemU8),
    layout_rows::planar_rgb(SJPEG_HIP_SRC_RGB_PLANAR_F32, kSrcRgbPlanarF, kElemF32),
    layout_rows::planar_rgb(SJPEG_HIP_SRC_RGB_PLANAR_F16, kSrcRgbPlanarF, kElemF16),
    layout_rows::planar_rgb(SJPEG_HIP_SRC_RGB_PLANAR_BF16, kSrcRgbPlanarF, kElemBF16),
    layout_rows::one_plane_float(SJPEG_HIP_SRC_RGB_F32, kElemF32, 3, 3),
    layout_rows::one_plane_float(SJPEG_HIP_SRC_RGB_F16, kElemF16, 3, 3),
    layout_rows::one_plane_float(SJPEG_HIP_SRC_RGB_BF16, kElemBF16, 3, 3),
    layout_rows::one_plane_float(SJPEG_HIP_SRC_RGBA_F32, kElemF32, 4, 3),
    layout_rows::one_plane_float(SJPEG_HIP_SRC_RGBA_F16, kElemF16, 4, 3),
    layout_rows::one_plane_float(SJPEG_HIP_SRC_RGBA_BF16, kElemBF16, 4, 3),
    layout_rows::one_plane_float(SJPEG_HIP_SRC_GRAY_F32, kElemF32, 1, 1),
    layout_rows::one_plane_float(SJPEG_HIP_SRC_GRAY_F16, kElemF16, 1, 1),
    layout_rows::one_plane_float(SJPEG_HIP_SRC_GRAY_BF16, kElemBF16, 1, 1),
};
constexpr bool layouts_in_place(int i = 0) { return i == kSourceFormats || (kSourceLayouts[i].format == i && layouts_in_place(i + 1)); }
static_assert(layouts_in_place(), "kSourceLayouts: a row's place is its SJPEG_HIP_SRC_* value");

// the row of a format, or NULL for a value that is none
inline const SourceLayout* source_layout(int format) {
  return format >= 0 && format < kSourceFormats ? &kSourceLayouts[format] : nullptr;
}

// bytes of a row of plane i of a picture `width` pixels wide, up to the last element that is read
inline int64_t row_bytes(const SourceLayout& L, int i, int64_t width) {
  const int64_t w = L.plane[i].chroma ? (width + 1) / 2 : width;
  return ((w - 1) * L.plane[i].step + L.plane[i].read) * L.esz;
}

// The kernels' three planes out of the caller's (frame_stride and out_frame NULL: one picture, no frame strides).
// Interleaved chroma: U and V walk the same plane.  One plane of float pixels: G and B lie g_off and b_off behind R (gray:
// all three the same), one pitch.  A plane nothing reads: NULL, stride 0.  Strides of either sign go through as they are.
inline void layout_planes(const SourceLayout& L, const void* const* plane, const int64_t* row_stride, const int64_t* frame_stride,
                          const uint8_t** out_plane, long long* out_row, long long* out_frame) {
  const bool one_float_plane = L.cls == kSrcRgbPlanarF && L.planes == 1;
  const int add[3] = {0, one_float_plane ? L.g_off : 0, one_float_plane ? L.b_off : 0};
  for (int i = 0; i < 3; ++i) {
    const int p = i < L.planes ? i : L.planes == 2 ? 1 : one_float_plane ? 0 : -1;
    out_plane[i] = p < 0 ? nullptr : static_cast<const uint8_t*>(plane[p]) + add[i];
    out_row[i] = p < 0 ? 0 : row_stride[p];
    if (out_frame != nullptr) out_frame[i] = p < 0 ? 0 : frame_stride[p];
  }
}

// where G and B of an RGB-like picture lie from its R, in bytes: inside the pixel, or (one_pitch) the distances of its G
// and B planes from its R plane -- hence 64 bits
inline void layout_rgb_offsets(const SourceLayout& L, const void* const* plane, long long* g_off, long long* b_off) {
  *g_off = L.one_pitch ? static_cast<const uint8_t*>(plane[1]) - static_cast<const uint8_t*>(plane[0]) : L.g_off;
  *b_off = L.one_pitch ? static_cast<const uint8_t*>(plane[2]) - static_cast<const uint8_t*>(plane[0]) : L.b_off;
}

// ---- the rules a picture's planes and strides keep, and the one routine that checks them
// (a NULL plane; a row stride below row_bytes(); one_pitch: a row / frame stride that is not plane 0's; float elements:
// a plane, row stride or frame stride off the element size)
enum { kFaultNone = 0, kFaultNullPlane, kFaultShortRow, kFaultRowPitch, kFaultFramePitch, kFaultElemPlane, kFaultElemRow, kFaultElemFrame };
struct LayoutFault { int rule, index; };

// The order a caller's checks come in decides which of two broken rules its message names, so each keeps its own:
// the uniform entries' (prepare_scan: planes, then pitches, then elements), the ragged entries' (ragged_frames: a
// plane's pitch right behind its row) and the ragged sharp conversion's (plane 0, then the other planes' pitches --
// their rows are as long as plane 0's by then).  A step that does not apply to the layout or the call is skipped.
constexpr LayoutFault kUniformChecks[] = {{kFaultNullPlane, 0}, {kFaultShortRow, 0}, {kFaultNullPlane, 1}, {kFaultShortRow, 1}, {kFaultNullPlane, 2},
                                          {kFaultShortRow, 2}, {kFaultRowPitch, 1}, {kFaultFramePitch, 1}, {kFaultRowPitch, 2}, {kFaultFramePitch, 2}};
constexpr LayoutFault kRaggedChecks[] = {{kFaultNullPlane, 0}, {kFaultShortRow, 0}, {kFaultNullPlane, 1}, {kFaultShortRow, 1}, {kFaultRowPitch, 1},
                                         {kFaultNullPlane, 2}, {kFaultShortRow, 2}, {kFaultRowPitch, 2}};
constexpr LayoutFault kSharpChecks[] = {{kFaultNullPlane, 0}, {kFaultShortRow, 0}, {kFaultNullPlane, 1}, {kFaultNullPlane, 2}, {kFaultRowPitch, 1},
                                        {kFaultRowPitch, 2}};

inline bool layout_rule_broken(const SourceLayout& L, int64_t width, const void* const* plane, const int64_t* row_stride,
                               const int64_t* frame_stride, LayoutFault c) {
  const int i = c.index;
  if (i >= L.planes) return false;
  switch (c.rule) {
    case kFaultNullPlane: return plane[i] == nullptr;
    case kFaultShortRow: return (row_stride[i] < 0 ? -row_stride[i] : row_stride[i]) < row_bytes(L, i, width);
    case kFaultRowPitch: return L.one_pitch && row_stride[i] != row_stride[0];
    case kFaultFramePitch: return L.one_pitch && frame_stride != nullptr && frame_stride[i] != frame_stride[0];
    case kFaultElemPlane: return reinterpret_cast<uintptr_t>(plane[i]) % static_cast<uintptr_t>(L.esz) != 0;
    case kFaultElemRow: return row_stride[i] % L.esz != 0;
    case kFaultElemFrame: return frame_stride != nullptr && frame_stride[i] % L.esz != 0;
    default: return false;
  }
}

// The first rule that one picture's planes and strides break (frame_stride: a uniform batch's, or NULL), checked in
// the order of `checks` and then element by element; {kFaultNone, 0} when they are in order.
template <size_t N>
inline LayoutFault layout_fault(const SourceLayout& L, int64_t width, const void* const* plane, const int64_t* row_stride,
                                const int64_t* frame_stride, const LayoutFault (&checks)[N]) {
  for (const LayoutFault& c : checks) {
    if (layout_rule_broken(L, width, plane, row_stride, frame_stride, c)) return c;
  }
  for (int i = 0; i < 3; ++i) {
    for (int rule : {kFaultElemPlane, kFaultElemRow, kFaultElemFrame}) {
      if (layout_rule_broken(L, width, plane, row_stride, frame_stride, {rule, i})) return {rule, i};
    }
  }
  return {kFaultNone, 0};
}

// a fault in the words of the ragged entries (they put "<entry>: frame <f>: " in front)
inline std::string layout_fault_text(const SourceLayout& L, LayoutFault f) {
  const std::string i = "[" + std::to_string(f.index) + "]";
  const std::string tail = " must be a multiple of the element size (" + std::to_string(L.esz) + " bytes)";
  switch (f.rule) {
    case kFaultNullPlane: return "null plane pointer";
    case kFaultShortRow: return "|row_stride| smaller than a row of the plane";
    case kFaultRowPitch: return "row_stride" + i + " must equal row_stride[0] (SJPEG_HIP_SRC_RGB_PLANAR)";
    case kFaultFramePitch: return "frame_stride" + i + " must equal frame_stride[0] (SJPEG_HIP_SRC_RGB_PLANAR)";
    case kFaultElemPlane: return "plane" + i + tail;
    case kFaultElemRow: return "row_stride" + i + tail;
    case kFaultElemFrame: return "frame_stride" + i + tail;
    default: return std::string();
  }
}

}  // namespace sjpeg_internal

#endif  // SJPEG_AMD_SOURCE_LAYOUT_H_
