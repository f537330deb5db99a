// ragged_aux.h -- what the ragged riskiness and sharp conversions (riskiness.hip, sharp_yuv.hip), the picture-making
// kernels and their plans, and the search (ragged_full.cc) share with the engine's ragged launch layer (scan_engine.hip)
// and the flows over it (ragged_flows.cc, engine_pictures.cc).  Internal: not part of include/sjpeg_hip.h.  The files
// that need the engine object itself include engine.h, which includes this.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "compose_math.h"
#include "jpeg_host.h"
#include "pillow_filter_math.h"
#include "pixel_elem.h"
#include "sjpeg_hip.h"
#include "source_layout.h"
#include "yuv_colour_math.h"

namespace sjpeg_internal {

// ---- sizes and mode helpers the ragged flows share (ragged_flows.cc, ragged_full.cc)
// a frame's share of device scratch: its kept histogram, its adaptation sums and totals (adapt_sums_kernel: [2][64]
// [deltas][2] int64, [2][64][2] int32), its symbol counts; a segment's partial of the statistics pass and its kept blocks
// (9 rows of 16 bytes for each of the workgroup's 256 threads), a persistent group's partial of the histogram pass (16-bit
// counters [2][64][128]): scan_engine.hip asserts the three against the kernels' constants
constexpr size_t kHist = 2 * 64 * 128 * sizeof(uint32_t);
constexpr size_t kSums = 2 * 64 * sjpeg_host::kAdaptDeltas * 2 * sizeof(int64_t), kTot = 2 * 64 * 2 * sizeof(int32_t);
constexpr size_t kFreq = 2 * 272 * sizeof(uint32_t), kStatsPartial = kFreq;
constexpr size_t kKeptSegBytes = 256 * 9 * 16, kHistPartial = 2 * 64 * 128 * sizeof(uint16_t);

// SjpegYUVMode (include/sjpeg.h); 1, 3 and 4 are SJPEG_HIP_YUV420 / 444 / 400
enum { kYuvAuto = 0, kYuv420 = 1, kYuvSharp = 2, kYuv444 = 3, kYuv400 = 4 };
// The mode groups of a call, in the order they are coded: 4:2:0, 4:4:4, 4:0:0 of the caller's format, then the sharp
// frames as planar 4:2:0.  What a group's frames are read as, and the sampling a frame of a mode is coded with:
constexpr int kGroupKinds[4] = {kYuv420, kYuv444, kYuv400, kYuvSharp};
inline int group_format(int kind, int format) { return kind == kYuvSharp ? SJPEG_HIP_SRC_YUV420 : format; }
inline int hip_yuv_mode(int mode) { return mode == kYuv444 ? SJPEG_HIP_YUV444 : mode == kYuv400 ? SJPEG_HIP_YUV400 : SJPEG_HIP_YUV420; }

inline size_t align16(size_t n) { return (n + 15) & ~size_t(15); }
// the planar 4:2:0 planes of a sharp frame: Y, U, V, each at a multiple of 16
inline size_t planes_bytes(const sjpeg_hip_ragged_frame& fr) {
  const size_t cw = (static_cast<size_t>(fr.width) + 1) / 2, ch = (static_cast<size_t>(fr.height) + 1) / 2;
  return align16(static_cast<size_t>(fr.width) * fr.height) + 2 * align16(cw * ch);
}
// The sharp frames of a part in an arena: the planes of frame after frame tightly packed, then the workspace.  planar[k]
// becomes sharp[k] read as planar 4:2:0 from there (plane[0..2], row_stride[0..2]), yuv[c][k] its plane c; returns where
// the workspace starts.
inline uint8_t* place_sharp_planes(uint8_t* arena, const std::vector<sjpeg_hip_ragged_frame>& sharp,
                                   std::vector<sjpeg_hip_ragged_frame>* planar, std::vector<uint8_t*> yuv[3]) {
  uint8_t* at = arena;
  *planar = sharp;
  for (sjpeg_hip_ragged_frame& fr : *planar) {
    const size_t cw = (static_cast<size_t>(fr.width) + 1) / 2, ch = (static_cast<size_t>(fr.height) + 1) / 2;
    const size_t bytes[3] = {static_cast<size_t>(fr.width) * fr.height, cw * ch, cw * ch};
    for (int c = 0; c < 3; ++c) {
      yuv[c].push_back(at);
      fr.plane[c] = at;
      fr.row_stride[c] = static_cast<int64_t>(c == 0 ? fr.width : cw);
      at += align16(bytes[c]);
    }
  }
  return at;
}

// ---- ragged riskiness: one descriptor per frame; a workgroup finds its frame by a binary search over wg_base
struct RiskFrame {
  const uint8_t* rgb;                    // row 0
  long long row_stride;                  // may be negative
  int W, H;
  int bands, cols;                       // the frame's workgroups: cols x bands (none when W or H < 2)
  unsigned wg_base, pad;                 // its first workgroup in the flat grid
  long long g_off, b_off;                // where G and B lie from R (layout_rgb_offsets)
};

// the frame's workgroups: bands of at least 16 rows, at most 64 of them; 256 columns each
inline void risk_frame_plan(int W, int H, RiskFrame* d) {
  d->W = W; d->H = H;
  if (W < 2 || H < 2) { d->bands = d->cols = 0; return; }
  const int rows = H - 1;
  d->bands = rows / 16 < 1 ? 1 : rows / 16 > 64 ? 64 : rows / 16;
  d->cols = (W - 1 + 255) / 256;
}

// d_sums[nframes][3] zeroed, then the flat grid of total_wgs workgroups over d_frames[nframes] (device memory)
// (pscale[3], pbias[3]: the engine's pixel transform per channel, read by the float formats alone)
int risk_ragged_launch(int format, const float* pscale, const float* pbias, const RiskFrame* d_frames, int nframes, unsigned total_wgs,
                       const uint8_t* d_table, uint64_t* d_sums, hipStream_t st);

// ---- ragged sharp conversion (sjpeg_hip_sharp_yuv_ragged); the descriptors go into the workspace through `up`
using UploadFn = int (*)(void* ctx, void* d_dst, const void* src, size_t bytes, hipStream_t st);
size_t sharp_ragged_workspace(int nframes, const sjpeg_hip_ragged_frame* frames);
int sharp_ragged_run(int format, const float* pscale, const float* pbias, int nframes, const sjpeg_hip_ragged_frame* frames, uint8_t* const* d_y,
                     uint8_t* const* d_u, uint8_t* const* d_v, void* d_workspace, size_t workspace_size,
                     hipStream_t st, UploadFn up, void* up_ctx, std::string* err);

// ---- ragged reduction (sjpeg_hip_reduce_ragged_src, reduce.hip): one descriptor per frame; a workgroup finds its frame
// by a binary search over tile_base.  A tile is 256 consecutive GROUPS of the frame in row-major order, a group four
// reduced pixels side by side (12 bytes of interleaved RGB, or 4 of gray: whole dwords of the reduced row).
struct ReduceFrame {
  const uint8_t* src;                    // plane 0, row 0
  long long row_stride;                  // may be negative
  long long off[3];                      // where R, G and B (gray: the value, thrice) lie from src (layout_rgb_offsets)
  uint8_t* dst;                          // the reduced picture: a multiple of 16
  int W, H, w2, h2;                      // the source's and the reduced picture's size
  int s, groups;                         // the factor; groups a reduced row: (w2 + 3) / 4
  unsigned dst_stride, tile_base;        // bytes between reduced rows; the frame's first workgroup in the flat grid
};
// A batch's reduction planned on the host, before any device work: the descriptors (dst: the picture's place from the
// buffer's start), the reduced format (SJPEG_HIP_SRC_RGB or _GRAY), the bytes the pictures take and the grid.
struct ReducePlan {
  int format = 0, reduced_format = 0;
  std::vector<ReduceFrame> frames;
  size_t bytes = 0;
  unsigned tiles = 0;
};
// Checks the format (an RGB-like or gray one) and the factors (1..8 each; NULL: all 1), then plans; the message names
// the frame.  The frames' planes and strides are the caller's to check (ragged_check).
int reduce_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const uint8_t* factors,
                ReducePlan* plan);
// the reduced pictures as frames of plan.reduced_format at `base` (out_offset / out_capacity: the source frames')
void reduce_plan_frames(const ReducePlan& plan, const sjpeg_hip_ragged_frame* frames, uint8_t* base, sjpeg_hip_ragged_frame* out);
// the flat grid over d_frames[nframes] (device memory, dst already absolute)
int reduce_ragged_launch(int format, const float* pscale, const float* pbias, const ReduceFrame* d_frames, int nframes, unsigned tiles,
                         hipStream_t st);
// The engine's half (engine_pictures.cc): the call ordered behind the engine's earlier work, the descriptors uploaded, the
// kernel launched on `stream`.  d_reduced == NULL: into the engine's own memory for reduced pictures -- one allocation
// of plan.bytes, apart from the arena of the sharp planes, counted by sjpeg_hip_engine_scratch_bytes and released by
// sjpeg_hip_engine_trim; *base says where.
int engine_reduce(sjpeg_hip_engine* e, const std::string& who, const ReducePlan& plan, uint8_t* d_reduced, uint8_t** base, void* stream);

// ---- ragged resize (sjpeg_hip_resize_ragged_src, resize.hip): one descriptor per frame; a workgroup finds its frame by
// a binary search over tile_base.  A tile is tw x th samples of the resized picture (tw a power of two in 4..256: a
// tile's row starts at a whole dword of the resized row), the frame's tiles in row-major order; 256 / tw lanes share a
// column of it.  The resized pictures lie in their buffer as the reduced ones do (reduce_round.h).
struct ResizeFrame {
  const uint8_t* src;                    // plane 0, row 0
  long long row_stride;                  // may be negative
  long long off[3];                      // where R, G and B (gray: the value, thrice) lie from src (layout_rgb_offsets)
  uint8_t* dst;                          // the resized picture: a multiple of 16
  int W, H, w2, h2;                      // the source's and the resized picture's size
  int tw, th;                            // the tile
  unsigned tiles_x, dst_stride;          // tiles a row of tiles; bytes between resized rows
  unsigned tile_base, orient;            // the frame's first workgroup in the flat grid; its EXIF orientation, 1..8
};
// The tile of a picture W x H -> w2 x h2 (set in d): P lanes a column, the largest power of two up to 64 that W / w'
// holds, so that a lane has about one source pixel a row; th: about 64 source rows a tile, so that the row two tiles
// share is one in 64.  Returns the picture's tiles.
inline unsigned long long resize_tile_rule(ResizeFrame* d) {
  int P = 1;
  while (P < 64 && 2 * P <= d->W / d->w2) P *= 2;
  d->tw = 256 / P;
  const int th = static_cast<int>((64ll * d->h2 + d->H - 1) / d->H);
  d->th = th < 1 ? 1 : th > 16 ? 16 : th;
  d->tiles_x = static_cast<unsigned>((d->w2 + d->tw - 1) / d->tw);
  return static_cast<unsigned long long>(d->tiles_x) * static_cast<unsigned long long>((d->h2 + d->th - 1) / d->th);
}
struct ResizePlan {
  int format = 0, resized_format = 0;
  std::vector<ResizeFrame> frames;
  size_t bytes = 0;
  unsigned tiles = 0;
  bool flat = false;                     // the frames are flattened as they are staged (the kernel's flat instantiations)
  sjpeg_hip_flatten flatten = {};        // ... by this
  int light = 0;                         // SJPEG_HIP_LIGHT_*: other than CODED, the kernel's linear instantiations
};
// Checks the sizes (sizes[f] = (w', h'), 1..the source's each; NULL: every frame at its own size) and the format (an
// RGB-like or gray one), then plans; the message names the frame.  The frames' planes and strides are the caller's to
// check (ragged_check).  orientations (NULL: all 1): each 1..8, checked with the sizes; the picture in the buffer is
// then the upright one of orient_math.h -- h' x w' for 5..8 --, and resize_plan_frames reports that size.  An
// orientation other than 1 takes a format the kernel reads, as a size other than the source's does.
// flatten (NULL: none): checked by flatten_check in front of the frames; every frame's row must then hold its last
// alpha element (the message names the frame and "alpha"); the plan is marked flat -- an alpha format under flatten
// goes through the kernel at any size and orientation, its resized format is SJPEG_HIP_SRC_RGB.
int resize_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                const uint8_t* orientations, ResizePlan* plan, const sjpeg_hip_flatten* flatten = nullptr);
// 0 for a flatten the format takes, else SJPEG_HIP_EINVAL: a format without alpha (named), premultiplied above 1, a
// float format's alpha transform that is not finite
int flatten_check(const std::string& who, int format, const sjpeg_hip_flatten& flatten);
void resize_plan_frames(const ResizePlan& plan, const sjpeg_hip_ragged_frame* frames, uint8_t* base, sjpeg_hip_ragged_frame* out);
int resize_ragged_launch(int format, const float* pscale, const float* pbias, const ResizeFrame* d_frames, int nframes, unsigned tiles,
                         hipStream_t st);
// ... of a flat plan (placed: a sheet's descriptors)
int resize_ragged_flat_launch(bool placed, int format, const float* pscale, const float* pbias, const sjpeg_hip_flatten& flatten,
                              const ResizeFrame* d_frames, int nframes, unsigned tiles, hipStream_t st);
// ... of a plan in linear light (flatten NULL: not flat; placed: a sheet's descriptors)
int resize_ragged_linear_launch(bool placed, int format, const float* pscale, const float* pbias, const sjpeg_hip_flatten* flatten,
                                const ResizeFrame* d_frames, int nframes, unsigned tiles, hipStream_t st);
// 0 for a light the linear entries take and a format whose samples are RGB light, else SJPEG_HIP_EINVAL: a light that
// is not SJPEG_HIP_LIGHT_CODED or _LINEAR_SRGB, a YUV-plane format (named)
int light_check(const std::string& who, int light, int format);
// The engine's half (engine_pictures.cc), as engine_reduce: d_resized == NULL: into the engine's memory for reduced
// pictures (the two kinds of call share it and its descriptors' buffer).  A flat plan runs the flat launch, a plan in
// linear light the linear one.
int engine_resize(sjpeg_hip_engine* e, const std::string& who, const ResizePlan& plan, uint8_t* d_resized, uint8_t** base, void* stream);

// ---- ragged resize of the YUV-plane formats (sjpeg_hip_resize_ragged_yuv_src; yuv_resize_plan.cc, resize.hip): one
// descriptor per PLANE of a frame -- Y, U, V of the planar formats, each a one-channel picture of its own; Y and the
// UV plane of NV12 / NV21, a picture of two-byte pixels that is staged once and leaves as two planes.  The flat grid
// runs over the tiles of every plane of every frame; a workgroup finds its plane by the binary search over tile_base.
struct YuvPlane {
  ResizeFrame r;                         // the plane as a picture: W, H, w2, h2, the tile and dst_stride are the PLANE's
                                         // (channels == 2: off[0], off[1] say where U and V lie in a pair; dst is U's)
  uint8_t* dst2;                         // channels == 2: V's plane, laid out as U's
  int channels, frame;                   // 1 or 2; the frame the plane belongs to
};
struct YuvResizePlan {
  int format = 0, resized_format = 0;    // the caller's; SJPEG_HIP_SRC_YUV420 or _YUV444, always planar
  int nframes = 0;
  std::vector<YuvPlane> planes;          // frame after frame
  size_t bytes = 0;
  unsigned tiles = 0;
  bool deep = false;                     // the source planes hold 16-bit samples (the kernel's deep instantiations)
  unsigned shift = 0;                    // ... whose byte lies this many bits up (sjpeg_hip_yuv_depth)
};
// the size of plane 0..2 of a width x height picture of a YUV-plane format, as the encoder reads it
inline void yuv_plane_dims(const SourceLayout& L, int width, int height, int plane, int* pw, int* ph) {
  const bool half = plane > 0 && L.implied == SJPEG_HIP_YUV420;
  *pw = half ? (width + 1) / 2 : width;
  *ph = half ? (height + 1) / 2 : height;
}
// the format's name where it is one of the table, for the messages that refuse it
const char* source_format_name(int format);
// 0 for one of the four YUV-plane formats, else SJPEG_HIP_EINVAL: the format named, the entries that take it pointed at
int yuv_format_check(const std::string& who, int format);
// Checks the format (one of the four YUV-plane ones: anything else is refused by name), the sizes and the orientations
// as resize_plan does, then plans: every plane by resize_plan's tw / th rule, the planes of frame after frame Y, U, V
// in reduce_round.h's layout, each turned as a picture of its own.  The frames' planes and strides are the caller's to
// check (ragged_check).  depth (NULL: planes of bytes): checked by yuv_depth_check, then the plan is marked deep -- the
// descriptors are the same (a pair's off[] counts samples); the made planes are bytes, so layout and bytes are too.
int yuv_resize_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                    const uint8_t* orientations, YuvResizePlan* plan, const sjpeg_hip_yuv_depth* depth = nullptr);
// 0 for a depth the deep entries take, else SJPEG_HIP_EINVAL naming the field: depth == NULL, bytes other than 2, a
// shift above 8, a reserved byte that is not 0
int yuv_depth_check(const std::string& who, const sjpeg_hip_yuv_depth* depth);
// the made pictures as frames of plan.resized_format at `base`: three planes, their strides, the upright size
void yuv_resize_plan_frames(const YuvResizePlan& plan, const sjpeg_hip_ragged_frame* frames, uint8_t* base, sjpeg_hip_ragged_frame* out);
int yuv_resize_ragged_launch(const YuvPlane* d_planes, int nplanes, unsigned tiles, hipStream_t st);
// ... of a deep plan (placed: a sheet's descriptors)
int yuv_resize_ragged_deep_launch(bool placed, unsigned shift, const YuvPlane* d_planes, int nplanes, unsigned tiles, hipStream_t st);
// the engine's half, as engine_resize; a deep plan runs the deep launch
int engine_yuv_resize(sjpeg_hip_engine* e, const std::string& who, const YuvResizePlan& plan, uint8_t* d_out, uint8_t** base, void* stream);

// ---- contact sheets (sjpeg_hip_sheet_ragged_src; sheet_plan.cc, resize.hip): the thumbnails of the two plans above,
// each stored into its rectangle of a larger picture.  A PLACED descriptor's dst (and dst2) is the thumbnail's first
// sample inside its sheet plane and its dst_stride the sheet plane's; kResizePlaced in its `orient` says so.  The
// kernel's placed instantiations read such descriptors: every tile leaves by the exact-span store, whose phase comes
// from the address the span starts at.
constexpr unsigned kResizePlaced = 0x100u;
// The background of a call's sheets: sheet s at s * sheet_bytes from the buffer's start, its plane c `off[c]` behind
// that -- rows[c] rows of row_dwords[c] dwords, dword k of a row pattern[c][k % 3] (an RGB row: a 12-byte pattern
// whose phase restarts at each row; a one-byte plane: three equal dwords).
struct SheetFill {
  size_t sheet_bytes = 0;
  int nsheets = 0, nplanes = 0;          // 1 (interleaved RGB, gray) or 3 (Y, U, V)
  size_t off[3] = {0, 0, 0};
  unsigned rows[3] = {0, 0, 0}, row_dwords[3] = {0, 0, 0};
  uint32_t pattern[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
};
struct SheetPlace { int32_t sheet, x0, y0, uw, uh; };   // sjpeg_hip_sheet_places: the #xywh= numbers of a storyboard
struct SheetPlan {
  int format = 0, out_format = 0;        // the caller's; SJPEG_HIP_SRC_RGB, _GRAY, _YUV420 or _YUV444
  bool yuv = false;                      // which of the two plans holds the (placed) descriptors
  int nframes = 0, nsheets = 0, width = 0, height = 0;
  ResizePlan rgb;
  YuvResizePlan planes;
  std::vector<SheetPlace> places;        // [nframes]
  SheetFill fill;
  size_t bytes = 0;                      // nsheets * fill.sheet_bytes
};
// the sheet's fields checked for the format (ranges, `reserved`, the size, evenness for a 4:2:0 format: the field is
// named); its size
int sheet_check(const std::string& who, const sjpeg_hip_sheet* sheet, int format, int* width, int* height);
// The sheet checked, the thumbnails planned by resize_plan / yuv_resize_plan (sizes == NULL: each fitted into its
// cell) -- their checks, their tile rule, their descriptors --, every thumbnail held to its cell, then each descriptor
// rewritten to its place.  flatten (NULL: none): handed to resize_plan; a YUV-plane format has no alpha and is
// refused by name.
int sheet_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_sheet* sheet,
               const int32_t (*sizes)[2], const uint8_t* orientations, SheetPlan* plan, const sjpeg_hip_flatten* flatten = nullptr,
               const sjpeg_hip_yuv_depth* depth = nullptr);   // (depth: handed to yuv_resize_plan)
// the sheets as frames of plan.out_format at `base` (out_offset, out_capacity: 0)
void sheet_plan_frames(const SheetPlan& plan, uint8_t* base, sjpeg_hip_ragged_frame* out /*[nsheets]*/);
int sheet_fill_launch(const SheetFill& fill, uint8_t* base, hipStream_t st);
int resize_ragged_placed_launch(int format, const float* pscale, const float* pbias, const ResizeFrame* d_frames, int nframes, unsigned tiles,
                                hipStream_t st);
int yuv_resize_ragged_placed_launch(const YuvPlane* d_planes, int nplanes, unsigned tiles, hipStream_t st);
// the engine's half, as engine_resize: the background fill, then the placed resize, both on `stream`
int engine_sheet(sjpeg_hip_engine* e, const std::string& who, const SheetPlan& plan, uint8_t* d_out, uint8_t** base, void* stream);

// ---- video colour conversion (sjpeg_hip_convert_ragged_yuv_src; yuv_colour_plan.cc, yuv_colour.hip): the made planes
// of the YUV plan above, or the thumbnails' rectangles of a sheet, converted in place to JFIF's colour by ONE launch
// behind the resize launch.  One descriptor per frame; a workgroup finds its frame by the binary search over tile_base.
// A tile is 256 consecutive LANES of the frame in row-major order, a lane four chroma samples of a row -- one dword of
// U and one of V -- and the luma samples above them.  A frame with identity colour has no tiles.
struct YuvColourFrame {
  uint8_t *y, *u, *v;                    // the planes' first samples (a placed frame's: inside its sheet planes)
  unsigned y_stride, c_stride;           // bytes between the rows of Y, and of U and V
  int uw, uh, cw, ch;                    // the upright luma and chroma sizes
  int s;                                 // luma samples a chroma sample, each way: 2 (4:2:0) or 1 (4:4:4)
  int lead;                              // placed: the bytes from the dword boundary in front of u to u, 0..3 (else 0)
  unsigned groups, tile_base;            // lanes a chroma row; the frame's first workgroup in the flat grid
  YuvColourTable table;
};
struct YuvColourPlan {
  std::vector<YuvColourFrame> frames;    // [nframes]; y, u, v from the buffer's start, as the plans count
  unsigned tiles = 0;
  bool placed = false;                   // the frames are a sheet's thumbnails: only their own bytes are stored
};
// 0 for colours the entries take (NULL: none to check), else SJPEG_HIP_EINVAL: a matrix or range above 1, a reserved
// byte that is not 0; the message names the frame (colour_per_frame == 0: colour[0] is every frame's)
int yuv_colour_check(const std::string& who, int nframes, const sjpeg_hip_yuv_colour* colour, int colour_per_frame);
// NULL, or BT.601 full range for every frame: there is nothing to convert
bool yuv_colour_all_identity(int nframes, const sjpeg_hip_yuv_colour* colour, int colour_per_frame);
// The colours checked, then a descriptor per frame of `planes` -- the plan of yuv_resize_plan, or the placed one of a
// sheet_plan of a YUV-plane format.
int yuv_colour_plan(const std::string& who, const YuvResizePlan& planes, const sjpeg_hip_yuv_colour* colour, int colour_per_frame,
                    YuvColourPlan* plan);
int yuv_colour_launch(bool placed, const YuvColourFrame* d_frames, int nframes, unsigned tiles, hipStream_t st);
// The engine's half (engine_pictures.cc): the descriptors rebased to `base`, uploaded into a buffer of their own and the
// kernel launched on `stream`, behind the resize launch that made the planes.  No tiles: nothing is done.
int engine_yuv_colour(sjpeg_hip_engine* e, const std::string& who, const YuvColourPlan& plan, uint8_t* base, void* stream);

// ---- unsharp mask (sjpeg_hip_unsharp_ragged_src; unsharp_plan.cc, unsharp.hip): the made pictures of any plan above
// but a sheet's, sharpened by ONE launch behind the launch that made them, out of place -- read at one base, written in
// the same layout at another.  One descriptor per PLANE to write, a plane rows of bytes with a channel step; the flat
// grid runs over the tiles of every plane of every frame, a workgroup finds its plane by the binary search over
// tile_base.  A tile is kUnsharpTileDwords dwords x kUnsharpTileRows rows of the plane, a plane's tiles in row-major
// order.  A plane with amount 0 (U and V) is copied by the same code.
constexpr unsigned kUnsharpTileDwords = 64, kUnsharpTileRows = 16;
struct UnsharpPlane {
  const uint8_t* src;                    // the made plane's first sample: a multiple of 4 (the plan: from the buffer's start)
  uint8_t* dst;                          // ... and where the sharpened one goes
  unsigned width_bytes, rows;            // the samples of a row (a pixel of interleaved RGB: three), the rows
  unsigned src_stride, dst_stride;       // bytes between rows: multiples of 4, each at least width_bytes rounded up to 4
  unsigned step;                         // bytes between two samples of a channel: 3 (interleaved RGB) or 1
  unsigned amount, threshold;            // sjpeg_hip_unsharp's, 0..255 each
  unsigned tile_base;                    // the plane's first workgroup in the flat grid
};
struct UnsharpPlan {
  std::vector<UnsharpPlane> planes;      // frame after frame; src == dst: the offset from the pictures' base
  unsigned tiles = 0;
  size_t bytes = 0;                      // what the pictures take from their base: the plan's that made them (the kind sets it)
};
// 0 for parameters the entries take (NULL: none to check), else SJPEG_HIP_EINVAL: a reserved byte that is not 0; the
// message names the frame (unsharp_per_frame == 0: unsharp[0] is every frame's)
int unsharp_check(const std::string& who, int nframes, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame);
// NULL, or amount 0 for every frame: there is nothing to sharpen
bool unsharp_all_zero(int nframes, const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame);
// The parameters checked, then the descriptors of `made` -- nframes made pictures of `format` (SJPEG_HIP_SRC_RGB, _GRAY,
// _YUV420 or _YUV444, anything else is refused) standing at `base`, as a plan kind's frames() reports them: one plane
// of step 3, one of step 1, or Y, U, V of step 1 with U's and V's amount 0.  A plane or stride that is no multiple of
// 4, a stride below the row and a batch of more than 0x7fffffff tiles are refused, naming the frame.
int unsharp_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* made, const uint8_t* base,
                 const sjpeg_hip_unsharp* unsharp, int unsharp_per_frame, UnsharpPlan* plan);
int unsharp_launch(const UnsharpPlane* d_planes, int nplanes, unsigned tiles, hipStream_t st);
// The engine's half (engine_pictures.cc): the descriptors rebased -- src to src_base, dst to d_out --, uploaded into a
// buffer of their own and the kernel launched on `stream`, behind the launch that made the pictures.  d_out == NULL:
// into the engine's memory for FINAL pictures, plan.bytes of it -- apart from the one for reduced pictures, where the made
// ones stay; counted by sjpeg_hip_engine_scratch_bytes and released by sjpeg_hip_engine_trim; *base says where.
int engine_unsharp(sjpeg_hip_engine* e, const std::string& who, const UnsharpPlan& plan, const uint8_t* src_base, uint8_t* d_out, uint8_t** base,
                   void* stream);

// ---- resampling with Pillow's filters (sjpeg_hip_resample_ragged_src; resample_plan.cc, resample.hip,
// resample_math.h): every frame resampled along x, then along y, by the tables of its two axes, to a size that may be
// larger or smaller on either axis, then turned.  One descriptor per frame; the flat grid runs over the tiles of every
// frame, a workgroup finds its frame by the binary search over tile_base.  A tile is tw x kResampleTileRows samples of
// the resampled STORED picture (tw one of kResampleTileCols, 16, 8, 4: the widest whose segment -- the union of its
// x-windows -- is at most kResampleSegmentMax source pixels), a frame's tiles in row-major order.  The tables of a call
// lie in ONE buffer of int32: per (filter, in, out) that occurs, once, the bounds {xmin, n} of every output sample and
// then its ksize coefficients; a pass that is not run (in == out) has the identity table, one tap of 2^22.  An axis
// whose ksize is above kResampleKsizeMax is refused.
constexpr unsigned kResampleTileCols = 32, kResampleTileRows = 16, kResampleStageBytes = 16384, kResampleSegmentMax = 4096;
constexpr int kResampleKsizeMax = 385;
struct ResampleFrame {
  const uint8_t* src;                    // plane 0, row 0
  long long row_stride;                  // may be negative
  long long off[3];                      // where R, G and B (gray: the value, thrice) lie from src (layout_rgb_offsets)
  uint8_t* dst;                          // the made picture: a multiple of 16 (the plan: from the buffer's start)
  const int32_t *xb, *xk, *yb, *yk;      // the axes' bounds and coefficients (the plan: int32s from the tables' start)
  int W, H, w2, h2;                      // the source's and the resampled stored picture's size
  int ksx, ksy;                          // coefficients a row of xk, yk
  int tw;                                // the tile's width
  unsigned tiles_x, dst_stride;          // tiles a row of tiles; bytes between the made picture's rows
  unsigned tile_base, orient;            // the frame's first workgroup in the flat grid; its EXIF orientation, 1..8
};
// ... and of the box entries (sjpeg_hip_resample_box_ragged_src; resample_box.hip), where a frame is REDUCED as it is
// staged: sample (X, Y) of the picture the tables are of -- r.W x r.H -- is Pillow's reduce of the block of fx x fy
// source samples at (x0 + X * fx, y0 + Y * fy), cut off at x0 + w and y0 + h.  m: the multipliers of an interior, a
// right-edge, a bottom-edge and a corner block (resample_math.h).  fx = fy = 1: the picture itself, m = 2^24.  A
// descriptor of its own: ResampleFrame keeps its size, and resample.hip's kernel its instructions.
struct ResampleStage {
  int fx, fy, x0, y0, w, h;
  uint32_t m[4];
};
struct ResampleBoxFrame {
  ResampleFrame r;
  ResampleStage s;
};
struct ResamplePlan {
  int format = 0, resized_format = 0;
  std::vector<ResampleFrame> frames;
  std::vector<ResampleStage> stages;     // a box call with a frame that is reduced: every frame's; else empty
  std::vector<int32_t> tables;           // what goes up: every table of the call, once
  int ntables = 0;                       // ... how many (identity tables included)
  size_t bytes = 0;
  unsigned tiles = 0;
  bool flat = false;                     // the frames are flattened as they are staged
  sjpeg_hip_flatten flatten = {};
};
// 0 for parameters the entries take, else SJPEG_HIP_EINVAL: resample == NULL, a filter that is none of
// SJPEG_HIP_RESAMPLE_*, a reserved byte that is not 0; the message names the frame (resample_per_frame == 0:
// resample[0] is every frame's)
int resample_check(const std::string& who, int nframes, const sjpeg_hip_resample* resample, int resample_per_frame);
// Checks the format (an RGB-like or gray one: a YUV-plane format is refused by name), the parameters, the sizes
// (sizes[f] = (w', h'), 1..65535 each, in the STORED orientation; NULL: every frame at its own size), the orientations
// and the flatten as resize_plan does, every axis's ksize against the cap and every table against resample_math.h's
// two bounds, then plans; the message names the frame and the axis.  The picture in the buffer is the upright one, in
// reduce_round.h's layout.  The frames' planes and strides are the caller's to check (ragged_check).
int resample_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                  const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_flatten* flatten,
                  ResamplePlan* plan);
// ... and of the box entries: every frame has a source box and a reducing_gap (box[f], or box[0] for all; sjpeg_hip.h,
// "THE DEFINITION of the box entries").  The box, the gap, a factor above kResampleFactorMax and a picture that Pillow
// would resample along y first are refused, naming the frame; the tables are of the reduced picture and of the box
// rounded to float32, one per (filter, in, out, box ends), held to the same bounds and window checks; the cap on ksize
// applies behind the reduce.  No frame reduced: plan->stages is empty and the plan is one for resample.hip's kernel.
int resample_box_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                      const uint8_t* orientations, const sjpeg_hip_resample* resample, int resample_per_frame, const sjpeg_hip_resample_box* box,
                      int box_per_frame, const sjpeg_hip_flatten* flatten, ResamplePlan* plan);
void resample_plan_frames(const ResamplePlan& plan, const sjpeg_hip_ragged_frame* frames, uint8_t* base, sjpeg_hip_ragged_frame* out);
// flatten NULL: not flat
int resample_launch(int format, const float* pscale, const float* pbias, const sjpeg_hip_flatten* flatten, const ResampleFrame* d_frames,
                    int nframes, unsigned tiles, hipStream_t st);
// ... the same over frames that are reduced as they are staged (resample_box.hip)
int resample_box_launch(int format, const float* pscale, const float* pbias, const sjpeg_hip_flatten* flatten, const ResampleBoxFrame* d_frames,
                        int nframes, unsigned tiles, hipStream_t st);
// The engine's half (engine_pictures.cc), as engine_resize; the tables go into engine memory of their own, counted by
// sjpeg_hip_engine_scratch_bytes and released by sjpeg_hip_engine_trim
int engine_resample(sjpeg_hip_engine* e, const std::string& who, const ResamplePlan& plan, uint8_t* d_out, uint8_t** base, void* stream);

// ---- Pillow's BoxBlur, GaussianBlur and UnsharpMask (sjpeg_hip_filter_ragged_src; pillow_filter_plan.cc,
// pillow_filter.hip, pillow_filter_math.h): the made RGB or gray pictures of the box entries filtered by TWO launches
// behind the launch that made them -- every pass along the rows from the made pictures to a scratch buffer of the same
// layout, every pass along the columns from there to the output, the unsharp combine fused into the second.  One
// descriptor per frame; each launch is a flat grid over the tiles of every frame, a workgroup finds its frame by the
// binary search over tile_base[launch].  A frame of kind 0, and an axis that is skipped, is copied by the same code.
struct PillowFilterPlane {
  const uint8_t* made;                   // the made picture's first sample: a multiple of 4 (the plan: from the buffer's start)
  uint8_t* mid;                          // ... the same place in the scratch buffer between the two launches
  uint8_t* dst;                          // ... and in the output
  unsigned width, rows;                  // pixels a row, rows
  unsigned stride;                       // bytes between rows, in all three: a multiple of 4, at least the row rounded up to 4
  unsigned step;                         // bytes a pixel: 3 (interleaved RGB) or 1
  unsigned kind, percent, threshold;     // sjpeg_hip_pillow_filter's
  PillowFilterAxis axis[2];              // along the rows, along the columns
  unsigned tile_base[2];                 // the frame's first workgroup in the row launch's and the column launch's grid
};
struct PillowFilterPlan {
  std::vector<PillowFilterPlane> planes; // frame after frame; made == mid == dst: the offset from the pictures' base
  unsigned tiles[2] = {0, 0};            // the grids of the row launch and the column launch
  size_t bytes = 0;                      // what the pictures take from their base: the plan's that made them (the kind sets it)
};
// 0 for parameters the entries take (NULL: none to check), else SJPEG_HIP_EINVAL naming the frame (filter_per_frame == 0:
// filter[0] is every frame's): an unknown kind, a radius that is negative or not finite, an axis whose integer box
// radius exceeds kPillowFilterRadiusMax or whose weights break pillow_filter_axis_bound, kind 3 with two radii, a
// reserved byte that is not 0
int pillow_filter_check(const std::string& who, int nframes, const sjpeg_hip_pillow_filter* filter, int filter_per_frame);
// NULL, or kind 0 for every frame (reserved bytes 0): there is nothing to filter
bool pillow_filter_all_none(int nframes, const sjpeg_hip_pillow_filter* filter, int filter_per_frame);
// The parameters checked, then the descriptors of `made` -- nframes made pictures of `format` (SJPEG_HIP_SRC_RGB or
// _GRAY, anything else is refused) standing at `base`, as a plan kind's frames() reports them -- and the two grids.  A
// plane or stride that is no multiple of 4, a stride below the row and more than 0x7fffffff tiles are refused.
int pillow_filter_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* made, const uint8_t* base,
                       const sjpeg_hip_pillow_filter* filter, int filter_per_frame, PillowFilterPlan* plan);
// launch 0: along the rows, made -> mid; launch 1: along the columns, mid (and made) -> dst
int pillow_filter_launch(int launch, const PillowFilterPlane* d_planes, int nplanes, unsigned tiles, hipStream_t st);
// The engine's half (engine_pictures.cc), as engine_unsharp: the descriptors rebased -- made to src_base, mid to the
// engine's scratch of the made pictures' layout, dst to d_out (NULL: the engine's memory for FINAL pictures) --,
// uploaded into a buffer of their own and the two launches on `stream`.
int engine_pillow_filter(sjpeg_hip_engine* e, const std::string& who, const PillowFilterPlan& plan, const uint8_t* src_base, uint8_t* d_out,
                         uint8_t** base, void* stream);

// ---- compose: a canvas and overlays behind the made pictures (sjpeg_hip_compose_ragged_src; compose_plan.cc,
// compose.hip, compose_math.h): the made RGB or gray pictures of the box or the filtered entries copied onto canvases
// of their own layout and overlays blended over them by ONE launch -- a flat grid over the tiles of every canvas, a
// workgroup finds its frame by the binary search over tile_base.  One descriptor per frame with its places resolved:
// the anchors are gone, an overlay's top-left is a canvas coordinate.  A frame without compose is a canvas of the
// picture's own size: copied by the same launch.
struct ComposePlace {
  const uint8_t* rgba;                   // the overlay's first pixel: a multiple of 4
  int ox, oy;                            // its top-left on the canvas; may be negative or beyond the canvas
  unsigned ow, oh;                       // its size in pixels
  unsigned stride;                       // bytes between its rows: a multiple of 4
  unsigned unused;
};
struct ComposeFrame {
  const uint8_t* made;                   // the made picture's first sample: a multiple of 4 (the plan: from the pictures' base)
  uint8_t* dst;                          // the canvas's first sample: a multiple of 16 (the plan: from the canvases' base)
  unsigned cw, ch;                       // the canvas, pixels and rows
  unsigned w, h, px, py;                 // the picture and where it lies: px + w <= cw, py + h <= ch
  unsigned src_stride, dst_stride;       // bytes between rows: multiples of 4
  unsigned step;                         // bytes a pixel: 3 (interleaved RGB) or 1
  unsigned colour;                       // the canvas's colour: R | G << 8 | B << 16 (gray: R alone is used)
  unsigned nplaces;                      // 0..kComposePlacesMax
  unsigned tile_base;                    // the frame's first workgroup in the grid
  ComposePlace place[kComposePlacesMax];
};
struct ComposePlan {
  std::vector<ComposeFrame> frames;      // frame after frame
  unsigned tiles = 0;                    // the grid
  size_t bytes = 0;                      // what the canvases take from their base
  bool identity = true;                  // every frame is its picture at its own size and has no place
};
// 0 for structs the entries take, else SJPEG_HIP_EINVAL naming the frame, overlay or place: what can be said without
// the pictures -- reserved bytes, modes, anchors, canvas sides, centerings, the place ranges, overlay indices, overlays
int compose_check(const std::string& who, int nframes, const sjpeg_hip_compose* compose, int compose_per_frame, const sjpeg_hip_overlay* overlays,
                  int noverlays, const sjpeg_hip_overlay_place* places, int nplaces);
// NULL, or every frame's canvas 0 x 0 with the picture at (0, 0) and no place (reserved bytes 0): nothing to compose
// whatever the pictures are
bool compose_all_none(int nframes, const sjpeg_hip_compose* compose, int compose_per_frame);
// The structs checked, then the descriptors over `made` -- nframes made pictures of `format` (SJPEG_HIP_SRC_RGB or
// _GRAY, anything else is refused) standing at `base` --: the canvases in the usual layout from offset 0, the places
// resolved, the grid.  A picture that leaves its canvas is refused, naming the frame.
int compose_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* made, const uint8_t* base,
                 const sjpeg_hip_compose* compose, int compose_per_frame, const sjpeg_hip_overlay* overlays, int noverlays,
                 const sjpeg_hip_overlay_place* places, int nplaces, ComposePlan* plan);
// the canvases as frames at `base`; out_offset and out_capacity are the caller's frames'
void compose_plan_frames(const ComposePlan& plan, const sjpeg_hip_ragged_frame* frames, uint8_t* base, sjpeg_hip_ragged_frame* out);
int compose_launch(const ComposeFrame* d_frames, int nframes, unsigned tiles, hipStream_t st);
// The engine's half (engine_pictures.cc): the descriptors rebased -- made to src_base, dst to d_out (NULL: the engine's
// memory for COMPOSED pictures, so that the launch is out of place whatever made the pictures) --, uploaded into a
// buffer of their own, and the launch on `stream`
int engine_compose(sjpeg_hip_engine* e, const std::string& who, const ComposePlan& plan, const uint8_t* src_base, uint8_t* d_out, uint8_t** base,
                   void* stream);

// ---- packed output of the ragged encodes (sjpeg_hip_encode_ragged_packed_src): where the frames of a call go when they
// lie back to back in one buffer.  Every ragged flow takes it as one optional argument (NULL: the frames' own
// out_offset, as ever) and hands it down to ragged_encode(), whose launches place their frames behind the engine's
// cursor.  A flow that codes a SUBSET or a reordering of its frames hands down a copy whose `index` names the caller's
// frame of each frame it passes on.
struct PackedSink {
  void* base;                    // d_packed, a multiple of 16
  uint64_t capacity;             // bytes behind it
  uint64_t* d_offsets;           // [nframes + 1], the caller's frame numbers; [nframes]: the cursor (bit 63: overflow)
  int nframes;                   // of the packed call
  const int* index;              // the caller's number of each frame handed to the flow (NULL: its own position)
};
// ---- per-picture metadata of a ragged call (sjpeg_hip_encode_ragged_full_meta_src): the call's entries, checked and
// turned into their segments before any device work.  The engine holds a pointer to it for the length of the call
// (engine_meta); every place that builds a frame's header, and the size search, asks it for the frame's entry.  `index`
// is PackedSink::index again: a flow that codes a subset of its frames points it at the caller's number of each frame
// it passes on.
struct FrameMeta {
  sjpeg_host::Metadata meta;       // what the search counts (SearchHeaderBits)
  std::vector<uint8_t> block;      // its segments: the bytes behind SOI + APP0
};
struct MetaCtx {
  std::vector<FrameMeta> entries;  // one for all frames, or one per frame
  int per_frame = 0;
  const int* index = nullptr;
  const FrameMeta& of(int f) const { return entries[per_frame ? (index != nullptr ? index[f] : f) : 0]; }
};
// the metadata of the call the engine is running (NULL: none), and setting it
MetaCtx* engine_meta(const sjpeg_hip_engine* e);
void engine_set_meta(sjpeg_hip_engine* e, MetaCtx* ctx);
// frame f's entry (f: as the flow at hand numbers its frames), or NULL without metadata
inline const FrameMeta* frame_meta(const sjpeg_hip_engine* e, int f) {
  const MetaCtx* const c = engine_meta(e);
  return c != nullptr ? &c->of(f) : nullptr;
}
// A frame's header behind *headers: SOI + APP0, the frame's metadata segments, DQT, SOF0, DHT (specs[4], or NULL for
// the default codes), SOS
bool append_frame_header(int width, int height, int yuv_mode, const uint8_t quant[2][64], const sjpeg_hip_huffman_spec* specs,
                         const FrameMeta* fm, std::vector<uint8_t>* headers);

// the entry points' flows with a sink (the public functions pass NULL); ragged_flows.cc and ragged_full.cc
int ragged_batch_flow(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes, const sjpeg_hip_ragged_frame* frames,
                      const uint8_t (*quant)[2][64], int quant_per_frame, const uint8_t* min_quant, int q_bias, int method,
                      int qdelta_max_luma, int qdelta_max_chroma, void* d_out, uint64_t* d_sizes, void* stream,
                      const PackedSink* sink);
int ragged_search_flow(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes, const sjpeg_hip_ragged_frame* frames,
                       const uint8_t (*quant)[2][64], int quant_per_frame, const uint8_t* min_quant, int q_bias, int method,
                       int qdelta_max_luma, int qdelta_max_chroma, const sjpeg_hip_search* search, int search_per_frame,
                       float* q_out, float* value_out, void* d_out, uint64_t* d_sizes, void* stream, const PackedSink* sink);

// ---- the search over a ragged batch (ragged_full.cc) and what it takes from the engine (scan_engine.hip: the launch
// layer; ragged_flows.cc: the flows)
int set_error(int code, const std::string& msg);          // sjpeg_hip_last_error() of the calling thread
size_t engine_scratch_limit(const sjpeg_hip_engine* e);   // SJPEG_HIP_SCRATCH_LIMIT_BYTES
int engine_device(const sjpeg_hip_engine* e);
// n sizes of engine-owned device memory (the search's sub-calls leave their sizes there, queued on the call's stream)
int engine_search_sizes(sjpeg_hip_engine* e, size_t n, uint64_t** d_sizes);
// the checks of a ragged encode's format, yuv_mode and frames (output ranges included); the message names the frame.
// esz: the size of a sample where it is not the format's own -- 2 for the deep entries, whose planes hold 16-bit
// samples: the same rules with rows twice as long, planes and strides multiples of 2
int ragged_check(const std::string& who, int format, int yuv_mode, int nframes, const sjpeg_hip_ragged_frame* frames, int esz = 0);
// the counted bits of frames[0, nframes) with the first plan, no host wait: ~0 for a frame that overflowed it (checked
// as sjpeg_hip_scan_counted_bits_ragged_src)
int counted_bits_first(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes, const sjpeg_hip_ragged_frame* frames,
                       const sjpeg_hip_scan_tables* tables, int tables_per_frame, uint64_t* d_bits, hipStream_t st);
// ... and frames[which[k]] counted again with their worst-case plan into d_bits[which[k]]
int counted_bits_recount(sjpeg_hip_engine* e, int format, int yuv_mode, const sjpeg_hip_ragged_frame* frames,
                         const sjpeg_hip_scan_tables* tables, int tables_per_frame, const std::vector<int>& which,
                         uint64_t* d_bits, hipStream_t st);
// AnalyseHisto's device half (adapt_sums_kernel, adapt_decide_kernel) over n consecutive frames: hist [n][2][64][128],
// each from its own starting matrices d_quant_in[n][128]; the adapted ones into d_quant_out[n][128].  d_sums / d_totlast:
// n frames' worth of scratch.
int adapt_ragged(const uint32_t* d_hist, const uint8_t* d_quant_in, int n, const uint8_t* min_quant, int ntab,
                 int qdelta_max_luma, int qdelta_max_chroma, int64_t* d_sums, int32_t* d_totlast, uint8_t* d_quant_out,
                 hipStream_t st);

// ... and, for any sampling and the trellis (sjpeg_hip_encode_ragged_full_src):
// the unsearched flow of a SjpegYUVMode and method 0..8 (sjpeg_hip_encode_ragged_auto_src / _trellis_src), with a sink
int ragged_unsearched_flow(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes, const sjpeg_hip_ragged_frame* frames,
                           const uint8_t (*quant)[2][64], int quant_per_frame, const uint8_t* min_quant, int q_bias, int method,
                           int qdelta_max_luma, int qdelta_max_chroma, void* d_out, uint64_t* d_sizes, int* modes, void* stream,
                           const PackedSink* sink);
// a mode group of a call: frames of one source format and sampling (the sharp frames: planar 4:2:0 in engine scratch)
struct ModeGroup {
  int format = 0, yuv_mode = 0;                   // SJPEG_HIP_SRC_*, SJPEG_HIP_YUV*
  std::vector<sjpeg_hip_ragged_frame> frames;
  std::vector<int> index;                         // the caller's number of each frame
};
// the method 0..6 flow of sjpeg_hip_encode_ragged_batch_src over several groups at once (every pass over all groups, then
// its one wait); quant[index], d_sizes[index]
int ragged_groups_flow(sjpeg_hip_engine* e, const std::string& who, const std::vector<ModeGroup>& groups,
                       const uint8_t (*quant)[2][64], const uint8_t* min_quant, int q_bias, int method, int qdelta_max_luma,
                       int qdelta_max_chroma, void* d_out, uint64_t* d_sizes, void* stream, const PackedSink* sink);
// the engine's kept blocks (kKeptSegWords a segment) for `segs` segments; its arena (the sharp planes); the counters of
// sjpeg_hip_engine_search_stats; the packed cursor zeroed on the stream
int engine_kept_blocks(sjpeg_hip_engine* e, size_t segs);
int engine_arena(sjpeg_hip_engine* e, size_t bytes, uint8_t** p);
uint64_t* engine_full_stats(sjpeg_hip_engine* e);
int engine_pack_begin(sjpeg_hip_engine* e, void* stream);
// the trellis statistics of frames[0, n) with tables[f] (SJPEG_HIP_QUANT_TRELLIS; trellis_len: the frame's rate table):
// d_freq[n][2][272]; frame f's quantized blocks stay kept_base[f] segments into the engine's kept blocks
int trellis_stats_ragged(sjpeg_hip_engine* e, const std::string& who, int format, int yuv_mode, int nframes,
                         const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_scan_tables* tables, const uint32_t* kept_base,
                         uint32_t* d_freq, hipStream_t st);
// ... and the encode that replays them with tables[f]'s codes (complete JPEGs: headers, EOI)
int replay_encode_ragged(sjpeg_hip_engine* e, const std::string& who, int format, int yuv_mode, int nframes,
                         const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_scan_tables* tables, const uint32_t* kept_base,
                         const void* headers, const size_t* header_offsets, void* d_out, uint64_t* d_sizes, hipStream_t st,
                         const PackedSink* sink);

// ---- one description of a _full_ call (ragged_full.cc) and of the shaped calls on top of it (ragged_shaped.cc)
// Where a call's streams and answers go: frame f at d_out + its out_offset (strided, the sheet entries: sheet s at
// s * out_stride) -- or packed: d_out is d_packed, the frames back to back behind the engine's cursor.
struct RaggedOut {
  void* d_out;
  uint64_t* d_sizes;
  int* modes;
  float *q_out, *value_out;
  void* stream;
  bool packed = false, strided = false;
  size_t out_stride = 0, packed_capacity = 0;
  uint64_t* d_offsets = nullptr;
  RaggedOut strided_by(size_t stride) const { RaggedOut o = *this; o.strided = true; o.out_stride = stride; return o; }
  RaggedOut packed_into(size_t capacity, uint64_t* offsets) const {          // (d_out is d_packed)
    RaggedOut o = *this; o.packed = true; o.packed_capacity = capacity; o.d_offsets = offsets; return o;
  }
  PackedSink sink(int nframes) const { return {d_out, packed_capacity, d_offsets, nframes, nullptr}; }
};
// The call: whose name its messages carry, what it codes and with what.  A pass-through renames it and hands it on; a
// flow that makes pictures hands on a copy with format, nframes and frames those of what it made.
struct RaggedCall {
  const std::string* who;
  sjpeg_hip_engine* e;
  int format, nframes;
  const sjpeg_hip_ragged_frame* frames;
  const sjpeg_hip_ragged_params* params;
  const sjpeg_hip_metadata* meta;       // NULL: none
  int meta_per_frame;
  RaggedOut out;
};
// The checks every encode entry starts with, in the order its messages are recorded in (tests/golden/c_messages.json):
// engine, params, d_offsets (packed), frames, the entry's sheet (has_sheet), d_out / d_packed, d_sizes, d_packed's
// alignment and capacity, out_stride (strided), the YUV-plane format (yuv_only), nframes.  Host only.
int encode_prologue(const RaggedCall& c, bool has_sheet = false, const void* sheet = nullptr, bool yuv_only = false);
// the checks of a _full_ call behind its prologue (host only), and the call itself: full_checks again, then the search
int full_checks(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_ragged_params& P);
int full_flow(const RaggedCall& c);
// the four sjpeg_hip_encode_ragged_full[_meta][_packed]_src entries: c.who is set here -- meta == NULL answers under
// the name of the entry without metadata
int full_entry(RaggedCall c);
// The call's metadata -- one entry, or one per frame -- checked and turned into segments, before any device work
int check_metadata(const std::string& who, int nframes, const sjpeg_hip_metadata* meta, int meta_per_frame, MetaCtx* ctx);
// the engine carries the call's metadata (NULL: the call has none) while the call runs
struct MetaScope {
  sjpeg_hip_engine* e;
  MetaScope(sjpeg_hip_engine* engine, MetaCtx* ctx) : e(ctx != nullptr ? engine : nullptr) { if (e != nullptr) engine_set_meta(e, ctx); }
  ~MetaScope() { if (e != nullptr) engine_set_meta(e, nullptr); }
};

}  // namespace sjpeg_internal
