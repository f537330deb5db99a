// yuv_resize_plan.cc -- the host half of the ragged resize of the YUV-plane formats (sjpeg_hip_resize_ragged_yuv_src,
// sjpeg_hip_encode_ragged_yuv_resized_src; sjpeg_hip.h): the size of a plane, the checks of the sizes and orientations,
// and the plan -- one descriptor per plane, two for the semi-planar formats -- that resize.hip's kernel runs over.
// Plain C++, no device work: tests/cxx/yuv_resize_plan_test.cc compiles it as it is.
#include <string.h>

#include <string>

#include "orient_math.h"
#include "ragged_aux.h"
#include "reduce_round.h"
#include "resize_math.h"
#include "sjpeg_hip.h"
#include "source_layout.h"

namespace sjpeg_internal {

const char* source_format_name(int format) {
  static const char* const kNames[kSourceFormats] = {
      "SJPEG_HIP_SRC_RGB", "SJPEG_HIP_SRC_BGRA", "SJPEG_HIP_SRC_RGBA", "SJPEG_HIP_SRC_GRAY", "SJPEG_HIP_SRC_YUV444",
      "SJPEG_HIP_SRC_YUV420", "SJPEG_HIP_SRC_NV12", "SJPEG_HIP_SRC_NV21", "SJPEG_HIP_SRC_RGB_PLANAR",
      "SJPEG_HIP_SRC_RGB_PLANAR_F32", "SJPEG_HIP_SRC_RGB_PLANAR_F16", "SJPEG_HIP_SRC_RGB_PLANAR_BF16", "SJPEG_HIP_SRC_RGB_F32",
      "SJPEG_HIP_SRC_RGB_F16", "SJPEG_HIP_SRC_RGB_BF16", "SJPEG_HIP_SRC_RGBA_F32", "SJPEG_HIP_SRC_RGBA_F16",
      "SJPEG_HIP_SRC_RGBA_BF16", "SJPEG_HIP_SRC_GRAY_F32", "SJPEG_HIP_SRC_GRAY_F16", "SJPEG_HIP_SRC_GRAY_BF16"};
  return format >= 0 && format < kSourceFormats ? kNames[format] : "this format";
}

// a format with luma and chroma planes of bytes: the four the kernel's per-plane grid reads
static bool yuv_planes(const SourceLayout& L) { return L.cls == kSrcPlanes && L.planes >= 2; }

int yuv_format_check(const std::string& who, int format) {
  const SourceLayout* const L = source_layout(format);
  if (L == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": unknown source format");
  if (yuv_planes(*L)) return 0;
  return set_error(SJPEG_HIP_EINVAL, who + ": " + source_format_name(format) + " is not a YUV-plane format (RGB-like and gray pictures are resized "
                                         "and turned by sjpeg_hip_orient_ragged_src and sjpeg_hip_encode_ragged_oriented_src)");
}

int yuv_depth_check(const std::string& who, const sjpeg_hip_yuv_depth* depth) {
  if (depth == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": depth == NULL");
  if (depth->bytes != 2) {
    return set_error(SJPEG_HIP_EINVAL, who + ": depth: bytes " + std::to_string(depth->bytes) + " is not 2 (samples of one byte go to the entries "
                                           "without a depth)");
  }
  if (depth->shift > 8) return set_error(SJPEG_HIP_EINVAL, who + ": depth: shift " + std::to_string(depth->shift) + " is not one of 0..8");
  if (depth->reserved[0] != 0 || depth->reserved[1] != 0) return set_error(SJPEG_HIP_EINVAL, who + ": depth: reserved must be 0");
  return 0;
}

int yuv_resize_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                    const uint8_t* orientations, YuvResizePlan* plan, const sjpeg_hip_yuv_depth* depth) {
  if (int rc = yuv_format_check(who, format)) return rc;
  if (depth != nullptr) { if (int rc = yuv_depth_check(who, depth)) return rc; }
  const SourceLayout* const L = source_layout(format);
  if (nframes < 1 || nframes > 65535) return set_error(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
  for (int f = 0; f < nframes; ++f) {
    const sjpeg_hip_ragged_frame& fr = frames[f];
    const std::string frame = who + ": frame " + std::to_string(f) + ": ";
    if (fr.width < 1 || fr.height < 1 || fr.width > 65535 || fr.height > 65535) {
      return set_error(SJPEG_HIP_EINVAL, frame + "bad dimensions " + std::to_string(fr.width) + "x" + std::to_string(fr.height));
    }
    if (orientations != nullptr && (orientations[f] < 1 || orientations[f] > 8)) {
      return set_error(SJPEG_HIP_EINVAL, frame + "orientation " + std::to_string(orientations[f]) + " is not one of 1..8 (EXIF tag 0x0112)");
    }
    if (sizes == nullptr) continue;
    const std::string size = "size " + std::to_string(sizes[f][0]) + "x" + std::to_string(sizes[f][1]);
    if (sizes[f][0] < 1 || sizes[f][1] < 1) return set_error(SJPEG_HIP_EINVAL, frame + size + " is below 1x1");
    if (sizes[f][0] > fr.width || sizes[f][1] > fr.height) {
      return set_error(SJPEG_HIP_EINVAL, frame + size + " is above the source's " + std::to_string(fr.width) + "x" + std::to_string(fr.height) +
                                             " (pictures are made smaller, never larger)");
    }
  }
  const bool semi = L->planes == 2;
  plan->format = format;
  plan->resized_format = L->implied == SJPEG_HIP_YUV444 ? SJPEG_HIP_SRC_YUV444 : SJPEG_HIP_SRC_YUV420;
  plan->nframes = nframes;
  plan->deep = depth != nullptr;
  plan->shift = depth != nullptr ? depth->shift : 0u;
  plan->planes.clear();
  plan->planes.reserve(static_cast<size_t>(nframes) * (semi ? 2 : 3));
  size_t at = 0;
  unsigned long long tiles = 0;
  for (int f = 0; f < nframes; ++f) {
    const sjpeg_hip_ragged_frame& fr = frames[f];
    const int w2 = sizes != nullptr ? sizes[f][0] : fr.width, h2 = sizes != nullptr ? sizes[f][1] : fr.height;
    const unsigned orient = orientations != nullptr ? orientations[f] : 1u;
    // where the three made planes lie: Y, U, V, each the UPRIGHT plane (its height x width for the orientations that
    // transpose), rows whole dwords apart, at a multiple of 16
    size_t place[3];
    unsigned stride[3];
    for (int c = 0; c < 3; ++c) {
      int pw, ph;
      yuv_plane_dims(*L, w2, h2, c, &pw, &ph);
      uint32_t uw, uh;
      oriented_size(static_cast<uint32_t>(pw), static_cast<uint32_t>(ph), static_cast<int>(orient), &uw, &uh);
      place[c] = at;
      stride[c] = static_cast<unsigned>(reduced_row_stride(static_cast<int>(uw), 1));
      at += reduced_picture_bytes(static_cast<int>(uw), static_cast<int>(uh), 1);
    }
    for (int i = 0; i < L->planes; ++i) {
      YuvPlane p;
      memset(&p, 0, sizeof(p));
      ResizeFrame& d = p.r;
      d.src = static_cast<const uint8_t*>(fr.plane[i]);
      d.row_stride = fr.row_stride[i];
      yuv_plane_dims(*L, fr.width, fr.height, i, &d.W, &d.H);
      yuv_plane_dims(*L, w2, h2, i, &d.w2, &d.h2);
      p.channels = semi && i == 1 ? 2 : 1;
      p.frame = f;
      if (p.channels == 2) { d.off[0] = L->uoff; d.off[1] = L->voff; }
      const unsigned long long plane_tiles = resize_tile_rule(&d);
      d.orient = orient;
      d.dst = reinterpret_cast<uint8_t*>(place[i]);               // (from the buffer's start: engine_yuv_resize adds it)
      d.dst_stride = stride[i];
      if (p.channels == 2) p.dst2 = reinterpret_cast<uint8_t*>(place[2]);
      d.tile_base = static_cast<unsigned>(tiles);
      tiles += plane_tiles;
      if (tiles > 0x7fffffffull) return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": the batch has too many tiles for one launch");
      plan->planes.push_back(p);
    }
  }
  plan->bytes = at;
  plan->tiles = static_cast<unsigned>(tiles);
  return 0;
}

void yuv_resize_plan_frames(const YuvResizePlan& plan, const sjpeg_hip_ragged_frame* frames, uint8_t* base, sjpeg_hip_ragged_frame* out) {
  for (int f = 0; f < plan.nframes; ++f) memset(&out[f], 0, sizeof(out[f]));
  for (size_t k = 0; k < plan.planes.size(); ++k) {
    const YuvPlane& p = plan.planes[k];
    const ResizeFrame& d = p.r;
    sjpeg_hip_ragged_frame& r = out[p.frame];
    // (the frame's descriptors in a row: Y, then U and V or the pair)
    const int c = k == 0 || plan.planes[k - 1].frame != p.frame ? 0 : k == 1 || plan.planes[k - 2].frame != p.frame ? 1 : 2;
    if (c == 0) {
      uint32_t uw, uh;
      oriented_size(static_cast<uint32_t>(d.w2), static_cast<uint32_t>(d.h2), static_cast<int>(d.orient), &uw, &uh);
      r.width = static_cast<int32_t>(uw); r.height = static_cast<int32_t>(uh);
      r.out_offset = frames[p.frame].out_offset; r.out_capacity = frames[p.frame].out_capacity;
      r.plane[0] = base + reinterpret_cast<uintptr_t>(d.dst);
      r.row_stride[0] = static_cast<int64_t>(d.dst_stride);
      continue;
    }
    r.plane[c] = base + reinterpret_cast<uintptr_t>(d.dst);
    r.row_stride[c] = static_cast<int64_t>(d.dst_stride);
    if (p.channels == 2) {
      r.plane[2] = base + reinterpret_cast<uintptr_t>(p.dst2);
      r.row_stride[2] = static_cast<int64_t>(d.dst_stride);
    }
  }
}

}  // namespace sjpeg_internal

extern "C" {

int sjpeg_hip_yuv16_samples(const sjpeg_hip_yuv_depth* depth, size_t n, const uint16_t* in, uint8_t* out) {
  static const std::string who = "sjpeg_hip_yuv16_samples";
  using sjpeg_internal::set_error;
  if (int rc = sjpeg_internal::yuv_depth_check(who, depth)) return rc;
  if (n != 0 && (in == nullptr || out == nullptr)) return set_error(SJPEG_HIP_EINVAL, who + ": in or out == NULL");
  // (a one-sample picture: S = x, A = 1)
  for (size_t i = 0; i < n; ++i) out[i] = static_cast<uint8_t>(sjpeg_internal::resize_round_deep(in[i], 1u, 1u, depth->shift));
  return 0;
}

int sjpeg_hip_yuv_plane_size(int format, int width, int height, int plane, int* plane_width, int* plane_height) {
  static const std::string who = "sjpeg_hip_yuv_plane_size";
  using sjpeg_internal::set_error;
  if (plane_width == nullptr || plane_height == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": plane_width or plane_height == NULL");
  if (int rc = sjpeg_internal::yuv_format_check(who, format)) return rc;
  const sjpeg_internal::SourceLayout* const L = sjpeg_internal::source_layout(format);
  if (width < 1 || height < 1 || width > 65535 || height > 65535) {
    return set_error(SJPEG_HIP_EINVAL, who + ": bad dimensions " + std::to_string(width) + "x" + std::to_string(height));
  }
  if (plane < 0 || plane > 2) return set_error(SJPEG_HIP_EINVAL, who + ": plane " + std::to_string(plane) + " is not one of 0..2 (Y, U, V)");
  sjpeg_internal::yuv_plane_dims(*L, width, height, plane, plane_width, plane_height);
  return 0;
}

size_t sjpeg_hip_resize_ragged_yuv_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames, const int32_t (*sizes)[2],
                                         const uint8_t* orientations) {
  if (frames == nullptr) {
    sjpeg_internal::set_error(SJPEG_HIP_EINVAL, "sjpeg_hip_resize_ragged_yuv_bytes: frames == NULL");
    return 0;
  }
  try {
    sjpeg_internal::YuvResizePlan plan;
    if (sjpeg_internal::yuv_resize_plan("sjpeg_hip_resize_ragged_yuv_bytes", format, nframes, frames, sizes, orientations, &plan) != 0) return 0;
    return plan.bytes;
  } catch (...) {
    return 0;
  }
}

}  // extern "C"
