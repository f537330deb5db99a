// reduce.hip -- pictures of a ragged batch reduced by 1/1 .. 1/8 on gfx950: thumbnails and pyramid levels in ONE launch
// in front of the ragged encodes (sjpeg_hip_reduce_ragged_src, sjpeg_hip_encode_ragged_reduced_src; sjpeg_hip.h).
//
// Reference: none -- the reference codes the picture it is given (src/enc.cc:391-448).  The contract is on the bytes:
// frame f's reduced picture is the box average of s x s source bytes, rounded half up (reduce_round.h), the edges
// replicating the last column and row; a source byte is what the encoder sees there today (pixel_elem.h for floats).
//
// Shape: a flat grid over the batch's tiles, a workgroup one tile of one frame, found by a binary search over the
// frames' first tiles -- so the factor, the format's fields and the element kind are wave-uniform.  A thread makes one
// GROUP: four reduced pixels side by side, i.e. 4 s source pixels of s source rows.  Adjacent lanes make adjacent
// groups, so a wave reads one contiguous run of each source row, every lane its own 12 s (RGB), 16 s (BGRA / RGBA) or
// 4 s (a plane) bytes of it as dwords -- no byte loads inside the picture --, and writes whole dwords of the reduced
// row.  Groups that touch the right or lower edge, and the float formats, take the per-element path.  No LDS, no
// atomics.  DESIGN.md section 4.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "pixel_elem.h"
#include "ragged_aux.h"
#include "reduce_round.h"
#include "sjpeg_hip.h"
#include "source_layout.h"

static_assert(sjpeg_internal::kReduceMax == SJPEG_HIP_REDUCE_MAX, "reduce_round.h and sjpeg_hip.h name one largest factor");

namespace {

using sjpeg_internal::ReduceFrame;

// how a group inside the picture reads its bytes
enum { kReducePacked3 = 0, kReducePacked4 = 1, kReducePlanes = 2, kReduceElems = 3 };

struct ReduceArgs {
  const ReduceFrame* frames;
  int nframes;
  int cls;                       // kReduce*
  int kind;                      // kElem* (pixel_elem.h)
  int pix_step;                  // bytes from a pixel to the next
  int channels;                  // 3, or 1 for the gray formats
  float pscale[3], pbias[3];     // the engine's pixel transform (float formats)
};

// The pictures lie in device memory: saying so (the pointers come out of a descriptor, so the compiler cannot know)
// makes the loads and stores global_* instead of flat_*.  A dword of it, aligned like a byte: the sources are aligned
// to their element only.
typedef uint32_t __attribute__((aligned(1))) Dword1;
typedef const __attribute__((address_space(1))) Dword1* GlobalDwords;
typedef __attribute__((address_space(1))) uint32_t* GlobalOut;
template <int N>
__device__ __forceinline__ void load_dwords(const uint8_t* p, uint32_t* w) {
  GlobalDwords const g = (GlobalDwords)(p);
#pragma unroll
  for (int i = 0; i < N; ++i) w[i] = g[i];
}

// byte i of the dwords w[]
#define REDUCE_BYTE(w, i) (((w)[(i) >> 2] >> (8 * ((i) & 3))) & 0xffu)

// 4 S pixels of STEP bytes each over S rows at p: acc[j][c] += byte c of the pixels of reduced pixel j
template <int S, int STEP>
__device__ __forceinline__ void sum_packed(const uint8_t* p, long long row_stride, uint32_t (*acc)[3]) {
#pragma unroll
  for (int dy = 0; dy < S; ++dy) {
    uint32_t w[S * STEP];
    load_dwords<S * STEP>(p + dy * row_stride, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int dx = 0; dx < S; ++dx) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[j][c] += REDUCE_BYTE(w, (j * S + dx) * STEP + c);
      }
    }
  }
}

// 4 S samples of one plane over S rows at p into channel C
template <int S, int C>
__device__ __forceinline__ void sum_plane(const uint8_t* p, long long row_stride, uint32_t (*acc)[3]) {
#pragma unroll
  for (int dy = 0; dy < S; ++dy) {
    uint32_t w[S];
    load_dwords<S>(p + dy * row_stride, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int dx = 0; dx < S; ++dx) acc[j][C] += REDUCE_BYTE(w, j * S + dx);
    }
  }
}

// one group: reduced pixels 4 gx .. 4 gx + 3 of reduced row gy
template <int S>
__device__ __forceinline__ void reduce_group(const ReduceArgs& a, const ReduceFrame& d, int gx, int gy) {
  uint32_t acc[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  const int x0 = gx * 4 * S, y0 = gy * S;
  if (a.cls != kReduceElems && x0 + 4 * S <= d.W && y0 + S <= d.H) {
    // inside the picture: every byte of the group's rows belongs to it
    const uint8_t* const row = d.src + static_cast<long long>(y0) * d.row_stride;
    if (a.cls == kReducePacked3) {
      sum_packed<S, 3>(row + static_cast<long long>(x0) * 3, d.row_stride, acc);
    } else if (a.cls == kReducePacked4) {
      sum_packed<S, 4>(row + static_cast<long long>(x0) * 4, d.row_stride, acc);
    } else {
      sum_plane<S, 0>(row + d.off[0] + x0, d.row_stride, acc);
      if (a.channels == 3) {
        sum_plane<S, 1>(row + d.off[1] + x0, d.row_stride, acc);
        sum_plane<S, 2>(row + d.off[2] + x0, d.row_stride, acc);
      }
    }
    if (a.cls != kReducePlanes && d.off[0] != 0) {          // B, G, R in memory (wave-uniform)
#pragma unroll
      for (int j = 0; j < 4; ++j) { const uint32_t t = acc[j][0]; acc[j][0] = acc[j][2]; acc[j][2] = t; }
    }
  } else {
    // the edges (the last column and row replicated) and the float formats: element by element, and never an element
    // that is not a used sample of a pixel of the picture
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xo = gx * 4 + j;
      if (xo >= d.w2) continue;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (c >= a.channels) continue;
        uint32_t sum = 0;
#pragma unroll 1
        for (int dy = 0; dy < S; ++dy) {
          const int y = min(y0 + dy, d.H - 1);
          const uint8_t* const row = d.src + static_cast<long long>(y) * d.row_stride + d.off[c];
#pragma unroll 1
          for (int dx = 0; dx < S; ++dx) {
            const int x = min(xo * S + dx, d.W - 1);
            sum += static_cast<uint32_t>(sjpeg_internal::elem_load_u8(row + static_cast<long long>(x) * a.pix_step, a.kind, a.pscale[c], a.pbias[c]));
          }
        }
        acc[j][c] = sum;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[j][c] = sjpeg_internal::reduce_round(acc[j][c], S);
  }
  // whole dwords of the reduced row; the last group's may reach into the row's padding, never past it
  uint8_t* const out = d.dst + static_cast<size_t>(gy) * d.dst_stride;
  if (a.channels == 1) {
    *(GlobalOut)(out + static_cast<size_t>(gx) * 4) = acc[0][0] | (acc[1][0] << 8) | (acc[2][0] << 16) | (acc[3][0] << 24);
    return;
  }
  const uint32_t o0 = acc[0][0] | (acc[0][1] << 8) | (acc[0][2] << 16) | (acc[1][0] << 24);
  const uint32_t o1 = acc[1][1] | (acc[1][2] << 8) | (acc[2][0] << 16) | (acc[2][1] << 24);
  const uint32_t o2 = acc[2][2] | (acc[3][0] << 8) | (acc[3][1] << 16) | (acc[3][2] << 24);
  const unsigned at = static_cast<unsigned>(gx) * 12u;
  GlobalOut const q = (GlobalOut)(out + at);
  if (at + 12u <= d.dst_stride) {
    q[0] = o0; q[1] = o1; q[2] = o2;
  } else {
    q[0] = o0;                                               // (at < 3 w2 <= dst_stride: the group has a pixel)
    if (at + 8u <= d.dst_stride) q[1] = o1;
  }
}

__global__ __launch_bounds__(256) void reduce_ragged_kernel(const ReduceArgs a) {
  const unsigned wg = blockIdx.x;
  int lo = 0, hi = a.nframes - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.frames[mid].tile_base <= wg) lo = mid; else hi = mid - 1;
  }
  const ReduceFrame d = a.frames[lo];
  const unsigned item = (wg - d.tile_base) * 256u + threadIdx.x;
  const unsigned gy = item / static_cast<unsigned>(d.groups);
  if (gy >= static_cast<unsigned>(d.h2)) return;
  const int gx = static_cast<int>(item - gy * static_cast<unsigned>(d.groups));
  switch (d.s) {
    case 1: reduce_group<1>(a, d, gx, static_cast<int>(gy)); break;
    case 2: reduce_group<2>(a, d, gx, static_cast<int>(gy)); break;
    case 3: reduce_group<3>(a, d, gx, static_cast<int>(gy)); break;
    case 4: reduce_group<4>(a, d, gx, static_cast<int>(gy)); break;
    case 5: reduce_group<5>(a, d, gx, static_cast<int>(gy)); break;
    case 6: reduce_group<6>(a, d, gx, static_cast<int>(gy)); break;
    case 7: reduce_group<7>(a, d, gx, static_cast<int>(gy)); break;
    default: reduce_group<8>(a, d, gx, static_cast<int>(gy)); break;
  }
}

const char* yuv_format_name(int format) {
  switch (format) {
    case SJPEG_HIP_SRC_YUV444: return "SJPEG_HIP_SRC_YUV444";
    case SJPEG_HIP_SRC_YUV420: return "SJPEG_HIP_SRC_YUV420";
    case SJPEG_HIP_SRC_NV12: return "SJPEG_HIP_SRC_NV12";
    case SJPEG_HIP_SRC_NV21: return "SJPEG_HIP_SRC_NV21";
    default: return "this format";
  }
}

// a format the kernel reads: every RGB-like row of the table and the gray ones
bool reducible(const sjpeg_internal::SourceLayout& L) { return L.rgb_like || (L.planes == 1 && L.implied == SJPEG_HIP_YUV400); }

}  // namespace

namespace sjpeg_internal {

int reduce_plan(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const uint8_t* factors,
                ReducePlan* plan) {
  const SourceLayout* const L = source_layout(format);
  if (L == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": unknown source format");
  if (nframes < 1 || nframes > 65535) return set_error(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
  for (int f = 0; f < nframes; ++f) {
    const int s = factors != nullptr ? factors[f] : 1;
    if (s < 1 || s > kReduceMax) {
      return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": factor " + std::to_string(s) + " is not one of 1..8");
    }
  }
  if (!reducible(*L)) {
    return set_error(SJPEG_HIP_EINVAL, who + ": " + yuv_format_name(format) + " pictures are not reduced (a factor above 1 takes an RGB-like or a gray format)");
  }
  const int channels = L->rgb_like ? 3 : 1;
  plan->format = format;
  plan->reduced_format = channels == 3 ? SJPEG_HIP_SRC_RGB : SJPEG_HIP_SRC_GRAY;
  plan->frames.assign(static_cast<size_t>(nframes), ReduceFrame());
  size_t at = 0;
  unsigned long long tiles = 0;
  for (int f = 0; f < nframes; ++f) {
    const sjpeg_hip_ragged_frame& fr = frames[f];
    ReduceFrame& d = plan->frames[f];
    memset(&d, 0, sizeof(d));
    if (fr.width < 1 || fr.height < 1 || fr.width > 65535 || fr.height > 65535) {
      return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": bad dimensions " + std::to_string(fr.width) + "x" + std::to_string(fr.height));
    }
    const uint8_t* planes[3];
    long long rows[3];
    layout_planes(*L, fr.plane, fr.row_stride, nullptr, planes, rows, nullptr);
    d.src = static_cast<const uint8_t*>(fr.plane[0]);
    d.row_stride = rows[0];
    long long g = 0, b = 0;
    if (channels == 3) layout_rgb_offsets(*L, fr.plane, &g, &b);
    d.off[0] = channels == 3 ? L->r_off : 0; d.off[1] = g; d.off[2] = b;
    d.s = factors != nullptr ? factors[f] : 1;
    d.W = fr.width; d.H = fr.height;
    d.w2 = reduced_dim(fr.width, d.s); d.h2 = reduced_dim(fr.height, d.s);
    d.groups = (d.w2 + 3) / 4;
    d.dst_stride = static_cast<unsigned>(reduced_row_stride(d.w2, channels));
    d.dst = reinterpret_cast<uint8_t*>(at);                       // (from the buffer's start: engine_reduce adds it)
    d.tile_base = static_cast<unsigned>(tiles);
    at += reduced_picture_bytes(d.w2, d.h2, channels);
    tiles += (static_cast<unsigned long long>(d.groups) * static_cast<unsigned long long>(d.h2) + 255ull) / 256ull;
    if (tiles > 0x7fffffffull) return set_error(SJPEG_HIP_EINVAL, who + ": frame " + std::to_string(f) + ": the batch has too many tiles for one launch");
  }
  plan->bytes = at;
  plan->tiles = static_cast<unsigned>(tiles);
  return 0;
}

void reduce_plan_frames(const ReducePlan& plan, const sjpeg_hip_ragged_frame* frames, uint8_t* base, sjpeg_hip_ragged_frame* out) {
  for (size_t f = 0; f < plan.frames.size(); ++f) {
    const ReduceFrame& d = plan.frames[f];
    sjpeg_hip_ragged_frame r;
    memset(&r, 0, sizeof(r));
    r.plane[0] = base + reinterpret_cast<uintptr_t>(d.dst);
    r.row_stride[0] = static_cast<int64_t>(d.dst_stride);
    r.width = d.w2; r.height = d.h2;
    r.out_offset = frames[f].out_offset; r.out_capacity = frames[f].out_capacity;
    out[f] = r;
  }
}

int reduce_ragged_launch(int format, const float* pscale, const float* pbias, const ReduceFrame* d_frames, int nframes, unsigned tiles,
                         hipStream_t st) {
  const SourceLayout& L = *source_layout(format);
  ReduceArgs a;
  memset(&a, 0, sizeof(a));
  a.frames = d_frames;
  a.nframes = nframes;
  a.kind = L.kind;
  a.channels = L.rgb_like ? 3 : 1;
  a.pix_step = L.plane[0].step * L.esz;
  a.cls = L.kind != kElemU8 ? kReduceElems : (L.one_pitch || a.channels == 1) ? kReducePlanes : L.pix_step == 3 ? kReducePacked3 : kReducePacked4;
  for (int c = 0; c < 3; ++c) { a.pscale[c] = pscale[c]; a.pbias[c] = pbias[c]; }
  hipLaunchKernelGGL(reduce_ragged_kernel, dim3(tiles), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace sjpeg_internal

extern "C" {

int sjpeg_hip_reduced_size(int width, int height, int factor, int* reduced_width, int* reduced_height) {
  static const std::string who = "sjpeg_hip_reduced_size";
  if (reduced_width == nullptr || reduced_height == nullptr) return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": reduced_width or reduced_height == NULL");
  if (factor < 1 || factor > SJPEG_HIP_REDUCE_MAX) return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": factor " + std::to_string(factor) + " is not one of 1..8");
  if (width < 1 || height < 1 || width > 65535 || height > 65535) {
    return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, who + ": bad dimensions " + std::to_string(width) + "x" + std::to_string(height));
  }
  *reduced_width = sjpeg_internal::reduced_dim(width, factor);
  *reduced_height = sjpeg_internal::reduced_dim(height, factor);
  return 0;
}

size_t sjpeg_hip_reduce_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames, const uint8_t* factors) {
  if (frames == nullptr) return 0;
  try {
    sjpeg_internal::ReducePlan plan;
    if (sjpeg_internal::reduce_plan("sjpeg_hip_reduce_ragged_bytes", format, nframes, frames, factors, &plan) != 0) return 0;
    return plan.bytes;
  } catch (...) {
    return 0;
  }
}

}  // extern "C"
