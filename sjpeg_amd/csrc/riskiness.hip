// riskiness.hip -- the stencil behind SjpegRiskiness() / SJPEG_YUV_AUTO on gfx950.
//
// Reference: /root/reference/src/jpeg_tools.cc:170-236 (SjpegRiskiness) and
// src/colors_rgb.cc:1085-1122 (pixel -> 7x7x7 YUV cell index).  Every pixel becomes the index of
// its cell; every position (i, j) with a right and a lower neighbour looks three pairs of
// cells up in a 343 x 343 score table and the picture's verdict is made of three sums.  The
// score table is trained data of the reference (src/score_7.cc); it ships beside the library as
// riskiness.bin (riskiness.NOTICE), or comes from sjpeg_hip_set_riskiness_table / SJPEG_HIP_RISKINESS_TABLE.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sjpeg_hip.h"
#include "ragged_aux.h"

namespace {

constexpr int kCells = 7;                         // kRGBSize
constexpr int kCells3 = kCells * kCells * kCells;
constexpr int kNoiseLevel = 4;

__device__ __forceinline__ uint32_t clip8(int v) { return v < 0 ? 0u : v > 255 ? 255u : static_cast<uint32_t>(v); }
__device__ __forceinline__ uint32_t cell(uint32_t v) { return (v * (0x0101u * (kCells - 1))) >> 16; }   // ~ v * 6 / 255

__device__ __forceinline__ int yuv_index(const uint8_t* p, long long ro, long long go, long long bo) {   // colors_rgb.cc:1104-1112
  const int r = p[ro], g = p[go], b = p[bo];
  const uint32_t y = cell(static_cast<uint32_t>((19595 * r + 38469 * g + 7471 * b + 32768) >> 16));
  const uint32_t u = cell(clip8(128 + ((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16)));
  const uint32_t v = cell(clip8(128 + ((32768 * r - 27439 * g - 5329 * b + 32768) >> 16)));
  return static_cast<int>(y + u * kCells + v * kCells * kCells);
}

// the ragged form's samples: bytes as they are, or float elements through the engine's pixel transform (pixel_elem.h)
__device__ __forceinline__ int yuv_index_elem(const uint8_t* p, long long ro, long long go, long long bo, int kind, const float* s, const float* t) {
  if (kind == sjpeg_internal::kElemU8) return yuv_index(p, ro, go, bo);
  const uint8_t px[3] = {static_cast<uint8_t>(sjpeg_internal::elem_load_u8(p + ro, kind, s[0], t[0])),
                         static_cast<uint8_t>(sjpeg_internal::elem_load_u8(p + go, kind, s[1], t[1])),
                         static_cast<uint8_t>(sjpeg_internal::elem_load_u8(p + bo, kind, s[2], t[2]))};
  return yuv_index(px, 0, 1, 2);
}

struct RiskArgs {
  const uint8_t* rgb;
  long long row_stride, frame_stride;
  int pix_step;
  long long r_off, g_off, b_off;                  // (64 bits: the planes of planar RGB lie anywhere)
  int W, H;
  const uint8_t* table;                           // [343 * 343]
  unsigned long long* out;                        // [nframes][3]: score_sum, score_num, gray_num
  int ekind;                                      // ragged form: element kind (pixel_elem.h) and the pixel transform
  float pscale[3], pbias[3];                      // (per channel R, G, B)
};

// One workgroup = 256 columns x a BAND of rows (the grid's y dimension cuts the picture into at most 64 bands): a
// thread walks down its column, keeps the cell index of the pixel it stands on for the next row (two conversions per
// position instead of three), and the three sums leave the workgroup as ONE atomic each.  (Round 3's kernel was one
// row per workgroup and three 64-bit atomics per WAVE on the same three addresses: 390 000 serialised atomics for a
// 4K picture, 4.3 ms of the 5.3 ms SjpegCompress() took.)
__global__ __launch_bounds__(256) void risk_scan(const RiskArgs a) {
  __shared__ unsigned long long part[4][3];
  const int frame = blockIdx.z;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int rows = a.H - 1;                                    // positions (i, j), j = 1 .. H - 1 (the row below)
  const int per = (rows + static_cast<int>(gridDim.y) - 1) / static_cast<int>(gridDim.y);
  const int j0 = 1 + static_cast<int>(blockIdx.y) * per, j1 = min(j0 + per, a.H);
#define RISK_INDEX(p) yuv_index(p, a.r_off, a.g_off, a.b_off)
#include "risk_scan_body.inc"
#undef RISK_INDEX
}

// The ragged form: a flat grid over the batch's workgroups; a workgroup finds its frame by a binary search over the
// frames' first workgroups, then runs the same body on a copy of the arguments rebased to that frame.
__global__ __launch_bounds__(256) void risk_scan_ragged(const RiskArgs common, const sjpeg_internal::RiskFrame* frames, int nframes) {
  __shared__ unsigned long long part[4][3];
  const unsigned wg = blockIdx.x;
  int lo = 0, hi = nframes - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (frames[mid].wg_base <= wg) lo = mid; else hi = mid - 1;
  }
  const sjpeg_internal::RiskFrame d = frames[lo];
  RiskArgs a = common;
  a.rgb = d.rgb; a.row_stride = d.row_stride; a.frame_stride = 0;
  a.g_off = d.g_off; a.b_off = d.b_off;
  a.W = d.W; a.H = d.H;
  a.out = common.out + static_cast<size_t>(lo) * 3;
  const unsigned local = wg - d.wg_base;
  const int frame = 0;
  const int i = (local % static_cast<unsigned>(d.cols)) * 256 + threadIdx.x;
  const int rows = a.H - 1;
  const int per = (rows + d.bands - 1) / d.bands;
  const int j0 = 1 + static_cast<int>(local / static_cast<unsigned>(d.cols)) * per, j1 = min(j0 + per, a.H);
#define RISK_INDEX(p) yuv_index_elem(p, a.r_off, a.g_off, a.b_off, a.ekind, a.pscale, a.pbias)
#include "risk_scan_body.inc"
#undef RISK_INDEX
}

}  // namespace

extern "C" int sjpeg_hip_riskiness_sums(const sjpeg_hip_source* src, int width, int height, int nframes,
                                        const uint8_t* d_table, uint64_t* d_sums, void* stream) {
  if (src == nullptr || src->plane[0] == nullptr || d_table == nullptr || d_sums == nullptr ||
      width <= 0 || height <= 0 || nframes <= 0 || nframes > 65535 || height > 65536) {
    return SJPEG_HIP_EINVAL;
  }
  RiskArgs a;
  memset(&a, 0, sizeof(a));
  // (no engine, no pixel transform: float planes go through sjpeg_hip_riskiness_ragged_src)
  const sjpeg_internal::SourceLayout* const L = sjpeg_internal::source_layout(src->format);
  if (L != nullptr && L->kind != sjpeg_internal::kElemU8) {
    return sjpeg_internal::set_error(SJPEG_HIP_EINVAL, std::string("sjpeg_hip_riskiness_sums: ") +
                                                           (L->one_pitch ? "SJPEG_HIP_SRC_RGB_PLANAR_F32 / _F16 / _BF16" : "SJPEG_HIP_SRC_RGB_F* / _RGBA_F* / _GRAY_F*") +
                                                           " need an engine's pixel transform: use sjpeg_hip_riskiness_ragged_src");
  }
  if (L == nullptr || !L->rgb_like) return SJPEG_HIP_EINVAL;
  const bool faulty = sjpeg_internal::layout_fault(*L, width, src->plane, src->row_stride, src->frame_stride, sjpeg_internal::kUniformChecks).rule != 0;
  if (L->one_pitch && faulty) return SJPEG_HIP_EINVAL;      // (the packed formats' strides are the caller's word here, as ever)
  a.pix_step = L->pix_step; a.r_off = L->r_off;
  sjpeg_internal::layout_rgb_offsets(*L, src->plane, &a.g_off, &a.b_off);
  hipStream_t st = static_cast<hipStream_t>(stream);
  a.rgb = static_cast<const uint8_t*>(src->plane[0]);
  a.row_stride = src->row_stride[0]; a.frame_stride = src->frame_stride[0];
  a.W = width; a.H = height;
  a.table = d_table;
  a.out = reinterpret_cast<unsigned long long*>(d_sums);
  if (hipMemsetAsync(d_sums, 0, static_cast<size_t>(nframes) * 3 * sizeof(uint64_t), st) != hipSuccess) return SJPEG_HIP_ERUNTIME;
  if (width < 2 || height < 2) return 0;                       // no (i, j) has both neighbours
  const int bands = height - 1 < 64 ? height - 1 : 64;
  hipLaunchKernelGGL(risk_scan, dim3((width - 1 + 255) / 256, bands, nframes), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : SJPEG_HIP_ERUNTIME;
}

namespace sjpeg_internal {

int risk_ragged_launch(int format, const float* pscale, const float* pbias, const RiskFrame* d_frames, int nframes, unsigned total_wgs,
                       const uint8_t* d_table, uint64_t* d_sums, hipStream_t st) {
  RiskArgs a;
  memset(&a, 0, sizeof(a));
  const SourceLayout* const L = source_layout(format);
  if (L == nullptr || !L->rgb_like) return SJPEG_HIP_EINVAL;
  a.pix_step = L->pix_step; a.r_off = L->r_off; a.g_off = L->g_off; a.b_off = L->b_off;   // (g_off, b_off: the frames' own are read)
  a.ekind = L->kind;
  for (int c = 0; c < 3; ++c) { a.pscale[c] = pscale[c]; a.pbias[c] = pbias[c]; }
  a.table = d_table;
  a.out = reinterpret_cast<unsigned long long*>(d_sums);
  if (hipMemsetAsync(d_sums, 0, static_cast<size_t>(nframes) * 3 * sizeof(uint64_t), st) != hipSuccess) return SJPEG_HIP_ERUNTIME;
  if (total_wgs == 0) return 0;                                // every frame 1 x N or N x 1
  hipLaunchKernelGGL(risk_scan_ragged, dim3(total_wgs), dim3(256), 0, st, a, d_frames, nframes);
  return hipGetLastError() == hipSuccess ? 0 : SJPEG_HIP_ERUNTIME;
}

}  // namespace sjpeg_internal
