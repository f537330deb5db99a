// ragged_aux.h -- what the ragged riskiness and sharp conversions (riskiness.hip, sharp_yuv.hip) share with the
// engine's ragged entry points (scan_engine.hip).  Internal: not part of include/sjpeg_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "sjpeg_hip.h"

namespace sjpeg_internal {

// the channel layout of a packed RGB / BGRA / RGBA source (the riskiness stencil and the sharp conversion start from
// these); false for any other format
inline bool rgb_layout(int format, int* pix_step, int* r_off, int* g_off, int* b_off) {
  switch (format) {
    case SJPEG_HIP_SRC_RGB: *pix_step = 3; *r_off = 0; *g_off = 1; *b_off = 2; return true;
    case SJPEG_HIP_SRC_BGRA: *pix_step = 4; *r_off = 2; *g_off = 1; *b_off = 0; return true;
    case SJPEG_HIP_SRC_RGBA: *pix_step = 4; *r_off = 0; *g_off = 1; *b_off = 2; return true;
    default: return false;
  }
}

// ---- ragged riskiness: one descriptor per frame; a workgroup finds its frame by a binary search over wg_base
struct RiskFrame {
  const uint8_t* rgb;                    // row 0
  long long row_stride;                  // may be negative
  int W, H;
  int bands, cols;                       // the frame's workgroups: cols x bands (none when W or H < 2)
  unsigned wg_base, pad;                 // its first workgroup in the flat grid
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
int risk_ragged_launch(int format, const RiskFrame* d_frames, int nframes, unsigned total_wgs,
                       const uint8_t* d_table, uint64_t* d_sums, hipStream_t st);

// ---- ragged sharp conversion (sjpeg_hip_sharp_yuv_ragged); the descriptors go into the workspace through `up`
using UploadFn = int (*)(void* ctx, void* d_dst, const void* src, size_t bytes, hipStream_t st);
size_t sharp_ragged_workspace(int nframes, const sjpeg_hip_ragged_frame* frames);
int sharp_ragged_run(int format, int nframes, const sjpeg_hip_ragged_frame* frames, uint8_t* const* d_y,
                     uint8_t* const* d_u, uint8_t* const* d_v, void* d_workspace, size_t workspace_size,
                     hipStream_t st, UploadFn up, void* up_ctx, std::string* err);

}  // namespace sjpeg_internal
