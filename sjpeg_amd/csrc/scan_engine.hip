// scan_engine.hip -- the MI355X (gfx950 / CDNA4) scan engine behind include/sjpeg_hip.h.
//
// Replaces the reference's per-MCU hot loop (Encoder::SinglePassScan,
// src/enc.cc:276-307) for whole frames / batches of frames resident in HBM.
// Written for wave64 + LDS from scratch; integer-only, no MFMA (8-point integer butterflies
// and a per-coefficient reciprocal multiply are not a dense contraction).
//
// Pipeline per batch (all on one stream, no host round trip):
//
//   K1 scan_segments   one workgroup per SEGMENT (= run of consecutive MCUs of one frame):
//        P1 colour  : RGB rows -> level-shifted Y/Cb/Cr int16 blocks in LDS
//                     (reference: src/colors_rgb.cc:785-879, edge replication
//                      src/colors_rgb.cc:1212-1232 == coordinate clamping)
//        P2 block   : one THREAD per 8x8 block, whole block in registers:
//                     AverageExtraLuma fix-up (src/encoders.cc:107-125), forward DCT
//                     (src/fdct.cc:67-144,174-209,596-609), quantization
//                     (src/quantize.cc:119-121,288-320) -> zig-zag int16 + non-zero mask
//        P3 entropy : DC prediction (src/entropy.cc:133-150) through LDS, per-thread
//                     run/size Huffman coding (src/entropy.cc:161-198), workgroup prefix
//                     scan of block bit lengths, MSB-first bit packing into an LDS window
//        P4 flush   : coalesced store of the segment's packed words + its bit length
//   K2 scan_seg_offsets   per frame: exclusive scan of segment bit lengths
//   K3 concat_chunks      gather: every 4 KiB chunk of the frame's single continuous
//                         (un-stuffed) bit stream is assembled from the segments at their
//                         bit offsets; final byte padded with 1-bits
//                         (src/bit_writer.cc:107-116); counts 0xFF bytes per chunk
//   K4 scan_chunk_offsets per frame: exclusive scan of 0xFF counts, final size
//   K5 stuff_chunks       0xFF -> 0xFF00 byte stuffing (src/bit_writer.h:172-196) into
//                         the caller's output slot, header in front, FF D9 behind
//                         (launches that are not fused: stuff_chunks_wave, one wave per chunk)
//
// The reference never emits restart markers, so bit-exactness needs exactly this
// bit-level stitching.
//
// This file is the one unit that defines and launches those kernels (scan_device.h, scan_segments.h, scan_reduce.h,
// stitch_kernels.h, included below), and holds what every launch needs: table digestion, the engine's life and
// setters, the upload ring and stream ordering, the uniform entries (statistics, encode, bands, adaptation) and the
// ragged launch layer (ragged_encode, ragged_analysis, the counted bits).  The flows that only CALL those launches are
// host files over engine.h: batch_flow.cc (frames of one size: lanes, parts), ragged_flows.cc (frames of different sizes:
// methods, mode groups, packed output), engine_pictures.cc (reduce, resize, sheets, colour).  A kernel is launched only
// from the unit that defines it -- the build has no relocatable device code -- so what a flow needs of a kernel here is a
// host function of sjpeg_internal (adapt_ragged, adapt_decide, scatter_sizes); and the kernels' parameter structs stay in
// this file's anonymous namespace: the flows name a source format, the launch layer derives the rest.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <type_traits>
#include <string>
#include <chrono>
#include <vector>
#include <functional>

#include "sjpeg_hip.h"
#include "jpeg_host.h"
#include "engine.h"
#include "stuff_wave_body.h"

using namespace sjpeg_internal;      // (the engine's types and the launch layer's declarations: engine.h)

namespace {

#include "scan_device.h"
#include "scan_segments.h"
#include "scan_reduce.h"
#include "stitch_kernels.h"

// ------------------------------------------------------------------------------------
// host side

thread_local std::string g_last_error;

}  // namespace

// sjpeg_hip_last_error() of the calling thread (fail() and HIP_TRY of engine.h end here)
int sjpeg_internal::set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

bool sjpeg_internal::frame_geo(int W, int H, int mode, FrameGeo* g) {
  if (W <= 0 || H <= 0 || W > 65535 || H > 65535) return false;   // src/enc.cc:406
  switch (mode) {
    case SJPEG_HIP_YUV420: g->bpm = 6; g->px = 16; g->seg_mcus = Geo<SJPEG_HIP_YUV420>::kSegMcus; break;
    case SJPEG_HIP_YUV444: g->bpm = 3; g->px = 8; g->seg_mcus = Geo<SJPEG_HIP_YUV444>::kSegMcus; break;
    case SJPEG_HIP_YUV400: g->bpm = 1; g->px = 8; g->seg_mcus = Geo<SJPEG_HIP_YUV400>::kSegMcus; break;
    default: return false;
  }
  g->mb_w = (W + g->px - 1) / g->px;                              // src/enc.cc:410-411
  g->mb_h = (H + g->px - 1) / g->px;
  g->n_mcus = g->mb_w * g->mb_h;
  g->nseg = (g->n_mcus + g->seg_mcus - 1) / g->seg_mcus;
  g->slot_words = ((static_cast<uint32_t>(g->seg_mcus) * g->bpm * kMaxBlockBits + 31) / 32 + 2 + 3) & ~3u;   // (whole 16-byte units)
  return true;
}

namespace {

// the quantizer part of DevTables (its first KiB)
void digest_quant(const sjpeg_hip_scan_tables* t, uint4 (*q)[32]) {
  for (int c = 0; c < 2; ++c) {
    for (int j = 0; j < 64; ++j) {
      uint4& e = q[c][j >> 1];
      const uint32_t iq = t->iquant[c][j], biq = static_cast<uint32_t>(t->bias[c][j]) * iq;
      const uint32_t qv = t->quant[c][j];
      if ((j & 1) == 0) { e.x = iq; e.y = biq; e.w = qv; } else { e.x |= iq << 16; e.z = biq; e.w |= qv << 16; }
    }
  }
}

void digest_tables(const sjpeg_hip_scan_tables* t, DevTables* d) {
  digest_quant(t, d->q);
  memset(d->pad_a, 0, sizeof(d->pad_a));
  memcpy(d->dc, t->dc_codes, sizeof(d->dc));
  memcpy(d->ac, t->ac_codes, sizeof(d->ac));
  memcpy(d->tlen, t->trellis_len, sizeof(d->tlen));
  // the lean walk's merged code words and the level bound under which it is provably in place
  // (scan_segments.h, P3): a symbol of run 0 must not emit more than 16 bits
  for (int c = 0; c < 2; ++c) {
    int n_safe = 0;
    for (int n = 1; n <= 10; ++n) {
      const uint32_t len0 = t->ac_codes[c][n] & 0xffu;            // symbol (run 0, size n); 0 = not in the table
      if (len0 + n > 16u) break;
      n_safe = n;
    }
    {
      const uint32_t zrl = t->ac_codes[c][0xf0];
      const uint32_t zl = zrl & 0xffu;
      unsigned long long v = 0;
      d->zrlpat[c][0] = make_uint4(0, 0, 0, 0);
      for (uint32_t k = 1; k <= 3; ++k) {
        v = (v << zl) | (zrl >> 16);
        const unsigned long long left = (zl == 0u) ? 0ull : v << (64u - k * zl);
        d->zrlpat[c][k] = make_uint4(static_cast<uint32_t>(left >> 32), static_cast<uint32_t>(left), k * zl, 0u);
      }
    }
    const uint32_t bad = ~((1u << n_safe) - 1u) & 0x7fffu;
    d->safe_mask[c] = bad | (bad << 16);
    d->eob_zrl[c][0] = t->ac_codes[c][0x00];
    d->eob_zrl[c][1] = t->ac_codes[c][0xf0];
    for (int n = 1; n <= 10; ++n) {
      for (int run = 0; run < 16; ++run) {
        const uint32_t cw = t->ac_codes[c][(run << 4) | n];
        const uint32_t len = cw & 0xffu, code = cw >> 16;
        d->acm[c][run][10 - n] = len == 0u ? 0u : ((code << n) | ((len + n) << 27));
      }
    }
  }
}

template <int KIND, int SRC>
int launch_scan_src(int mode, dim3 grid, hipStream_t st, const ScanArgs& a) {
  static const int kLdsPad = getenv("SJPEG_HIP_LDS_PAD") ? atoi(getenv("SJPEG_HIP_LDS_PAD")) : 0;  // occupancy experiments
  const int lds = kLdsPad;                        // (the kernel's own LDS is a static array)
  switch (mode) {
    case SJPEG_HIP_YUV420:
      hipLaunchKernelGGL((scan_segments<SJPEG_HIP_YUV420, KIND, SRC>), grid, dim3(kScanThreads), lds, st, a);
      break;
    case SJPEG_HIP_YUV444:
      hipLaunchKernelGGL((scan_segments<SJPEG_HIP_YUV444, KIND, SRC>), grid, dim3(kScanThreads), lds, st, a);
      break;
    default:
      hipLaunchKernelGGL((scan_segments<SJPEG_HIP_YUV400, KIND, SRC>), grid, dim3(kScanThreads), lds, st, a);
      break;
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

template <int KIND>
int launch_scan(int mode, int src_class, dim3 grid, hipStream_t st, const ScanArgs& a) {
  switch (src_class) {
    case kSrcRgb24: return launch_scan_src<KIND, kSrcRgb24>(mode, grid, st, a);
    case kSrcRgbx32: return launch_scan_src<KIND, kSrcRgbx32>(mode, grid, st, a);
    case kSrcRgbPlanar: return launch_scan_src<KIND, kSrcRgbPlanar>(mode, grid, st, a);
    // (float planes; the kinds that read no pixel have no twin of their own: the byte-planar class's code serves)
    case kSrcRgbPlanarF: return launch_scan_src<KIND, (KIND == kKindEncodeReplay || KIND == kKindStatsCoef) ? kSrcRgbPlanar : kSrcRgbPlanarF>(mode, grid, st, a);
    default: return launch_scan_src<KIND, kSrcPlanes>(mode, grid, st, a);
  }
}

sjpeg_hip_source rgb_source(const void* d_rgb, int64_t row_stride, int64_t frame_stride) {
  sjpeg_hip_source s;
  memset(&s, 0, sizeof(s));
  s.format = SJPEG_HIP_SRC_RGB;
  s.plane[0] = d_rgb; s.row_stride[0] = row_stride; s.frame_stride[0] = frame_stride;
  return s;
}

}  // namespace

// the event behind everything the engine has put on its own (stitch) stream so far
int sjpeg_internal::side_mark(sjpeg_hip_engine* e) {
  if (e->side_pending && !e->side_recorded) {
    HIP_TRY(hipEventRecord(e->side_done, e->side));
    e->side_recorded = true;
  }
  return 0;
}

// Orders this call after everything the engine was asked to do on another stream.
int sjpeg_internal::order_on_stream(sjpeg_hip_engine* e, hipStream_t st) {
  if (e->last_stream_valid && e->last_stream != st) {
    // The previous call's stream belongs to the caller and may be gone by now (sjpeg_hip.h asks for
    // it to outlive the engine's next call, but a destroyed handle must not wedge the engine): if
    // the event hand-over fails, wait for the whole device instead and carry on.
    bool ordered = (e->cross_ev != nullptr) || hipEventCreateWithFlags(&e->cross_ev, hipEventDisableTiming) == hipSuccess;
    ordered = ordered && hipEventRecord(e->cross_ev, e->last_stream) == hipSuccess &&
              hipStreamWaitEvent(st, e->cross_ev, 0) == hipSuccess;
    if (ordered && e->side_pending) ordered = side_mark(e) == 0 && hipStreamWaitEvent(st, e->side_done, 0) == hipSuccess;
    if (!ordered) {
      (void)hipGetLastError();                     // clear the sticky error of the stale handle
      e->last_stream_valid = false;
      e->tables_held_at = nullptr; e->header_held_at = nullptr;   // (their streams may be the stale one)
      HIP_TRY(hipDeviceSynchronize());
    }
  }
  e->last_stream = st;
  e->last_stream_valid = true;
  return 0;
}

// the call is ordered behind the engine's earlier work (another stream, pipelined mode's stitch stream)
int sjpeg_internal::ragged_ordered(sjpeg_hip_engine* e, hipStream_t st) {
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = order_on_stream(e, st)) return rc;
  if (e->side_pending) {
    if (int rc = side_mark(e)) return rc;
    HIP_TRY(hipStreamWaitEvent(st, e->side_done, 0));
  }
  return 0;
}

namespace {
// The copy of a staged upload: a kernel reads the engine's pinned block over the bus and writes device memory.  Not
// hipMemcpyAsync: that call took 6-9 ms ONCE per process -- the first copy it is asked for while kernels of the same
// stream are still running (the second default-parameter batch call of a process; now and then a later one) --, the
// "6-8 ms call some tens of calls in" of round 4, named in round 5 by the marks of SJPEG_HIP_BATCH_DEBUG=2
// (profiles/r05/slow_call.txt: `upload: hipMemcpyAsync 6920 us`).  A kernel stays on the stream's own queue: no copy
// engine, no hand-over between queues, and a launch costs the host less than the copy call did.
__global__ __launch_bounds__(256) void stage_copy_kernel(uint8_t* dst, const uint8_t* src, size_t bytes) {
  const size_t n16 = bytes >> 4;
  const uint4* const s4 = reinterpret_cast<const uint4*>(src);
  uint4* const d4 = reinterpret_cast<uint4*>(dst);
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n16; i += static_cast<size_t>(gridDim.x) * 256) d4[i] = s4[i];
  if (blockIdx.x == 0 && threadIdx.x < (bytes & 15u)) dst[(n16 << 4) + threadIdx.x] = src[(n16 << 4) + threadIdx.x];
}

}  // namespace

// bytes between two places the DEVICE can address (device memory, mapped pinned host memory), by that kernel; the
// runtime's copy where the addresses do not allow 16-byte accesses
int sjpeg_internal::copy_by_kernel(void* dst, const void* src, size_t bytes, hipStream_t st, hipMemcpyKind fallback_kind, const void* fallback_src, void* fallback_dst) {
  if (bytes == 0) return 0;
  if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15u) != 0 || dst == nullptr || src == nullptr) {
    HIP_TRY(hipMemcpyAsync(fallback_dst, fallback_src, bytes, fallback_kind, st));
    return 0;
  }
  const size_t n16 = bytes >> 4;
  const unsigned blocks = static_cast<unsigned>(n16 >= 256 * 64 ? 64 : (n16 + 255) / 256 + (n16 == 0 ? 1 : 0));
  hipLaunchKernelGGL(stage_copy_kernel, dim3(blocks), dim3(256), 0, st, static_cast<uint8_t*>(dst), static_cast<const uint8_t*>(src), bytes);
  HIP_TRY(hipGetLastError());
  return 0;
}

// dst <- src on the stream, through one of the engine's pinned blocks when the copy is not tiny (see sjpeg_hip_engine::stage)
int sjpeg_internal::upload(sjpeg_hip_engine* e, void* dst, const void* src, size_t bytes, hipStream_t st) {
  // (for a very large one -- the per-frame tables of a batch of tens of thousands of frames -- the runtime's pinning is
  // small beside the copy, and four pinned blocks of that size would not be)
  if (bytes == 0) return 0;
  if (bytes > (static_cast<size_t>(8) << 20)) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
    return 0;
  }
  sjpeg_hip_engine::Stage& s = e->stage[e->stage_next];
  e->stage_next = (e->stage_next + 1) & 3;
  dbg_mark("upload: begin");
  if (s.busy) { HIP_TRY(hipEventSynchronize(s.ev)); s.busy = false; }       // (four uploads ago: long done)
  dbg_mark("upload: block free");
  if (s.cap < bytes) {
    // ALL four blocks grow together, to a power of two: hipHostFree + hipHostMalloc of one block takes milliseconds,
    // and blocks that grew one by one -- whenever the ring brought a small block to a large upload -- were the
    // "6-8 ms call some tens of calls in" of the default-parameter batch path (round 4; named in round 5 by the
    // library's own host timeline: the second call's statistics launch, profiles/r05/slow_call.txt).  Now the first
    // upload of a size class pays for the four, once.
    size_t want = static_cast<size_t>(256) << 10;
    while (want < bytes) want <<= 1;
    for (auto& g : e->stage) {
      if (g.cap >= want) continue;
      if (g.busy) { HIP_TRY(hipEventSynchronize(g.ev)); g.busy = false; }
      if (g.p) (void)hipHostFree(g.p);
      g.p = nullptr; g.dp = nullptr; g.cap = 0;
      if (hipHostMalloc(&g.p, want, hipHostMallocMapped) != hipSuccess) { g.p = nullptr; return fail(SJPEG_HIP_ENOMEM, "hipHostMalloc(upload block) failed"); }
      g.cap = want;
      // (the address the device reads the block at; without one the copy falls back to the runtime's)
      if (hipHostGetDevicePointer(&g.dp, g.p, 0) != hipSuccess) { (void)hipGetLastError(); g.dp = nullptr; }
    }
  }
  if (s.ev == nullptr && hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) != hipSuccess) { s.ev = nullptr; return fail(SJPEG_HIP_ERUNTIME, "hipEventCreate failed"); }
  dbg_mark("upload: block sized");
  memcpy(s.p, src, bytes);
  dbg_mark("upload: memcpy");
  hipStream_t const us = e->up_stream != nullptr ? e->up_stream : st;
  if (int rc = copy_by_kernel(dst, s.dp, bytes, us, hipMemcpyHostToDevice, s.p, dst)) return rc;
  dbg_mark("upload: copy launched");
  HIP_TRY(hipEventRecord(s.ev, us));
  dbg_mark("upload: hipEventRecord");
  s.busy = true;
  if (e->up_stream != nullptr) e->up_wait = s.ev;
  return 0;
}

// the call's stream waits for the early uploads (sjpeg_hip_engine::up_stream) in front of the kernel that reads them
int sjpeg_internal::sync_uploads(sjpeg_hip_engine* e, hipStream_t st) {
  if (e->up_wait != nullptr) {
    HIP_TRY(hipStreamWaitEvent(st, e->up_wait, 0));
    e->up_wait = nullptr;
  }
  return 0;
}

namespace {

// A batch coded in parts: where a part's per-frame tables / headers start in the engine's buffers (frames), and how many
// frames those buffers are for -- the parts' uploads must not land on each other.
inline int part_first_frame(const sjpeg_hip_engine* e) { return e->replay_total > 0 ? e->replay_first : 0; }
inline int part_total_frames(const sjpeg_hip_engine* e, int nframes) { return e->replay_total > 0 ? e->replay_total : nframes; }

// Segment scratch of an encode call, sized from the bytes the caller gives every frame (out_stride)
// instead of for the worst case: a frame's un-stuffed stream is never longer than its stuffed one, so
// `budget` words hold it whenever the frame fits its output slot -- and a frame that does not fit
// reports size 0 anyway.  Every segment has a slot of about three quarters of its share of the budget (the
// ordinary segment fits; K3 reads it without indirection); what a longer segment has beyond that, and
// the rows of the checked walk (scan_segments.h), come out of a per-frame pool.  Both are at most as
// long as the stream, hence 2 x budget.  budget_bytes == SIZE_MAX: worst case (bands, which have no
// output slot to go by).
struct SegPlan { uint32_t slot_words, pool_words; size_t ubuf_words; };
SegPlan seg_plan(const FrameGeo& g, size_t budget_bytes) {
  const size_t worst_total = static_cast<size_t>(g.nseg) * g.slot_words;
  size_t budget = budget_bytes == SIZE_MAX ? worst_total : budget_bytes / 4 + 16;
  if (budget > worst_total) budget = worst_total;
  SegPlan p;
  // (three quarters of a segment's share: at half of it the segments of an 8K 4:4:4 q90 frame -- 0.77 B per
  // pixel against slots of 0.75 -- went through the pool, K3's slow path, every other time)
  size_t sw = (budget * 3 / static_cast<size_t>(g.nseg) / 4 + 63) & ~size_t(63);
  const size_t floor_words = g.slot_words < 1024u ? g.slot_words : 1024u;
  if (sw < floor_words) sw = floor_words;
  if (sw > g.slot_words || budget >= worst_total) sw = g.slot_words;   // (worst-case budget: no segment is ever longer than its slot)
  p.slot_words = static_cast<uint32_t>(sw);
  size_t pool = (sw == g.slot_words ? budget : 2 * budget) + 64;
  if (pool > 0xfffffff0u) pool = 0xfffffff0u;      // (word offsets are 32 bit: 16 GiB per frame)
  p.pool_words = static_cast<uint32_t>(pool);
  p.ubuf_words = (budget + kChunkWords + 3) & ~size_t(3);
  return p;
}

// the engine's pixel transform into a launch's arguments (a->pone, one gray plane read as R, G and B: channel 0's thrice)
void put_transform(const sjpeg_hip_engine* e, ScanArgs* a) {
  for (int c = 0; c < 3; ++c) { a->pscale[c] = e->pscale[a->pone ? 0 : c]; a->pbias[c] = e->pbias[a->pone ? 0 : c]; }
}
// a format's fields of a launch's arguments (the float class's stay zero for the byte formats, which ignore them)
void layout_args(const SourceLayout& L, ScanArgs* a) {
  a->rsh = L.rsh; a->bsh = L.bsh; a->cstep = L.cstep; a->uoff = L.uoff; a->voff = L.voff;
  if (L.kind != kElemU8) { a->pkind = L.kind; a->pesz = L.esz; a->pstep = L.pstep; a->pone = L.pone; }
}

int prepare_scan(sjpeg_hip_engine* e, const sjpeg_hip_source* src,
                 int W, int H, int mode, int nframes, const sjpeg_hip_scan_tables* tables,
                 hipStream_t st, FrameGeo* g, ScanArgs* a, int* src_class, bool per_frame_tables = false,
                 bool piped_encode = false, size_t seg_budget_bytes = 0 /* 0: not an encode, no segment scratch */,
                 SegPlan* plan_out = nullptr, bool no_tables = false /* the histogram kind reads none */) {
  if (e == nullptr || src == nullptr || src->plane[0] == nullptr || tables == nullptr || nframes <= 0) {
    return fail(SJPEG_HIP_EINVAL, "null argument or nframes <= 0");
  }
  if (!frame_geo(W, H, mode, g)) return fail(SJPEG_HIP_EINVAL, "bad dimensions or yuv_mode");
  // the format's row (source_layout.h): the colour mode it implies, what its planes and strides must keep
  // (reference argument checks: src/api.cc:35-36,205-206,260; src/encoders.cc:352-355,427-432)
  memset(a, 0, sizeof(*a));
  const SourceLayout* const L = source_layout(src->format);
  if (L == nullptr) return fail(SJPEG_HIP_EINVAL, "unknown source format");
  *src_class = L->cls;
  layout_args(*L, a);
  if (L->implied != 0 && mode != L->implied) return fail(SJPEG_HIP_EINVAL, "yuv_mode does not match the source format");
  const LayoutFault fault = layout_fault(*L, W, src->plane, src->row_stride, src->frame_stride, kUniformChecks);
  switch (fault.rule) {
    case kFaultNone: break;
    case kFaultRowPitch:      // one pitch, three bases (sjpeg_hip.h): the kernels reach G and B at a uniform distance from R
      return fail(SJPEG_HIP_EINVAL, "SJPEG_HIP_SRC_RGB_PLANAR: row_stride[" + std::to_string(fault.index) + "] must equal row_stride[0]");
    case kFaultFramePitch:
      return fail(SJPEG_HIP_EINVAL, "SJPEG_HIP_SRC_RGB_PLANAR: frame_stride[" + std::to_string(fault.index) + "] must equal frame_stride[0]");
    case kFaultElemPlane: case kFaultElemRow: case kFaultElemFrame:      // float elements: addresses and strides in whole elements
      return fail(SJPEG_HIP_EINVAL, std::string(L->one_pitch ? "SJPEG_HIP_SRC_RGB_PLANAR_F32 / _F16 / _BF16: " : "SJPEG_HIP_SRC_RGB_F* / _RGBA_F* / _GRAY_F*: ") +
                                        layout_fault_text(*L, fault));
    default: return fail(SJPEG_HIP_EINVAL, layout_fault_text(*L, fault));
  }
  layout_planes(*L, src->plane, src->row_stride, src->frame_stride, a->plane, a->row_stride, a->frame_stride);
  put_transform(e, a);                            // (read by the float class alone)
  if (nframes > 65535) return fail(SJPEG_HIP_EINVAL, "nframes > 65535");
  dbg_mark("prepare: begin");
  HIP_TRY(hipSetDevice(e->device));
  if (int rc0 = order_on_stream(e, st)) return rc0;
  dbg_mark("prepare: ordered");
  // anything but a pipelined encode shares buffers with the stitch still running on the engine's stream
  if (e->side_pending && !piped_encode) {
    if (int rcm = side_mark(e)) return rcm;
    HIP_TRY(hipStreamWaitEvent(st, e->side_done, 0));
  }
  int rc;
  const int ntab = per_frame_tables ? nframes : 1;
  // (per-frame tables of a batch's part lie behind those of the parts in front)
  const int tab_first = per_frame_tables ? part_first_frame(e) : 0;
  if (per_frame_tables && tab_first + nframes > part_total_frames(e, nframes)) return fail(SJPEG_HIP_EINVAL, "part outside the batch");
  if ((rc = e->tables.ensure(per_frame_tables ? part_total_frames(e, nframes) : 1))) return rc;
  const size_t total_segs = static_cast<size_t>(nframes) * g->nseg;
  if ((rc = e->seg_nbits.ensure(total_segs))) return rc;
  SegPlan plan = {0, 0, 0};
  if (seg_budget_bytes != 0) {
    plan = seg_plan(*g, seg_budget_bytes);
    if ((rc = e->seg_words.ensure(total_segs * plan.slot_words))) return rc;
    if ((rc = e->pool.ensure(static_cast<size_t>(nframes) * plan.pool_words))) return rc;
    if ((rc = e->pool_ctr.ensure(static_cast<size_t>(nframes) * 2))) return rc;
    if ((rc = e->seg_xbase.ensure(total_segs))) return rc;
  }
  if (plan_out != nullptr) *plan_out = plan;
  dbg_mark("prepare: buffers");
  if (!no_tables) {
    // (pageable source: the copy has left the host buffer when the call returns)
    std::vector<DevTables> host_tables(ntab);
    for (int i = 0; i < ntab; ++i) digest_tables(tables + i, &host_tables[i]);
    // (early uploads are never skipped: what the buffer holds was put there by another stream's order)
    const bool held = e->up_stream == nullptr && tab_first == 0 && e->tables_held_at == e->tables.p && e->tables_stream == st &&
                      e->tables_held.size() == static_cast<size_t>(ntab) &&
                      memcmp(e->tables_held.data(), host_tables.data(), sizeof(DevTables) * ntab) == 0;
    dbg_mark("prepare: tables digested");
    if (!held) {
      e->tables_held_at = nullptr;
      if (int rcu = upload(e, e->tables.p + tab_first, host_tables.data(), sizeof(DevTables) * ntab, st)) return rcu;
      dbg_mark("prepare: tables uploaded");
      if (ntab <= 16 && e->up_stream == nullptr && tab_first == 0) {   // (a big batch of per-frame tables is not worth holding)
        e->tables_held.swap(host_tables);
        e->tables_held_at = e->tables.p; e->tables_stream = st;
      } else {
        e->tables_held.clear();
      }
    }
  }
  a->W = W; a->H = H; a->mb_w = g->mb_w; a->n_mcus = g->n_mcus; a->nseg = g->nseg;
  a->seg_first = 0;
  a->rst = (tables->flags & SJPEG_HIP_RESTART_MARKERS) ? 1 : 0;
  a->has_clip = (W % g->px != 0) || (H % g->px != 0);
  a->tables = e->tables.p + tab_first;
  a->tables_stride = per_frame_tables ? 1 : 0;
  a->seg_words = e->seg_words.p;
  a->pool = e->pool.p; a->pool_words = plan.pool_words; a->pool_ctr = e->pool_ctr.p; a->seg_xbase = e->seg_xbase.p;
  a->replay = nullptr;
  a->slot_words = plan.slot_words;
  a->seg_nbits = e->seg_nbits.p;
  a->coeffs = nullptr;
  a->partial = nullptr;
  a->ablate = e->ablate;
  a->stamps = nullptr;
  if (e->want_stamps) {
    if (int rc2 = e->stamps.ensure(total_segs * 8)) return rc2;
    a->stamps = e->stamps.p;
    // SJPEG_HIP_STAMPS=2: the 100 MHz real-time counter (one clock for the whole device: when workgroups start
    // and end relative to each other) instead of the shader-clock cycle counter (per CU: phase durations)
    a->stamp_real = e->stamp_mode == 2 ? 1 : (e->stamp_mode == 3 ? 2 : 0);
    e->stamps_n = total_segs * 8;
  }
  return 0;
}

}  // namespace

extern "C" {

int sjpeg_hip_abi_version(void) { return SJPEG_HIP_ABI_VERSION; }

const char* sjpeg_hip_last_error(void) { return g_last_error.c_str(); }
// (the other translation units of the C-ABI report through the same thread-local text)
__attribute__((visibility("hidden"))) void sjpeg_hip_internal_set_last_error(const char* msg) { g_last_error = msg ? msg : ""; }

int sjpeg_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int sjpeg_hip_engine_create(int device, sjpeg_hip_engine** engine) {
  if (engine == nullptr) return fail(SJPEG_HIP_EINVAL, "engine == NULL");
  *engine = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    return fail(SJPEG_HIP_ENODEV, "no HIP device available (this library has no CPU fallback)");
  }
  if (device < 0 || device >= n) return fail(SJPEG_HIP_EINVAL, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    return fail(SJPEG_HIP_ENODEV, std::string("device is ") + prop.gcnArchName +
                                      ", this library is built for gfx950 only");
  }
  sjpeg_hip_engine* e = new (std::nothrow) sjpeg_hip_engine;
  if (e == nullptr) return fail(SJPEG_HIP_ENOMEM, "host allocation failed");
  e->device = device;
  if (prop.multiProcessorCount > 0) e->cu_count = prop.multiProcessorCount;
  // (two streams, as in round 5, and not one more: the device has four hardware queues by default, and with a third
  // engine-owned stream made here the stitch stream of the pipelined mode -- made later, by set_pipelined -- shared the
  // caller's queue: the headline step went from 0.889 to 1.096 ms, K1 and the stitch one after the other.  The fourth
  // lane of the batch path, an experiment knob, makes its stream when it is asked for.)
  if (hipStreamCreateWithFlags(&e->batch_side, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&e->batch_up, hipStreamNonBlocking) != hipSuccess) {
    if (e->batch_side) (void)hipStreamDestroy(e->batch_side);
    delete e;
    return fail(SJPEG_HIP_ERUNTIME, "hipStreamCreate failed");
  }
  if (const char* ab = getenv("SJPEG_HIP_ABLATE")) {                       // profiling / race-stress aid only
    e->ablate = atoi(ab);
    if (e->ablate != 0) {
      fprintf(stderr, "sjpeg_amd: SJPEG_HIP_ABLATE=%d is set: kernels skip phases or stall waves on purpose, "
                      "the output of this engine is NOT valid JPEG data\n", e->ablate);
    }
  }
  if (const char* hs = getenv("SJPEG_HIP_HISTO_SLOTS")) e->histo_slots = atoi(hs);
  if (const char* sm = getenv("SJPEG_HIP_STAMPS")) { e->want_stamps = true; e->stamp_mode = atoi(sm); }
  if (const char* sl = getenv("SJPEG_HIP_SCRATCH_LIMIT_BYTES")) { const long long v = atoll(sl); if (v > 0) e->scratch_limit = static_cast<size_t>(v); }
  *engine = e;
  return 0;
}

void sjpeg_hip_engine_destroy(sjpeg_hip_engine* e) {
  if (e == nullptr) return;
  (void)hipSetDevice(e->device);
  if (!e->is_lane) {
    for (hipStream_t bs : {e->batch_side, e->batch_up, e->batch_lane3}) if (bs) (void)hipStreamSynchronize(bs);   // (the lanes' work)
    for (auto& l : e->lane) { if (l) sjpeg_hip_engine_destroy(l); l = nullptr; }
    for (auto& ev : e->lane_done) if (ev) (void)hipEventDestroy(ev);
    if (e->lane_in) (void)hipEventDestroy(e->lane_in);
  }
  e->tables.release(); e->header.release(); e->seg_words.release(); e->seg_nbits.release(); e->pool.release(); e->pool_ctr.release(); e->seg_xbase.release(); e->replay.release();
  e->ubuf.release(); e->chunk_ff.release(); e->partial.release(); e->seg_off.release(); e->chunk_off.release(); e->hdr_off.release(); e->stamps.release();
  e->frame_flags.release(); e->ragged.release(); e->hdr_stage.release();
  e->risk_table.release(); e->auto_buf.release(); e->sharp_arena.release(); e->search_sizes.release(); e->pack_cursor.release();
  e->reduced.release(); e->reduce_desc.release(); e->colour_desc.release(); e->final_pictures.release(); e->unsharp_desc.release(); e->resample_tables.release(); e->filter_mid.release(); e->filter_desc.release(); e->composed.release(); e->compose_desc.release();
  for (auto& ev : e->ev) if (ev) (void)hipEventDestroy(ev);
  for (auto& sg : e->stage) {
    if (sg.busy) (void)hipEventSynchronize(sg.ev);
    if (sg.ev) (void)hipEventDestroy(sg.ev);
    if (sg.p) (void)hipHostFree(sg.p);
  }
  e->seg_words2.release(); e->seg_nbits2.release(); e->pool2.release(); e->pool_ctr2.release(); e->seg_xbase2.release();
  if (e->side) { (void)hipStreamSynchronize(e->side); (void)hipStreamDestroy(e->side); }
  for (hipStream_t bs : {e->batch_side, e->batch_up, e->batch_lane3}) if (bs) { (void)hipStreamSynchronize(bs); (void)hipStreamDestroy(bs); }
  for (hipEvent_t ev : {e->k1_done, e->side_done, e->k3_done[0], e->k3_done[1], e->cross_ev}) if (ev) (void)hipEventDestroy(ev);
  delete e;
}

int sjpeg_hip_engine_trim(sjpeg_hip_engine* e) {
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, "engine == NULL");
  HIP_TRY(hipSetDevice(e->device));
  // the engine does not own the streams its calls ran on: wait for the whole device
  HIP_TRY(hipDeviceSynchronize());
  for (auto& l : e->lane) { if (l != nullptr) { if (int rcl = sjpeg_hip_engine_trim(l)) return rcl; } }
  e->seg_words.release(); e->seg_nbits.release(); e->pool.release(); e->pool_ctr.release(); e->seg_xbase.release();
  e->seg_words2.release(); e->seg_nbits2.release(); e->pool2.release(); e->pool_ctr2.release(); e->seg_xbase2.release();
  e->ubuf.release(); e->chunk_ff.release(); e->partial.release(); e->replay.release();
  e->seg_off.release(); e->chunk_off.release(); e->hdr_off.release(); e->stamps.release();
  e->frame_flags.release(); e->ragged.release(); e->hdr_stage.release();
  e->auto_buf.release(); e->sharp_arena.release(); e->search_sizes.release(); e->pack_cursor.release();
  e->reduced.release(); e->reduce_desc.release(); e->colour_desc.release(); e->final_pictures.release(); e->unsharp_desc.release(); e->resample_tables.release(); e->filter_mid.release(); e->filter_desc.release(); e->composed.release(); e->compose_desc.release();
  e->tables.release(); e->header.release();        // (per-frame tables of a large batch are scratch like the rest)
  for (auto& sg : e->stage) {                      // ... and so are the pinned blocks they were uploaded through
    // (their copies are done: the device was waited for above; the event is waited for all the same, so that the
    // block's life does not hang on that one line)
    if (sg.busy && sg.ev) (void)hipEventSynchronize(sg.ev);
    if (sg.p) (void)hipHostFree(sg.p);
    sg.p = nullptr; sg.dp = nullptr; sg.cap = 0; sg.busy = false;
  }
  e->tables_held_at = nullptr; e->header_held_at = nullptr;
  e->replay_w = e->replay_h = e->replay_mode = e->replay_nframes = 0;
  e->stamps_n = 0;
  e->last_nseg = e->last_nframes = 0;
  e->ctr_clean_at[0] = e->ctr_clean_at[1] = nullptr;
  e->ctr_clean_n[0] = e->ctr_clean_n[1] = 0;
  e->k3_pending[0] = e->k3_pending[1] = e->side_pending = e->side_recorded = false;
  e->last_stream_valid = false;
  e->ev_valid = false;
  return 0;
}

int sjpeg_hip_engine_set_pixel_transform(sjpeg_hip_engine* e, float scale, float bias) {
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_engine_set_pixel_transform: engine == NULL");
  if (!(scale - scale == 0.0f) || !(bias - bias == 0.0f)) {      // (neither NaN nor an infinity)
    return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_engine_set_pixel_transform: scale and bias must be finite");
  }
  for (int c = 0; c < 3; ++c) { e->pscale[c] = scale; e->pbias[c] = bias; }
  return 0;
}

int sjpeg_hip_engine_set_pixel_transform3(sjpeg_hip_engine* e, const float scale[3], const float bias[3]) {
  if (e == nullptr || scale == nullptr || bias == nullptr) {
    return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_engine_set_pixel_transform3: engine, scale or bias == NULL");
  }
  for (int c = 0; c < 3; ++c) {
    if (!(scale[c] - scale[c] == 0.0f) || !(bias[c] - bias[c] == 0.0f)) {      // (neither NaN nor an infinity)
      return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_engine_set_pixel_transform3: scale[" + std::to_string(c) + "] and bias[" +
                                        std::to_string(c) + "] must be finite");
    }
  }
  for (int c = 0; c < 3; ++c) { e->pscale[c] = scale[c]; e->pbias[c] = bias[c]; }
  return 0;
}

int sjpeg_hip_engine_get_pixel_transform3(const sjpeg_hip_engine* e, float scale[3], float bias[3]) {
  if (e == nullptr || scale == nullptr || bias == nullptr) {
    return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_engine_get_pixel_transform3: engine, scale or bias == NULL");
  }
  for (int c = 0; c < 3; ++c) { scale[c] = e->pscale[c]; bias[c] = e->pbias[c]; }
  return 0;
}

int sjpeg_hip_engine_get_pixel_transform(const sjpeg_hip_engine* e, float* scale, float* bias) {
  if (e == nullptr || scale == nullptr || bias == nullptr) {
    return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_engine_get_pixel_transform: engine, scale or bias == NULL");
  }
  *scale = e->pscale[0]; *bias = e->pbias[0];        // (channel 0: sjpeg_hip_engine_get_pixel_transform3 has all three)
  return 0;
}

int sjpeg_hip_engine_set_pipelined(sjpeg_hip_engine* e, int on) {
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, "engine == NULL");
  HIP_TRY(hipSetDevice(e->device));
  if (on && e->side == nullptr) {
    {
      // the stitch stream gets the device's least priority: its kernels are meant to take the issue
      // slots K1 leaves idle, not K1's (measured: step -0.3 % at best, profiles/HISTORY.md)
      int least = 0, greatest = 0;
      if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess ||
          hipStreamCreateWithPriority(&e->side, hipStreamNonBlocking, least) != hipSuccess) {
        (void)hipGetLastError();
        e->side = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
      }
    }
    for (hipEvent_t* ev : {&e->k1_done, &e->side_done, &e->k3_done[0], &e->k3_done[1]}) {
      HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    }
  }
  if (!on && e->pipelined) {                       // drain: from here on the caller's stream orders everything again
    HIP_TRY(hipStreamSynchronize(e->side));
    e->k3_pending[0] = e->k3_pending[1] = e->side_pending = e->side_recorded = false;
  }
  e->pipelined = on != 0;
  e->header_held_at = nullptr;                    // the header buffer changes streams
  return 0;
}

int sjpeg_hip_engine_wait(sjpeg_hip_engine* e, void* stream) {
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, "engine == NULL");
  if (e->side_pending) {
    HIP_TRY(hipSetDevice(e->device));
    if (int rcm = side_mark(e)) return rcm;
    HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(stream), e->side_done, 0));
  }
  return 0;
}

size_t sjpeg_hip_frame_bound(int width, int height, int yuv_mode, size_t header_size) {
  FrameGeo g;
  if (!frame_geo(width, height, yuv_mode, &g)) return 0;
  // un-stuffed worst case = slots; stuffing at most doubles it
  const size_t unstuffed = static_cast<size_t>(g.nseg) * g.slot_words * 4;
  // (a multiple of 16: the default out_stride of the bindings is what sjpeg_hip_compact_streams accepts)
  return (header_size + 2 * unstuffed + 2 + 64 + 15) & ~size_t(15);
}

// profiling only (not in the public header): copies the per-workgroup cycle stamps of the last scan
size_t sjpeg_hip_debug_stamps(sjpeg_hip_engine* e, unsigned long long* out, size_t cap) {
  if (e == nullptr || !e->want_stamps || e->stamps.p == nullptr) return 0;
  const size_t n = e->stamps_n < cap ? e->stamps_n : cap;
  if (hipMemcpy(out, e->stamps.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return n;
}

int sjpeg_hip_engine_set_timing(sjpeg_hip_engine* e, int enable) {
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, "engine == NULL");
  HIP_TRY(hipSetDevice(e->device));
  if (enable && e->ev[0] == nullptr) {
    for (auto& ev : e->ev) HIP_TRY(hipEventCreate(&ev));
  }
  e->timing = enable != 0;
  e->ev_valid = false;
  return 0;
}

static float elapsed(sjpeg_hip_engine* e, int i0, int i1) {
  if (e == nullptr || !e->ev_valid) return -1.f;
  if (hipEventSynchronize(e->ev[i1]) != hipSuccess) return -1.f;
  float ms = -1.f;
  if (hipEventElapsedTime(&ms, e->ev[i0], e->ev[i1]) != hipSuccess) return -1.f;
  return ms;
}
float sjpeg_hip_engine_last_scan_ms(sjpeg_hip_engine* e) { return elapsed(e, 0, 1); }
float sjpeg_hip_engine_last_total_ms(sjpeg_hip_engine* e) { return elapsed(e, 0, 2); }

size_t sjpeg_hip_engine_scratch_bytes(sjpeg_hip_engine* e) {
  if (e == nullptr) return 0;
  auto b = [](const auto& buf) { return buf.cap * sizeof(*buf.p); };
  size_t lanes = 0;
  for (auto* l : e->lane) if (l != nullptr) lanes += sjpeg_hip_engine_scratch_bytes(l);
  return lanes + b(e->tables) + b(e->header) + b(e->seg_words) + b(e->seg_nbits) + b(e->pool) + b(e->pool_ctr) + b(e->seg_xbase) +
         b(e->ubuf) + b(e->chunk_ff) + b(e->partial) + b(e->replay) + b(e->seg_off) + b(e->chunk_off) + b(e->stamps) +
         b(e->hdr_off) + b(e->seg_words2) + b(e->seg_nbits2) + b(e->pool2) + b(e->pool_ctr2) + b(e->seg_xbase2) + b(e->ragged) + b(e->hdr_stage) +
         b(e->risk_table) + b(e->auto_buf) + b(e->sharp_arena) + b(e->search_sizes) + b(e->pack_cursor) + b(e->reduced) + b(e->reduce_desc) + b(e->colour_desc) +
         b(e->final_pictures) + b(e->unsharp_desc) + b(e->resample_tables) + b(e->filter_mid) + b(e->filter_desc) + b(e->composed) + b(e->compose_desc);
}

int sjpeg_hip_scan_coeffs_src(sjpeg_hip_engine* e, const sjpeg_hip_source* src, int width, int height,
                              int yuv_mode, int nframes, const sjpeg_hip_scan_tables* tables,
                              int16_t* d_coeffs, void* stream) {
  if (d_coeffs == nullptr) return fail(SJPEG_HIP_EINVAL, "d_coeffs == NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  FrameGeo g;
  ScanArgs a;
  int cls = 0;
  const int rc = prepare_scan(e, src, width, height, yuv_mode, nframes, tables, st, &g, &a, &cls);
  if (rc) return rc;
  a.coeffs = d_coeffs;
  return launch_scan<kKindTap>(yuv_mode, cls, dim3(g.nseg, nframes), st, a);
}

int sjpeg_hip_scan_coeffs(sjpeg_hip_engine* e, const void* d_rgb, int64_t row_stride,
                          int64_t frame_stride, int width, int height, int yuv_mode, int nframes,
                          const sjpeg_hip_scan_tables* tables, int16_t* d_coeffs, void* stream) {
  const sjpeg_hip_source s = rgb_source(d_rgb, row_stride, frame_stride);
  return sjpeg_hip_scan_coeffs_src(e, &s, width, height, yuv_mode, nframes, tables, d_coeffs, stream);
}

static int scan_statistics(sjpeg_hip_engine* e, const sjpeg_hip_source* src, int width, int height,
                           int yuv_mode, int nframes, const sjpeg_hip_scan_tables* tables,
                           bool histogram, uint32_t* d_out, void* stream, bool per_frame_tables = false) {
  if (d_out == nullptr) return fail(SJPEG_HIP_EINVAL, "output pointer == NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  sjpeg_hip_scan_tables dummy;
  if (tables == nullptr) {                        // the histogram does not depend on any table
    memset(&dummy, 0, sizeof(dummy));
    tables = &dummy;
  }
  FrameGeo g;
  ScanArgs a;
  int cls = 0;
  int rc = prepare_scan(e, src, width, height, yuv_mode, nframes, tables, st, &g, &a, &cls, per_frame_tables, false, 0, nullptr, histogram);
  if (rc) return rc;
  const int words = histogram ? kHistoWords : kStatsWords;
  const int part_total = e->replay_total > 0 ? e->replay_total : nframes;
  const int part_first = e->replay_total > 0 ? e->replay_first : 0;
  if (part_first < 0 || part_first + nframes > part_total) return fail(SJPEG_HIP_EINVAL, "part outside the batch");
  // The histogram kind is persistent: `groups` workgroups per frame walk the frame's segments and leave one partial
  // each (kHistoPartialWords).  As many as run at once, in whole trips -- 16 4K frames of 791 segments on 768 slots: 17
  // trips, 47 groups a frame, 752 workgroups --; at least nseg / 256 (16-bit counters), at most what the partial
  // buffer's frame stride has room for.
  size_t frame_words = static_cast<size_t>(g.nseg) * words;
  int groups = g.nseg;
  if (histogram) {
    // (THREE per CU although four would fit: the kernel runs no faster with four -- tools/histogram_ablate.py with
    // SJPEG_HIP_HISTO_SLOTS --, and four persistent workgroups of 128 registers hold a SIMD's whole register file until the
    // launch ends: the small kernels of the side stream -- the sums of the previous part, their read-back -- would wait)
    const long long slots = e->histo_slots > 0 ? e->histo_slots : 3ll * e->cu_count;
    const long long trips = std::max(1ll, (static_cast<long long>(g.nseg) * nframes + slots - 1) / slots);
    groups = static_cast<int>((g.nseg + trips - 1) / trips);
    const int min_groups = (g.nseg + kHistoMaxSegsPerGroup - 1) / kHistoMaxSegsPerGroup;
    // (small batches: a partial per segment if need be -- twice the old stride; large ones keep the old stride)
    if (static_cast<size_t>(part_total) * g.nseg * kHistoPartialWords * sizeof(uint32_t) <= (256u << 20)) frame_words = static_cast<size_t>(g.nseg) * kHistoPartialWords;
    frame_words = std::max(frame_words, static_cast<size_t>(min_groups) * kHistoPartialWords);
    groups = std::min(groups, static_cast<int>(frame_words / kHistoPartialWords));
    groups = std::max(groups, min_groups);
  }
  if ((rc = e->partial.ensure(static_cast<size_t>(part_total) * frame_words))) return rc;
  uint32_t* const partial = e->partial.p + static_cast<size_t>(part_first) * frame_words;
  a.partial = partial;
  const bool coefs_in = !histogram && e->coefs_use && (tables->flags & SJPEG_HIP_QUANT_KEEP) && !(tables->flags & SJPEG_HIP_QUANT_TRELLIS);
  if (coefs_in) {
    const int total = e->replay_total > 0 ? e->replay_total : nframes;
    if (e->replay.p == nullptr || e->replay_w != width || e->replay_h != height || e->replay_mode != yuv_mode || e->replay_nframes != total) {
      return fail(SJPEG_HIP_EINVAL, "no histogram pass of these frames left its coefficients behind");
    }
  }
  static const bool force_keep = getenv("SJPEG_HIP_FORCE_COEF_KEEP") != nullptr;   // (measurement aid: tools/histogram_ablate.py)
  if ((!histogram && (tables->flags & SJPEG_HIP_QUANT_KEEP)) || (histogram && (e->coefs_keep || force_keep))) {
    const size_t per_frame = static_cast<size_t>(g.nseg) * kScanThreads * 36;
    const int total = e->replay_total > 0 ? e->replay_total : nframes;
    const int first = e->replay_total > 0 ? e->replay_first : 0;
    if (first < 0 || first + nframes > total) return fail(SJPEG_HIP_EINVAL, "kept-block range outside the batch");
    if ((rc = e->replay.ensure(static_cast<size_t>(total) * per_frame))) return rc;
    a.replay = e->replay.p + static_cast<size_t>(first) * per_frame;
    e->replay_w = width; e->replay_h = height; e->replay_mode = yuv_mode; e->replay_nframes = total;
  }
  dbg_mark("statistics: buffers");
  if ((rc = sync_uploads(e, st))) return rc;
  if (histogram) rc = launch_scan<kKindHisto>(yuv_mode, cls, dim3(groups, nframes), st, a);
  else if (tables != nullptr && (tables->flags & SJPEG_HIP_QUANT_TRELLIS)) rc = launch_scan<kKindStatsTrellis>(yuv_mode, cls, dim3(g.nseg, nframes), st, a);
  else if (coefs_in) rc = launch_scan_src<kKindStatsCoef, kSrcRgb24>(yuv_mode, dim3(g.nseg, nframes), st, a);   // (reads no pixel)
  else rc = launch_scan<kKindStats>(yuv_mode, cls, dim3(g.nseg, nframes), st, a);
  if (rc) return rc;
  dbg_mark("statistics: pass launched");
  // The symbol counts (544 words a frame): slices of the segments meet in the output with device-scope atomics -- small
  // enough for the atomics not to matter, they take the slices they can get (16 frames: 7 us with 32, 25 with 2).
  const int xblocks = histogram ? 32 : (words + kThreads - 1) / kThreads;
  int slices = 4096 / (xblocks * nframes);
  if (slices > 32) slices = 32;
  // (the histogram's partials: a workgroup's four waves share the groups; slices -- and their atomics -- only where one
  // wave would walk more than 64 partials: single large frames)
  if (histogram) slices = std::min(slices, (groups + 255) / 256);
  static const int slices_env = getenv("SJPEG_HIP_REDUCE_SLICES") ? atoi(getenv("SJPEG_HIP_REDUCE_SLICES")) : 0;   // (experiments)
  if (slices_env > 0) slices = slices_env;
  if (slices < 1 || g.nseg < 64) slices = 1;
  if (histogram && groups < slices) slices = groups;
  const dim3 grid(xblocks, nframes, slices);
  hipStream_t rs = st;
  if (e->reduce_stream != nullptr && e->reduce_ev != nullptr) {   // (a batch coded in parts: see sjpeg_hip_encode_batch_src)
    rs = e->reduce_stream;
    HIP_TRY(hipEventRecord(e->reduce_ev, st));
    HIP_TRY(hipStreamWaitEvent(rs, e->reduce_ev, 0));
    dbg_mark("statistics: side stream waits");
  }
  if (!(histogram && slices == 1)) {               // (one slice stores, several add)
    HIP_TRY(hipMemsetAsync(d_out, 0, static_cast<size_t>(nframes) * words * (histogram ? 4 : 1) * sizeof(uint32_t), rs));
    dbg_mark("statistics: memset");
  }
  if (histogram) {
    static_assert(kThreads == kScanThreads, "reduce_partials16: a thread per thread of the scan kernel");
    // (the partials of a launch lie back to back: frame f of this launch at f * groups * kHistoPartialWords)
    hipLaunchKernelGGL(reduce_partials16<>, grid, dim3(kThreads), 0, rs, reinterpret_cast<const uint4*>(partial), groups, d_out);
  } else {
    hipLaunchKernelGGL(reduce_partials<>, grid, dim3(kThreads), 0, rs, partial, g.nseg, words, d_out);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int sjpeg_hip_scan_quant_error_src(sjpeg_hip_engine* e, const sjpeg_hip_source* src, int width,
                                   int height, int yuv_mode, int nframes,
                                   const sjpeg_hip_scan_tables* tables, uint64_t* d_err, void* stream) {
  if (d_err == nullptr || tables == nullptr) return fail(SJPEG_HIP_EINVAL, "null argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  FrameGeo g;
  ScanArgs a;
  int cls = 0;
  int rc = prepare_scan(e, src, width, height, yuv_mode, nframes, tables, st, &g, &a, &cls);
  if (rc) return rc;
  if ((rc = e->partial.ensure(static_cast<size_t>(nframes) * g.nseg * 2))) return rc;
  a.partial = e->partial.p;
  if ((rc = launch_scan<kKindError>(yuv_mode, cls, dim3(g.nseg, nframes), st, a))) return rc;
  hipLaunchKernelGGL(reduce_error<>, dim3(nframes), dim3(kThreads), 0, st,
                     reinterpret_cast<const unsigned long long*>(e->partial.p), g.nseg,
                     reinterpret_cast<unsigned long long*>(d_err));
  HIP_TRY(hipGetLastError());
  return 0;
}

int sjpeg_hip_engine_entropy_bits(sjpeg_hip_engine* e, uint64_t* bits, int nframes) {
  if (e == nullptr || bits == nullptr || nframes <= 0) return fail(SJPEG_HIP_EINVAL, "null argument");
  if (e->last_nseg <= 0 || nframes > e->last_nframes) return fail(SJPEG_HIP_EINVAL, "no matching encode call");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  for (int f = 0; f < nframes; ++f) {
    HIP_TRY(hipMemcpy(&bits[f], e->seg_off.p + static_cast<size_t>(f) * (e->last_nseg + 1) + e->last_nseg,
                      sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  return 0;
}

int sjpeg_hip_scan_histogram_src(sjpeg_hip_engine* e, const sjpeg_hip_source* src, int width, int height,
                                 int yuv_mode, int nframes, uint32_t* d_hist, void* stream) {
  return scan_statistics(e, src, width, height, yuv_mode, nframes, nullptr, true, d_hist, stream);
}

int sjpeg_hip_scan_histogram(sjpeg_hip_engine* e, const void* d_rgb, int64_t row_stride,
                             int64_t frame_stride, int width, int height, int yuv_mode, int nframes,
                             uint32_t* d_hist, void* stream) {
  const sjpeg_hip_source s = rgb_source(d_rgb, row_stride, frame_stride);
  return scan_statistics(e, &s, width, height, yuv_mode, nframes, nullptr, true, d_hist, stream);
}

int sjpeg_hip_scan_symbol_stats_src(sjpeg_hip_engine* e, const sjpeg_hip_source* src, int width,
                                    int height, int yuv_mode, int nframes,
                                    const sjpeg_hip_scan_tables* tables, uint32_t* d_freq, void* stream) {
  if (tables == nullptr) return fail(SJPEG_HIP_EINVAL, "tables == NULL");
  return scan_statistics(e, src, width, height, yuv_mode, nframes, tables, false, d_freq, stream);
}

int sjpeg_hip_scan_symbol_stats(sjpeg_hip_engine* e, const void* d_rgb, int64_t row_stride,
                                int64_t frame_stride, int width, int height, int yuv_mode,
                                int nframes, const sjpeg_hip_scan_tables* tables, uint32_t* d_freq,
                                void* stream) {
  const sjpeg_hip_source s = rgb_source(d_rgb, row_stride, frame_stride);
  return sjpeg_hip_scan_symbol_stats_src(e, &s, width, height, yuv_mode, nframes, tables, d_freq, stream);
}

int sjpeg_hip_encode_scan(sjpeg_hip_engine* e, const void* d_rgb, int64_t row_stride,
                          int64_t frame_stride, int width, int height, int yuv_mode, int nframes,
                          const sjpeg_hip_scan_tables* tables, const void* header,
                          size_t header_size, int append_eoi, void* d_out, size_t out_stride,
                          uint64_t* d_sizes, void* stream) {
  const sjpeg_hip_source s = rgb_source(d_rgb, row_stride, frame_stride);
  return sjpeg_hip_encode_scan_src(e, &s, width, height, yuv_mode, nframes, tables, header, header_size,
                                   append_eoi, d_out, out_stride, d_sizes, stream);
}

// header_offsets == NULL: one header (and one set of tables) for every frame; else per frame
static int encode_scan_one(sjpeg_hip_engine* e, const sjpeg_hip_source* src, int width, int height,
                            int yuv_mode, int nframes, const sjpeg_hip_scan_tables* tables,
                            const void* header, size_t header_size, const size_t* header_offsets,
                            int append_eoi, void* d_out, size_t out_stride, uint64_t* d_sizes,
                            void* stream, const int* seg_range = nullptr /* restart mode: code only these segments */,
                            uint64_t* d_pack_off = nullptr /* packed output: [nframes + 1] frame starts */) {
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, "engine == NULL");
  if (d_out == nullptr || d_sizes == nullptr) return fail(SJPEG_HIP_EINVAL, "d_out/d_sizes == NULL");
  if (d_pack_off != nullptr && ((out_stride & 15u) != 0 || (reinterpret_cast<uintptr_t>(d_out) & 15u) != 0 || out_stride >= (1ull << 32))) {
    return fail(SJPEG_HIP_EINVAL, "packed output: d_out and out_stride must be multiples of 16, out_stride below 4 GiB");
  }
  if (header == nullptr) header_size = 0;
  const bool multi = header_offsets != nullptr;
  hipStream_t st = static_cast<hipStream_t>(stream);
  FrameGeo g;
  ScanArgs a;
  int cls = 0;
  const bool piped = e->pipelined;
  SegPlan plan;
  int rc = prepare_scan(e, src, width, height, yuv_mode, nframes, tables, st, &g, &a, &cls, multi, piped,
                        out_stride > 0 ? out_stride : 1, &plan);
  if (rc) return rc;
  int rst_tail = 0;
  if (seg_range != nullptr) {                      // a band of restart intervals: segments [begin, end) of the one frame
    if (nframes != 1 || multi || !a.rst) return fail(SJPEG_HIP_EINVAL, "a segment range needs one frame in restart mode");
    if (seg_range[0] < 0 || seg_range[1] > g.nseg || seg_range[0] >= seg_range[1]) return fail(SJPEG_HIP_EINVAL, "bad segment range");
    rst_tail = seg_range[1] < g.nseg ? 1 : 0;
    a.seg_first = seg_range[0];
    a.nseg = seg_range[1] - seg_range[0];
    g.nseg = a.nseg;                               // (everything below works on the band)
  }
  hipStream_t hs = piped ? e->side : st;           // the stream of the stitch kernels and of what only they read
  size_t largest_header = header_size;
  if (multi) {
    if (tables->flags & SJPEG_HIP_QUANT_REPLAY) {
      for (int f = 1; f < nframes; ++f) if (!(tables[f].flags & SJPEG_HIP_QUANT_REPLAY)) return fail(SJPEG_HIP_EINVAL, "flags must agree between the frames' tables");
    }
    for (int f = 1; f < nframes; ++f) {
      if ((tables[f].flags ^ tables->flags) & SJPEG_HIP_RESTART_MARKERS) return fail(SJPEG_HIP_EINVAL, "flags must agree between the frames' tables");
    }
    largest_header = 0;
    std::vector<uint32_t> offs(static_cast<size_t>(nframes) + 1);
    for (int f = 0; f <= nframes; ++f) {
      if (header_offsets[f] > header_size || (f > 0 && header_offsets[f] < header_offsets[f - 1])) {
        return fail(SJPEG_HIP_EINVAL, "header_offsets must ascend inside the header blob");
      }
      offs[f] = static_cast<uint32_t>(header_offsets[f]);
      if (f > 0 && header_offsets[f] - header_offsets[f - 1] > largest_header) largest_header = header_offsets[f] - header_offsets[f - 1];
    }
    // (a batch's part: its nframes + 1 offsets behind those of the parts in front -- two slots a frame)
    if ((rc = e->hdr_off.ensure(2 * static_cast<size_t>(part_total_frames(e, nframes)) + 2))) return rc;
    if (int rcu = upload(e, e->hdr_off.p + 2 * static_cast<size_t>(part_first_frame(e)), offs.data(), offs.size() * sizeof(uint32_t), hs)) return rcu;
  }
  header_size = header == nullptr ? 0 : header_size;
  if (out_stride < largest_header + 2 + 64) {
    return fail(SJPEG_HIP_ECAPACITY, "out_stride " + std::to_string(out_stride) + " too small");
  }
  const size_t ubuf_words = plan.ubuf_words;
  const uint32_t max_chunks = static_cast<uint32_t>((ubuf_words + kChunkWords - 1) / kChunkWords);
  if ((rc = e->seg_off.ensure(static_cast<size_t>(nframes) * (g.nseg + 1)))) return rc;
  if ((rc = e->ubuf.ensure(static_cast<size_t>(nframes) * ubuf_words))) return rc;
  if ((rc = e->chunk_ff.ensure(static_cast<size_t>(nframes) * max_chunks))) return rc;
  if ((rc = e->chunk_off.ensure(static_cast<size_t>(nframes) * max_chunks))) return rc;
  if ((rc = e->frame_flags.ensure(static_cast<size_t>(nframes)))) return rc;
  // (a batch's part: its headers behind those of the parts in front, kPartHeaderBytes a frame -- what
  // sjpeg_hip_encode_batch_src builds its headers in)
  constexpr size_t kPartHeaderBytes = 2048;
  const size_t hdr_first = (multi && e->replay_total > 0) ? static_cast<size_t>(part_first_frame(e)) * kPartHeaderBytes : 0;
  const size_t hdr_room = (multi && e->replay_total > 0) ? static_cast<size_t>(e->replay_total) * kPartHeaderBytes : 0;
  if (e->up_stream != nullptr && hdr_room != 0 && header_size > static_cast<size_t>(nframes) * kPartHeaderBytes) {
    return fail(SJPEG_HIP_EINVAL, "headers of a batch's part do not fit its share of the header buffer");
  }
  if ((rc = e->header.ensure(std::max(hdr_room, hdr_first + (header_size > 0 ? header_size : static_cast<size_t>(1)))))) return rc;
  if (header_size > 0) {
    const uint8_t* const hb = static_cast<const uint8_t*>(header);
    const bool held = e->up_stream == nullptr && hdr_first == 0 && e->header_held_at == e->header.p && e->header_stream == hs &&
                      e->header_held.size() == header_size && memcmp(e->header_held.data(), hb, header_size) == 0;
    if (!held) {
      e->header_held_at = nullptr;
      if (int rcu = upload(e, e->header.p + hdr_first, header, header_size, hs)) return rcu;
      if (e->up_stream == nullptr && hdr_first == 0) {
        e->header_held.assign(hb, hb + header_size);
        e->header_held_at = e->header.p; e->header_stream = hs;
      }
    }
  }

  e->last_nseg = g.nseg; e->last_nframes = nframes;
  const int set = piped ? e->set : 0;
  if (piped) {
    if (set == 1) {                                // the second set of what K1 writes and K2 / K3 read
      const size_t total_segs = static_cast<size_t>(nframes) * g.nseg;
      if ((rc = e->seg_words2.ensure(total_segs * plan.slot_words))) return rc;
      if ((rc = e->seg_nbits2.ensure(total_segs))) return rc;
      if ((rc = e->pool2.ensure(static_cast<size_t>(nframes) * plan.pool_words))) return rc;
      if ((rc = e->pool_ctr2.ensure(static_cast<size_t>(nframes) * 2))) return rc;
      if ((rc = e->seg_xbase2.ensure(total_segs))) return rc;
      a.seg_words = e->seg_words2.p; a.seg_nbits = e->seg_nbits2.p;
      a.pool = e->pool2.p; a.pool_ctr = e->pool_ctr2.p; a.seg_xbase = e->seg_xbase2.p;
    }
    // this set was last read by the K3 of the call before the previous one
    // (two calls back: as a rule long done, and a query costs the host a tenth of what a wait in the queue does)
    if (e->k3_pending[set]) {
      if (hipEventQuery(e->k3_done[set]) == hipSuccess) e->k3_pending[set] = false;
      else { (void)hipGetLastError(); HIP_TRY(hipStreamWaitEvent(st, e->k3_done[set], 0)); }
    }
  }
  if (e->ctr_clean_at[set] != a.pool_ctr || e->ctr_clean_n[set] < static_cast<size_t>(nframes)) {
    HIP_TRY(hipMemsetAsync(a.pool_ctr, 0, static_cast<size_t>(nframes) * 2 * sizeof(uint32_t), st));
  }
  e->ctr_clean_at[set] = nullptr;                  // dirty from K1 on, until this call's K4 is in the queue
  StitchArgs s;
  s.nseg = g.nseg; s.nframes = nframes;
  s.seg_nbits = a.seg_nbits; s.seg_off = e->seg_off.p;
  s.seg_words = a.seg_words; s.slot_words = plan.slot_words;
  s.pool = a.pool; s.pool_words = plan.pool_words; s.seg_xbase = a.seg_xbase; s.pool_ctr = a.pool_ctr;
  s.ubuf = e->ubuf.p; s.ubuf_words = ubuf_words;
  s.chunk_ff = e->chunk_ff.p; s.chunk_off = e->chunk_off.p; s.max_chunks = max_chunks;
  s.header = e->header.p + hdr_first; s.header_size = static_cast<uint32_t>(header_size);
  s.append_eoi = append_eoi;
  s.out = static_cast<uint8_t*>(d_out); s.out_stride = out_stride;
  s.sizes = reinterpret_cast<unsigned long long*>(d_sizes);
  s.pack_off = reinterpret_cast<unsigned long long*>(d_pack_off);
  s.seg_nbits64 = nullptr; s.total_bits_out = nullptr; s.subs = 1; s.wide_subs = 0;
  // few segments (one 4K frame: 791, one 8K 4:4:4 frame: 6172): one wave per 768 words of a slot instead of
  // one per segment -- a 1030-word segment was two dependent round trips of one wave (8K 4:4:4: K3 38 us)
  if (static_cast<size_t>(nframes) * g.nseg <= 8192 && (plan.slot_words & 3u) == 0u && plan.slot_words >= 776u) {
    s.subs = (plan.slot_words + kWideSpec * 256u - 1u) / (kWideSpec * 256u);
    s.wide_subs = s.subs > 1u ? 1u : 0u;
    if (!s.wide_subs) s.subs = 1;
  }
  s.hdr_off = multi ? e->hdr_off.p + 2 * static_cast<size_t>(part_first_frame(e)) : nullptr;
  s.seg_first = a.seg_first; s.rst_tail = rst_tail;
  s.frame_flags = e->frame_flags.p;
  // few, small frames (the launches whose time is launch latency): K4 inside K5 -- one dependent launch less.  (Not
  // in pipelined mode, whose hand-over hangs on K4; not with packed output or restart markers, which read what K4 writes.)
  static const bool no_fuse_k4 = getenv("SJPEG_HIP_NO_FUSED_K4") != nullptr;        // (A/B)
  // (2 = the large form: ONE frame of up to 8192 segments whatever its output slot -- an 8K 4:4:4 q90 frame is 6172 segments
  // and 25 MB; its K2 + K4 were 10 + 9.6 us as launches, VERDICT r05 #2 iii -- every workgroup adds up what it needs itself)
  static const bool no_fuse_big = getenv("SJPEG_HIP_NO_FUSED_BIG") != nullptr;      // (A/B)
  const bool fuse_ok = !no_fuse_k4 && !piped && s.pack_off == nullptr && !a.rst && static_cast<size_t>(nframes) * g.nseg <= 8192;
  s.fused_k4 = !fuse_ok ? 0 : max_chunks <= kFusedChunks ? 1 : (nframes == 1 && !no_fuse_big && max_chunks <= kFusedChunksBig) ? 2 : 0;
  static const bool no_fuse_k2 = getenv("SJPEG_HIP_NO_FUSED_K2") != nullptr;        // (A/B)
  // (the fused K3 keeps bit offsets in 32 bits: max_chunks <= 2^17 chunks of 4 KiB = 2^32 bits)
  s.fused_k2 = (!s.fused_k4 || no_fuse_k2 || e->ablate != 0) ? 0 : (s.fused_k4 == 1 && g.nseg <= kFusedSegs) ? 1 : (g.nseg <= kFusedSegsBig && nframes == 1 && !no_fuse_big) ? 2 : 0;
  if (s.fused_k2) {                                // K1 clears the 0xFF counters K2 would have
    a.clear_ff = e->chunk_ff.p; a.clear_n = max_chunks;
    a.clear_per = (max_chunks + static_cast<uint32_t>(g.nseg) - 1u) / static_cast<uint32_t>(g.nseg);
  }

  if ((rc = sync_uploads(e, st))) return rc;
  if (hs != st && (rc = sync_uploads(e, hs))) return rc;
  if (e->timing) HIP_TRY(hipEventRecord(e->ev[0], st));
  if (tables->flags & SJPEG_HIP_QUANT_REPLAY) {
    const int first = e->replay_total > 0 ? e->replay_first : 0;
    const int total = e->replay_total > 0 ? e->replay_total : nframes;
    if (e->replay.p == nullptr || e->replay_w != width || e->replay_h != height || e->replay_mode != yuv_mode ||
        e->replay_nframes != total || first < 0 || first + nframes > total) {
      return fail(SJPEG_HIP_EINVAL, "SJPEG_HIP_QUANT_REPLAY: no kept coefficients of this geometry "
                                    "(run the statistics pass with SJPEG_HIP_QUANT_KEEP first)");
    }
    a.replay = e->replay.p + static_cast<size_t>(first) * g.nseg * kScanThreads * 36;
    rc = launch_scan<kKindEncodeReplay>(yuv_mode, cls, dim3(g.nseg, nframes), st, a);
  } else if (tables->flags & SJPEG_HIP_QUANT_TRELLIS) {
    rc = launch_scan<kKindEncodeTrellis>(yuv_mode, cls, dim3(g.nseg, nframes), st, a);
  } else {
    rc = launch_scan<kKindEncode>(yuv_mode, cls, dim3(g.nseg, nframes), st, a);
  }
  if (rc) return rc;
  dbg_mark("encode: K1 launched");
  if (e->timing) HIP_TRY(hipEventRecord(e->ev[1], st));
  if (piped) {
    HIP_TRY(hipEventRecord(e->k1_done, st));
    dbg_mark("encode: k1_done recorded");
    HIP_TRY(hipStreamWaitEvent(hs, e->k1_done, 0));
    dbg_mark("encode: side waits k1_done");
  }

  if (!s.fused_k2) {
    hipLaunchKernelGGL(scan_seg_offsets<>, dim3(nframes), dim3(kThreads), 0, hs, s);
    HIP_TRY(hipGetLastError());
  }
  dbg_mark("encode: K2 launched");
  // the chunk count is only known on the device: a fixed grid strides over the chunks
  uint32_t gx = 4096u / static_cast<uint32_t>(nframes);
  if (gx < 64) gx = 64;
  if (gx > max_chunks) gx = max_chunks;
  if (s.fused_k2 == 2) hipLaunchKernelGGL(place_segments<2>, dim3((g.nseg * s.subs + 3) / 4, nframes), dim3(kThreads), 0, hs, s);
  else if (s.fused_k2) hipLaunchKernelGGL(place_segments<1>, dim3((g.nseg * s.subs + 3) / 4, nframes), dim3(kThreads), 0, hs, s);
  else hipLaunchKernelGGL(place_segments<0>, dim3((g.nseg * s.subs + 3) / 4, nframes), dim3(kThreads), 0, hs, s);
  HIP_TRY(hipGetLastError());
  if (!s.fused_k4) {
    hipLaunchKernelGGL(scan_chunk_offsets<>, dim3(nframes), dim3(kThreads), 0, hs, s);
    HIP_TRY(hipGetLastError());
  }
  e->ctr_clean_at[set] = a.pool_ctr; e->ctr_clean_n[set] = static_cast<size_t>(nframes);
  dbg_mark("encode: K3 K4 launched");
  if (piped) {                                     // (K4 is the last reader of this set: it looks at the pool's overrun flag)
    HIP_TRY(hipEventRecord(e->k3_done[set], hs));
    dbg_mark("encode: k3_done recorded");
    e->k3_pending[set] = true;
    e->set = set ^ 1;
  }
  if (s.pack_off != nullptr) {                     // packed output: the frames' places, then header / EOI / padding
    hipLaunchKernelGGL(pack_frame_offsets, dim3(1), dim3(kThreads), 0, hs, s);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pack_frame_edges, dim3(nframes), dim3(kThreads), 0, hs, s);
    HIP_TRY(hipGetLastError());
  }
  if (s.fused_k4 == 2) hipLaunchKernelGGL(stuff_chunks<2>, dim3(gx, nframes), dim3(kThreads), 0, hs, s);
  else if (s.fused_k4) hipLaunchKernelGGL(stuff_chunks<1>, dim3(gx, nframes), dim3(kThreads), 0, hs, s);
  // (not fused: one wave per chunk over max_chunks, four to a workgroup -- the chunk count is on the device)
  else hipLaunchKernelGGL(stuff_chunks_wave, dim3((max_chunks + 3u) / 4u, nframes), dim3(kThreads), 0, hs, s);
  HIP_TRY(hipGetLastError());
  dbg_mark("encode: K5 launched");
  if (a.rst && g.nseg - 1 + rst_tail > 0) {
    hipLaunchKernelGGL(patch_restart_markers, dim3((g.nseg - 1 + rst_tail + 3) / 4, nframes), dim3(kThreads), 0, hs, s);
    HIP_TRY(hipGetLastError());
  }
  if (piped) {
    e->side_pending = true;                        // (side_done itself: side_mark(), when somebody waits for it)
    e->side_recorded = false;
  }
  if (e->timing) {
    HIP_TRY(hipEventRecord(e->ev[2], hs));
    e->ev_valid = true;
  }
  return 0;
}

// A batch whose segment scratch would pass the engine's limit (SJPEG_HIP_SCRATCH_LIMIT_BYTES, 16 GiB by default: 64 8K
// 4:4:4 frames would take 21 GB in pipelined mode, sized as it is from out_stride alone -- VERDICT r04 #10) is coded
// as several launches of as many frames as the limit holds; the calls queue behind each other like any others (and
// pipeline with each other in pipelined mode).  Packed output and band calls are one launch by construction.
static int encode_scan_impl(sjpeg_hip_engine* e, const sjpeg_hip_source* src, int width, int height,
                            int yuv_mode, int nframes, const sjpeg_hip_scan_tables* tables,
                            const void* header, size_t header_size, const size_t* header_offsets,
                            int append_eoi, void* d_out, size_t out_stride, uint64_t* d_sizes,
                            void* stream, const int* seg_range = nullptr, uint64_t* d_pack_off = nullptr) {
  FrameGeo g;
  if (e != nullptr && src != nullptr && nframes > 1 && seg_range == nullptr && d_pack_off == nullptr && d_out != nullptr && d_sizes != nullptr &&
      frame_geo(width, height, yuv_mode, &g)) {
    const SegPlan plan = seg_plan(g, out_stride > 0 ? out_stride : 1);
    const size_t per_frame = ((static_cast<size_t>(g.nseg) * plan.slot_words + plan.pool_words) * (e->pipelined ? 2 : 1) + plan.ubuf_words) * sizeof(uint32_t);
    size_t fit = per_frame == 0 ? static_cast<size_t>(nframes) : e->scratch_limit / per_frame;
    if (fit < 1) fit = 1;
    if (fit < static_cast<size_t>(nframes)) {
      // (a replay call addresses the kept blocks of frames [replay_first, replay_first + nframes) of a buffer for
      // replay_total frames: every launch its own range of it)
      const bool replay = tables != nullptr && (tables->flags & SJPEG_HIP_QUANT_REPLAY) != 0;
      // (the launches share what is uploaded once for all of them -- the header blob -- and follow each other: their
      // uploads stay in the call's stream)
      struct Restore { sjpeg_hip_engine* e; int first, total; hipStream_t up; ~Restore() { e->replay_first = first; e->replay_total = total; e->up_stream = up; } } restore{e, e->replay_first, e->replay_total, e->up_stream};
      e->up_stream = nullptr;
      if (replay && e->replay_total <= 0) { e->replay_total = nframes; e->replay_first = 0; }
      const int base_first = e->replay_first;
      for (int f0 = 0; f0 < nframes; f0 += static_cast<int>(fit)) {
        if (replay) e->replay_first = base_first + f0;
        const int nf = nframes - f0 < static_cast<int>(fit) ? nframes - f0 : static_cast<int>(fit);
        sjpeg_hip_source part = *src;
        for (int i = 0; i < 3; ++i) {
          if (part.plane[i] != nullptr) part.plane[i] = static_cast<const uint8_t*>(part.plane[i]) + static_cast<int64_t>(f0) * part.frame_stride[i];
        }
        const bool multi = header_offsets != nullptr;
        const int rc = encode_scan_one(e, &part, width, height, yuv_mode, nf, multi ? tables + f0 : tables, header, header_size,
                                       multi ? header_offsets + f0 : nullptr, append_eoi, static_cast<uint8_t*>(d_out) + static_cast<size_t>(f0) * out_stride,
                                       out_stride, d_sizes + f0, stream);
        if (rc) return rc;
      }
      return 0;
    }
  }
  return encode_scan_one(e, src, width, height, yuv_mode, nframes, tables, header, header_size, header_offsets, append_eoi,
                         d_out, out_stride, d_sizes, stream, seg_range, d_pack_off);
}

int sjpeg_hip_encode_scan_src(sjpeg_hip_engine* e, const sjpeg_hip_source* src, int width, int height,
                              int yuv_mode, int nframes, const sjpeg_hip_scan_tables* tables,
                              const void* header, size_t header_size, int append_eoi, void* d_out,
                              size_t out_stride, uint64_t* d_sizes, void* stream) {
  return encode_scan_impl(e, src, width, height, yuv_mode, nframes, tables, header, header_size, nullptr,
                          append_eoi, d_out, out_stride, d_sizes, stream);
}

int sjpeg_hip_encode_scan_packed_src(sjpeg_hip_engine* e, const sjpeg_hip_source* src, int width, int height,
                                     int yuv_mode, int nframes, const sjpeg_hip_scan_tables* tables,
                                     const void* header, size_t header_size, int append_eoi, void* d_out,
                                     size_t out_stride, uint64_t* d_sizes, uint64_t* d_offsets, void* stream) {
  if (d_offsets == nullptr) return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_encode_scan_packed_src: d_offsets == NULL");
  return encode_scan_impl(e, src, width, height, yuv_mode, nframes, tables, header, header_size, nullptr,
                          append_eoi, d_out, out_stride, d_sizes, stream, nullptr, d_offsets);
}

int sjpeg_hip_encode_intervals_src(sjpeg_hip_engine* e, const sjpeg_hip_source* src, int width, int height,
                                   int yuv_mode, const sjpeg_hip_scan_tables* tables, int seg_begin, int seg_end,
                                   void* d_out, size_t out_cap, uint64_t* d_size, void* stream) {
  if (tables == nullptr || !(tables->flags & SJPEG_HIP_RESTART_MARKERS)) {
    return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_encode_intervals_src needs tables with SJPEG_HIP_RESTART_MARKERS");
  }
  const int range[2] = {seg_begin, seg_end};
  return encode_scan_impl(e, src, width, height, yuv_mode, 1, tables, nullptr, 0, nullptr, /*append_eoi=*/0,
                          d_out, out_cap, d_size, stream, range);
}

int sjpeg_hip_encode_scan_multi(sjpeg_hip_engine* e, const sjpeg_hip_source* src, int width, int height,
                                int yuv_mode, int nframes, const sjpeg_hip_scan_tables* tables,
                                const void* headers, const size_t* header_offsets, int append_eoi,
                                void* d_out, size_t out_stride, uint64_t* d_sizes, void* stream) {
  if (tables == nullptr || headers == nullptr || header_offsets == nullptr || nframes <= 0) {
    return fail(SJPEG_HIP_EINVAL, "null argument or nframes <= 0");
  }
  return encode_scan_impl(e, src, width, height, yuv_mode, nframes, tables, headers, header_offsets[nframes],
                          header_offsets, append_eoi, d_out, out_stride, d_sizes, stream);
}

int sjpeg_hip_scan_symbol_stats_multi(sjpeg_hip_engine* e, const sjpeg_hip_source* src, int width, int height,
                                      int yuv_mode, int nframes, const sjpeg_hip_scan_tables* tables,
                                      uint32_t* d_freq, void* stream) {
  if (tables == nullptr) return fail(SJPEG_HIP_EINVAL, "tables == NULL");
  return scan_statistics(e, src, width, height, yuv_mode, nframes, tables, false, d_freq, stream, true);
}

// ==== ragged batches: pictures of different sizes in one call ====================================================
// Every frame has its own geometry, planes, output place and capacity; they share the source format, the yuv_mode and
// method 0.  The segment scratch is laid out frame after frame by prefix sums (a frame takes what ITS capacity asks,
// seg_plan), every kernel runs a flat grid over the launch's total work, and a workgroup finds its frame in a
// workgroup -> frame map built here beside the descriptors (RaggedFrame, scan_device.h).  A batch whose scratch would
// pass the engine's limit goes in several launches over consecutive frame ranges.  DESIGN.md section 4.
namespace {

struct RaggedLaunch {
  int f0, nf;
  uint32_t segs, place_wgs, stuff_wgs, chunks;
  size_t pool_words, ubuf_words;
  size_t k1_map, place_map, stuff_map;     // where the launch's maps start in the u32 part of the blob
  size_t hdr_bytes;                        // its frames' headers: staged launch by launch (sjpeg_hip_engine::hdr_stage)
  size_t hoff;                             // where its nf + 1 header offsets start in the blob's offsets
};

// The source format of a ragged call (as prepare_scan): the kernel's per-format fields in *a (zeroed first), the source
// class and the format's row.  who: the entry point, for the messages.
int format_fields(const std::string& who, int format, int yuv_mode, ScanArgs* a, int* cls, const SourceLayout** layout) {
  memset(a, 0, sizeof(*a));
  const SourceLayout* const L = source_layout(format);
  if (L == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": unknown source format");
  *cls = L->cls; *layout = L;
  layout_args(*L, a);                          // (the engine's pixel transform: ragged_encode / ragged_analysis put it in)
  if (yuv_mode != SJPEG_HIP_YUV420 && yuv_mode != SJPEG_HIP_YUV444 && yuv_mode != SJPEG_HIP_YUV400) {
    return fail(SJPEG_HIP_EINVAL, who + ": bad yuv_mode");
  }
  if (L->implied != 0 && yuv_mode != L->implied) return fail(SJPEG_HIP_EINVAL, who + ": yuv_mode does not match the source format");
  return 0;
}

// a frame's planes (the kernels' three out of the caller's: layout_planes) and geometry in its descriptor
void ragged_geometry(const SourceLayout& L, const sjpeg_hip_ragged_frame& fr, const FrameGeo& g, RaggedFrame* d) {
  layout_planes(L, fr.plane, fr.row_stride, nullptr, d->plane, d->row_stride, nullptr);
  d->W = fr.width; d->H = fr.height; d->mb_w = g.mb_w; d->n_mcus = g.n_mcus; d->nseg = g.nseg;
  d->has_clip = (fr.width % g.px != 0) || (fr.height % g.px != 0);
}

}  // namespace

}  // extern "C"

// the checks of format_fields alone, for the flows: the launch layer derives the fields again from the format
int sjpeg_internal::ragged_format(const std::string& who, int format, int yuv_mode) {
  ScanArgs a;
  int cls = 0;
  const SourceLayout* layout = nullptr;
  return format_fields(who, format, yuv_mode, &a, &cls, &layout);
}

// Every frame of a ragged call of a known format checked (the message names the frame); its geometry into (*geo)[f].
// out_ranges: the frames' output ranges are checked too (the encodes; the analysis passes ignore them).
int sjpeg_internal::ragged_frames(const std::string& who, int format, int yuv_mode, int nframes,
                                  const sjpeg_hip_ragged_frame* frames, bool out_ranges, std::vector<FrameGeo>* geo, int esz) {
  geo->resize(nframes);
  SourceLayout L = *source_layout(format);
  if (esz != 0) L.esz = esz;                     // (the deep entries: the format's planes with samples of esz bytes)
  for (int f = 0; f < nframes; ++f) {
    const sjpeg_hip_ragged_frame& fr = frames[f];
    const std::string w = who + ": frame " + std::to_string(f) + ": ";
    if (!frame_geo(fr.width, fr.height, yuv_mode, &(*geo)[f])) {
      return fail(SJPEG_HIP_EINVAL, w + "bad dimensions " + std::to_string(fr.width) + "x" + std::to_string(fr.height));
    }
    const LayoutFault fault = layout_fault(L, fr.width, fr.plane, fr.row_stride, nullptr, kRaggedChecks);
    if (fault.rule != kFaultNone) return fail(SJPEG_HIP_EINVAL, w + layout_fault_text(L, fault));
    if (out_ranges && fr.out_capacity > UINT64_MAX - fr.out_offset) return fail(SJPEG_HIP_EINVAL, w + "out_offset + out_capacity overflows");
  }
  return 0;
}

extern "C" int sjpeg_hip_encode_ragged_src(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_scan_tables* tables,
                                int tables_per_frame, const void* headers, const size_t* header_offsets,
                                int append_eoi, void* d_out, uint64_t* d_sizes, void* stream) {
  static const std::string kWhoEncode = "sjpeg_hip_encode_ragged_src";
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_encode_ragged_src: engine == NULL");
  if (frames == nullptr || tables == nullptr || d_out == nullptr || d_sizes == nullptr) {
    return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_encode_ragged_src: frames, tables, d_out or d_sizes == NULL");
  }
  if (nframes < 1 || nframes > 65535) return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_encode_ragged_src: nframes must be 1..65535");
  if ((headers == nullptr) != (header_offsets == nullptr)) {
    return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_encode_ragged_src: headers and header_offsets go together");
  }
  const int ntab = tables_per_frame ? nframes : 1;
  constexpr uint32_t kNotRagged = SJPEG_HIP_QUANT_TRELLIS | SJPEG_HIP_QUANT_KEEP | SJPEG_HIP_QUANT_REPLAY | SJPEG_HIP_RESTART_MARKERS;
  for (int t = 0; t < ntab; ++t) {
    if (tables[t].flags & kNotRagged) {
      return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_encode_ragged_src: tables[" + std::to_string(t) +
                                        "]: trellis, keep / replay and restart-marker flags are not taken by ragged batches");
    }
  }
  if (int rcf = ragged_format(kWhoEncode, format, yuv_mode)) return rcf;
  size_t header_size = 0;
  if (header_offsets != nullptr) {
    for (int f = 0; f <= nframes; ++f) {
      // (a launch addresses its staged headers with 32-bit offsets: one header stays below 4 GiB, the launches are cut)
      if (f > 0 && (header_offsets[f] < header_offsets[f - 1] || header_offsets[f] - header_offsets[f - 1] > 0xffffffffu)) {
        return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_encode_ragged_src: header_offsets[" + std::to_string(f) + "] must ascend (below 4 GiB)");
      }
    }
    header_size = header_offsets[nframes];
  }
  // per frame: checks, geometry
  std::vector<FrameGeo> geo;
  if (int rcg = ragged_frames(kWhoEncode, format, yuv_mode, nframes, frames, true, &geo)) return rcg;
  try {
    return ragged_encode(e, format, yuv_mode, nframes, frames, geo, tables, tables_per_frame, headers, header_offsets,
                         header_size, append_eoi, d_out, d_sizes, static_cast<hipStream_t>(stream), nullptr);
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

// The ragged encode of checked frames (ragged_frames, ragged_format): K1 kKindEncodeRagged, K2 .. K5.  d_bits != NULL:
// a count without output (sjpeg_hip_scan_counted_bits_ragged_src) -- K1 .. K3, then counted_bits_ragged instead of
// K4 and K5, no header, nothing written to d_out or d_sizes; the frames' out_capacity plans the segment scratch only.
// kept != NULL: K1 is kKindEncodeReplayRagged -- it codes the blocks a trellis statistics pass left at `kept` and reads no
// pixel; frame f's lie kept_base[f] segments behind `kept`, kKeptSegWords a segment (ragged_analysis, kPassStatsTrellis:
// the same table, so a frame's blocks have one place whichever frames a launch covers).
// sink != NULL: packed output -- d_out and the frames' out_offset are not used; per launch K4 leaves the sizes only,
// place_ragged_frames puts the launch's frames behind the engine's cursor (each start into its descriptor, where K5
// takes it from, and into the caller's offsets), pack_ragged_edges writes header, EOI and padding (stitch_kernels.h).
int sjpeg_internal::ragged_encode(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                  const sjpeg_hip_ragged_frame* frames, const std::vector<FrameGeo>& geo,
                                  const sjpeg_hip_scan_tables* tables, int tables_per_frame, const void* headers,
                                  const size_t* header_offsets, size_t header_size, int append_eoi, void* d_out, uint64_t* d_sizes,
                                  hipStream_t st, unsigned long long* d_bits, uint32_t* kept, const PackedSink* sink,
                                  const uint32_t* kept_base) {
  ScanArgs a;                                     // the format's fields, its source class and its row
  int cls = kSrcPlanes;
  const SourceLayout* layout = nullptr;
  if (int rcf = format_fields("internal", format, yuv_mode, &a, &cls, &layout)) return rcf;
  put_transform(e, &a);                           // (the float class's pixel transform)
  const int ntab = tables_per_frame ? nframes : 1;
  if (kept != nullptr && kept_base == nullptr) return fail(SJPEG_HIP_EINVAL, "internal: the ragged replay takes its frames' kept bases");
  if (sink != nullptr && (d_bits != nullptr || d_sizes == nullptr)) return fail(SJPEG_HIP_EINVAL, "internal: packed output needs the sizes");
  std::vector<SegPlan> plan(nframes);
  std::vector<uint32_t> max_chunks(nframes);
  for (int f = 0; f < nframes; ++f) {
    const sjpeg_hip_ragged_frame& fr = frames[f];
    plan[f] = seg_plan(geo[f], fr.out_capacity > 0 ? static_cast<size_t>(fr.out_capacity) : 1);
    max_chunks[f] = static_cast<uint32_t>((plan[f].ubuf_words + kChunkWords - 1) / kChunkWords);
  }

  // launches over consecutive frame ranges, each inside the engine's scratch limit (one frame at least); the blob's
  // maps: K1 one entry per segment, K3 one per workgroup of four segments, K5 one per workgroup
  std::vector<RaggedLaunch> launches;
  size_t map_words = 0;
  {
    RaggedLaunch cur = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};     // (the fields not named: zero)
    uint32_t slot_max = 0;
    auto bytes_of = [](size_t segs, uint32_t slot, size_t pool, size_t ubuf) { return (segs * slot + pool + ubuf) * sizeof(uint32_t); };
    for (int f = 0; f < nframes; ++f) {
      const uint32_t slot = std::max(slot_max, plan[f].slot_words);
      const size_t pool_f = (static_cast<size_t>(plan[f].pool_words) + 3) & ~size_t(3);
      // (the staged headers are scratch like the rest, and one launch's stay below 4 GiB: 32-bit offsets)
      const size_t hdr_f = header_offsets != nullptr ? header_offsets[f + 1] - header_offsets[f] : 0;
      if (cur.nf > 0 && (bytes_of(static_cast<size_t>(cur.segs) + geo[f].nseg, slot, cur.pool_words + pool_f, cur.ubuf_words + plan[f].ubuf_words) +
                                 cur.hdr_bytes + hdr_f > e->scratch_limit ||
                         static_cast<size_t>(cur.segs) + geo[f].nseg > (1u << 30) || cur.hdr_bytes + hdr_f > 0xffffffffull)) {
        launches.push_back(cur);
        cur = {f, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        slot_max = 0;
      }
      cur.hdr_bytes += hdr_f;
      slot_max = std::max(slot_max, plan[f].slot_words);
      cur.nf += 1;
      cur.segs += static_cast<uint32_t>(geo[f].nseg);
      cur.pool_words += pool_f;
      cur.ubuf_words += plan[f].ubuf_words;
      cur.chunks += max_chunks[f];
    }
    launches.push_back(cur);
    for (RaggedLaunch& l : launches) {
      l.place_wgs = l.stuff_wgs = 0;
      uint32_t gx = 4096u / static_cast<uint32_t>(l.nf);           // K5 workgroups per frame, as a uniform launch of nf frames
      if (gx < 64) gx = 64;
      for (int f = l.f0; f < l.f0 + l.nf; ++f) {
        l.place_wgs += static_cast<uint32_t>((geo[f].nseg + 3) / 4);
        l.stuff_wgs += std::min(gx, max_chunks[f]);
      }
      l.k1_map = map_words; l.place_map = l.k1_map + l.segs; l.stuff_map = l.place_map + l.place_wgs;
      map_words = l.stuff_map + l.stuff_wgs;
      l.hoff = static_cast<size_t>(l.f0) + static_cast<size_t>(&l - launches.data());     // (nf + 1 offsets a launch)
    }
  }

  // the blob: descriptors | digested tables | maps | header offsets (per launch: its nf + 1, from the first of its
  // headers) | header bytes (a call of ONE launch: they travel with the blob, no upload of their own; a call of several
  // stages each launch's in hdr_stage) | (packed) the caller's frame numbers
  const bool hdr_in_blob = launches.size() == 1;
  const size_t off_tab = align16(sizeof(RaggedFrame) * nframes);
  const size_t off_map = off_tab + sizeof(DevTables) * ntab;
  const size_t off_hoff = align16(off_map + map_words * sizeof(uint32_t));
  const size_t off_hdr = align16(off_hoff + (header_offsets != nullptr ? (static_cast<size_t>(nframes) + launches.size()) * sizeof(uint32_t) : 0));
  const size_t off_pidx = align16(off_hdr + (hdr_in_blob ? launches[0].hdr_bytes : 0));
  const size_t blob_bytes = align16(off_pidx + (sink != nullptr ? static_cast<size_t>(nframes) * sizeof(uint32_t) : 0));
  std::vector<uint4> blob(blob_bytes / 16);
  uint8_t* const hb = reinterpret_cast<uint8_t*>(blob.data());
  RaggedFrame* const desc = reinterpret_cast<RaggedFrame*>(hb);
  for (int t = 0; t < ntab; ++t) digest_tables(tables + t, reinterpret_cast<DevTables*>(hb + off_tab) + t);
  uint32_t* const maps = reinterpret_cast<uint32_t*>(hb + off_map);
  std::vector<uint32_t> slot_of(launches.size());
  for (size_t li = 0; li < launches.size(); ++li) {
    const RaggedLaunch& l = launches[li];
    uint32_t slot = 0;
    for (int f = l.f0; f < l.f0 + l.nf; ++f) slot = std::max(slot, plan[f].slot_words);
    slot_of[li] = slot;
    uint32_t seg = 0, place = 0, stuff = 0, chunk = 0;
    unsigned long long pool = 0, ubuf = 0;
    uint32_t gx = 4096u / static_cast<uint32_t>(l.nf);
    if (gx < 64) gx = 64;
    for (int f = l.f0; f < l.f0 + l.nf; ++f) {
      const sjpeg_hip_ragged_frame& fr = frames[f];
      const FrameGeo& g = geo[f];
      RaggedFrame& d = desc[f];
      ragged_geometry(*layout, fr, g, &d);
      d.seg_base = seg; d.pool_base = pool; d.pool_words = plan[f].pool_words;
      d.ubuf_base = ubuf; d.ubuf_words = static_cast<uint32_t>(plan[f].ubuf_words);
      d.chunk_base = chunk; d.max_chunks = max_chunks[f];
      d.out_offset = fr.out_offset; d.out_capacity = fr.out_capacity;
      d.place_base = place;
      d.kept_base = kept != nullptr ? kept_base[f] : 0u;
      d.stuff_base = stuff; d.stuff_wgs = std::min(gx, max_chunks[f]);
      const uint32_t fl = static_cast<uint32_t>(f - l.f0);
      for (int k = 0; k < g.nseg; ++k) maps[l.k1_map + seg + k] = fl;
      for (int k = 0; k < (g.nseg + 3) / 4; ++k) maps[l.place_map + place + k] = fl;
      for (uint32_t k = 0; k < d.stuff_wgs; ++k) maps[l.stuff_map + stuff + k] = fl;
      seg += static_cast<uint32_t>(g.nseg); place += static_cast<uint32_t>((g.nseg + 3) / 4); stuff += d.stuff_wgs;
      chunk += max_chunks[f];
      pool += (static_cast<unsigned long long>(plan[f].pool_words) + 3) & ~3ull;
      ubuf += plan[f].ubuf_words;
    }
  }
  size_t n_hdr = 0;
  if (header_offsets != nullptr) {
    uint32_t* const ho = reinterpret_cast<uint32_t*>(hb + off_hoff);
    for (const RaggedLaunch& l : launches) {
      for (int k = 0; k <= l.nf; ++k) ho[l.hoff + k] = static_cast<uint32_t>(header_offsets[l.f0 + k] - header_offsets[l.f0]);
      if (!hdr_in_blob) n_hdr = std::max(n_hdr, l.hdr_bytes);
    }
    if (hdr_in_blob && launches[0].hdr_bytes > 0) memcpy(hb + off_hdr, static_cast<const uint8_t*>(headers) + header_offsets[0], launches[0].hdr_bytes);
  }
  if (sink != nullptr) {
    uint32_t* const pi = reinterpret_cast<uint32_t*>(hb + off_pidx);
    for (int f = 0; f < nframes; ++f) pi[f] = static_cast<uint32_t>(sink->index != nullptr ? sink->index[f] : f);
  }

  // scratch for the largest launch
  if (int rc0 = ragged_ordered(e, st)) return rc0;   // (pipelined mode: the call runs ordered, behind the engine's stitch)
  size_t n_segs = 0, n_words = 0, n_pool = 0, n_ubuf = 0, n_chunks = 0, n_f = 0, n_off = 0;
  for (size_t li = 0; li < launches.size(); ++li) {
    const RaggedLaunch& l = launches[li];
    n_segs = std::max(n_segs, static_cast<size_t>(l.segs));
    n_words = std::max(n_words, static_cast<size_t>(l.segs) * slot_of[li]);
    n_pool = std::max(n_pool, l.pool_words);
    n_ubuf = std::max(n_ubuf, l.ubuf_words);
    n_chunks = std::max(n_chunks, static_cast<size_t>(l.chunks));
    n_f = std::max(n_f, static_cast<size_t>(l.nf));
    n_off = std::max(n_off, static_cast<size_t>(l.segs) + l.nf);
  }
  int rc;
  if ((rc = e->ragged.ensure(blob.size())) || (rc = e->seg_nbits.ensure(n_segs)) || (rc = e->seg_words.ensure(n_words)) ||
      (rc = e->pool.ensure(n_pool)) || (rc = e->pool_ctr.ensure(2 * n_f)) || (rc = e->seg_xbase.ensure(n_segs)) ||
      (rc = e->seg_off.ensure(n_off)) || (rc = e->ubuf.ensure(n_ubuf)) || (rc = e->chunk_ff.ensure(n_chunks)) ||
      (rc = e->chunk_off.ensure(n_chunks)) || (rc = e->frame_flags.ensure(n_f)) || (n_hdr > 0 && (rc = e->hdr_stage.ensure(n_hdr / 16 + 1)))) {
    return rc;
  }
  if (sink != nullptr && e->pack_cursor.p == nullptr) return fail(SJPEG_HIP_EINVAL, "internal: packed output without its cursor");
  if ((rc = upload(e, e->ragged.p, blob.data(), blob_bytes, st))) return rc;
  if ((rc = sync_uploads(e, st))) return rc;
  const uint8_t* const db = reinterpret_cast<const uint8_t*>(e->ragged.p);
  const uint32_t* const dmaps = reinterpret_cast<const uint32_t*>(db + off_map);
  e->ctr_clean_at[0] = e->ctr_clean_at[1] = nullptr;   // (the pool counters are this call's now; its K2s leave them at zero)
  e->last_nseg = e->last_nframes = 0;                  // (sjpeg_hip_engine_entropy_bits: not after a ragged call)
  if (e->timing) HIP_TRY(hipEventRecord(e->ev[0], st));
  for (size_t li = 0; li < launches.size(); ++li) {
    const RaggedLaunch& l = launches[li];
    HIP_TRY(hipMemsetAsync(e->pool_ctr.p, 0, static_cast<size_t>(l.nf) * 2 * sizeof(uint32_t), st));
    a.tables = reinterpret_cast<const DevTables*>(db + off_tab) + (tables_per_frame ? l.f0 : 0);
    a.tables_stride = tables_per_frame ? 1 : 0;
    a.seg_words = e->seg_words.p; a.slot_words = slot_of[li];
    a.seg_nbits = e->seg_nbits.p; a.seg_xbase = e->seg_xbase.p;
    a.pool = e->pool.p; a.pool_ctr = e->pool_ctr.p;
    a.ablate = e->ablate;
    a.rframes = reinterpret_cast<const RaggedFrame*>(db) + l.f0;
    a.rmap = dmaps + l.k1_map;
    if (kept != nullptr) {
      a.replay = kept;                                 // (every frame's own place: RaggedFrame::kept_base)
      rc = launch_scan_src<kKindEncodeReplayRagged, kSrcRgb24>(yuv_mode, dim3(l.segs), st, a);   // (reads no pixel)
    } else {
      rc = launch_scan<kKindEncodeRagged>(yuv_mode, cls, dim3(l.segs), st, a);
    }
    if (rc) return rc;
    if (e->timing && li + 1 == launches.size()) HIP_TRY(hipEventRecord(e->ev[1], st));
    // the launch's headers: behind the stitch kernels of the launch in front, which read theirs from the same place
    if (!hdr_in_blob && l.hdr_bytes > 0 && d_bits == nullptr) {
      if ((rc = upload(e, e->hdr_stage.p, static_cast<const uint8_t*>(headers) + header_offsets[l.f0], l.hdr_bytes, st))) return rc;
      if ((rc = sync_uploads(e, st))) return rc;
    }
    StitchArgs s{};
    s.nframes = l.nf;
    s.seg_nbits = e->seg_nbits.p; s.seg_off = e->seg_off.p;
    s.seg_words = e->seg_words.p; s.slot_words = slot_of[li];
    s.pool = e->pool.p; s.seg_xbase = e->seg_xbase.p; s.pool_ctr = e->pool_ctr.p;
    s.ubuf = e->ubuf.p; s.chunk_ff = e->chunk_ff.p; s.chunk_off = e->chunk_off.p;
    s.header = hdr_in_blob ? db + off_hdr : reinterpret_cast<const uint8_t*>(e->hdr_stage.p); s.header_size = 0;
    s.hdr_off = header_offsets != nullptr ? reinterpret_cast<const uint32_t*>(db + off_hoff) + l.hoff : nullptr;
    s.append_eoi = append_eoi;
    s.out = static_cast<uint8_t*>(sink != nullptr ? sink->base : d_out);
    s.sizes = d_sizes != nullptr ? reinterpret_cast<unsigned long long*>(d_sizes) + l.f0 : nullptr;
    s.subs = 1; s.wide_subs = 0;
    s.frame_flags = e->frame_flags.p;
    s.rframes = a.rframes; s.rmap_place = dmaps + l.place_map; s.rmap_stuff = dmaps + l.stuff_map;
    hipLaunchKernelGGL(scan_seg_offsets<true>, dim3(l.nf), dim3(kThreads), 0, st, s);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((place_segments<0, true>), dim3(l.place_wgs), dim3(kThreads), 0, st, s);
    HIP_TRY(hipGetLastError());
    if (d_bits != nullptr) {
      hipLaunchKernelGGL(counted_bits_ragged, dim3(l.nf), dim3(kThreads), 0, st, s, d_bits + l.f0);
      HIP_TRY(hipGetLastError());
      continue;
    }
    if (sink != nullptr) {
      // K4 with pack_off set leaves the size only (what it points at is never read: the starts go into the descriptors)
      StitchArgs s4 = s;
      s4.pack_off = e->pack_cursor.p;
      hipLaunchKernelGGL(scan_chunk_offsets<true>, dim3(l.nf), dim3(kThreads), 0, st, s4);
      HIP_TRY(hipGetLastError());
      PackArgs p;
      p.nframes = l.nf; p.total = static_cast<uint32_t>(sink->nframes);
      p.sizes = s.sizes;
      p.rframes = const_cast<RaggedFrame*>(s.rframes);
      p.index = reinterpret_cast<const uint32_t*>(db + off_pidx) + l.f0;
      p.offsets = reinterpret_cast<unsigned long long*>(sink->d_offsets);
      p.capacity = sink->capacity;
      p.cursor = e->pack_cursor.p;
      hipLaunchKernelGGL(place_ragged_frames, dim3(1), dim3(kThreads), 0, st, p);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL((stuff_chunks<0, true>), dim3(l.stuff_wgs), dim3(kThreads), 0, st, s);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(pack_ragged_edges, dim3(l.nf), dim3(kThreads), 0, st, s);
      HIP_TRY(hipGetLastError());
      continue;
    }
    hipLaunchKernelGGL(scan_chunk_offsets<true>, dim3(l.nf), dim3(kThreads), 0, st, s);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((stuff_chunks<0, true>), dim3(l.stuff_wgs), dim3(kThreads), 0, st, s);
    HIP_TRY(hipGetLastError());
  }
  if (e->timing) {
    HIP_TRY(hipEventRecord(e->ev[2], st));
    e->ev_valid = true;
  }
  return 0;
}

// The analysis passes over a ragged batch: the histogram (kKindHistoRagged, persistent groups), the symbol statistics
// (kKindStatsRagged, a workgroup per segment) or the quantization error (kKindErrorRagged, a workgroup per segment) of
// frames [0, nframes), then their ragged reduce -- d_out[f] = [2][64][128] or [2][272] words, or one 64-bit total: what
// the uniform pass makes of frame f alone.  The frames have been checked (ragged_frames); `a` holds the format's fields
// (ragged_format).  The partials of a launch stay inside the engine's scratch limit: a larger batch goes in several
// launches over consecutive frames.  kPassStatsTrellis: the statistics with trellis quantization (kKindStatsTrellisRagged;
// tables with SJPEG_HIP_QUANT_TRELLIS); its quantized blocks stay behind at `kept`, frame f's kept_base[f] segments in
// (kKeptSegWords a segment), whatever the launches and whichever frames the call covers -- for ragged_encode to replay.
int sjpeg_internal::ragged_analysis(sjpeg_hip_engine* e, RaggedPass pass, int format, int yuv_mode, int nframes,
                                    const sjpeg_hip_ragged_frame* frames, const std::vector<FrameGeo>& geo,
                                    const sjpeg_hip_scan_tables* tables, int tables_per_frame, uint32_t* d_out, hipStream_t st,
                                    uint32_t* kept, const uint32_t* kept_base) {
  const bool histogram = pass == kPassHisto, error = pass == kPassError, trellis = pass == kPassStatsTrellis;
  ScanArgs a;                                     // the format's fields, its source class and its row
  int cls = kSrcPlanes;
  const SourceLayout* layout = nullptr;
  if (int rcf = format_fields("internal", format, yuv_mode, &a, &cls, &layout)) return rcf;
  put_transform(e, &a);                           // (the float class's pixel transform)
  if (trellis && (kept == nullptr || kept_base == nullptr)) return fail(SJPEG_HIP_EINVAL, "internal: the ragged trellis statistics keep their blocks");
  // a partial: one group's / one segment's; a frame's result (words)
  const size_t part_words = histogram ? kHistoPartialWords : error ? 2 : kStatsWords;
  const int words = histogram ? 2 * 64 * 128 : error ? 2 : kStatsWords;
  // The histogram's groups.  A frame's group count is its own: as many as the uniform launch's 3 x CU slots give it in
  // whole trips over the batch's segments -- at least ceil(nseg / 256) (16-bit counters), at most one per segment.
  const long long slots = e->histo_slots > 0 ? e->histo_slots : 3ll * e->cu_count;
  long long all_segs = 0;
  for (int f = 0; f < nframes; ++f) all_segs += geo[f].nseg;
  const long long trips = std::max(1ll, (all_segs + slots - 1) / slots);
  std::vector<uint32_t> units(nframes);        // K1 workgroups of a frame: groups (histogram) or segments
  for (int f = 0; f < nframes; ++f) {
    const int nseg = geo[f].nseg;
    int g = nseg;
    if (histogram) {
      g = static_cast<int>((nseg + trips - 1) / trips);
      g = std::max(g, (nseg + kHistoMaxSegsPerGroup - 1) / kHistoMaxSegsPerGroup);
      g = std::min(g, nseg);
    }
    units[f] = static_cast<uint32_t>(g);
  }
  // launches: consecutive frames whose partials fit the limit (one frame at least)
  struct Launch { int f0, nf; uint32_t units, max_units; size_t map; };
  std::vector<Launch> launches;
  {
    Launch cur = {0, 0, 0, 0, 0};
    for (int f = 0; f < nframes; ++f) {
      const size_t more = static_cast<size_t>(cur.units) + units[f];
      if (cur.nf > 0 && (more * part_words * sizeof(uint32_t) > e->scratch_limit || more > (1u << 30))) {
        launches.push_back(cur);
        cur = {f, 0, 0, 0, 0};
      }
      cur.nf += 1;
      cur.units += units[f];
      cur.max_units = std::max(cur.max_units, units[f]);
    }
    launches.push_back(cur);
  }
  // the blob: descriptors | digested tables (statistics) | the launches' workgroup -> frame maps
  const int ntab = histogram ? 0 : (tables_per_frame ? nframes : 1);
  const size_t off_tab = align16(sizeof(RaggedFrame) * nframes);
  const size_t off_map = off_tab + sizeof(DevTables) * ntab;
  size_t map_words = 0;
  for (Launch& l : launches) { l.map = map_words; map_words += l.units; }
  const size_t blob_bytes = align16(off_map + map_words * sizeof(uint32_t));
  std::vector<uint4> blob(blob_bytes / 16);
  uint8_t* const hb = reinterpret_cast<uint8_t*>(blob.data());
  RaggedFrame* const desc = reinterpret_cast<RaggedFrame*>(hb);
  for (int t = 0; t < ntab; ++t) digest_tables(tables + t, reinterpret_cast<DevTables*>(hb + off_tab) + t);
  uint32_t* const maps = reinterpret_cast<uint32_t*>(hb + off_map);
  for (const Launch& l : launches) {
    uint32_t base = 0;
    for (int f = l.f0; f < l.f0 + l.nf; ++f) {
      RaggedFrame& d = desc[f];
      ragged_geometry(*layout, frames[f], geo[f], &d);
      d.seg_base = base;                       // (the histogram: its first group -- and partial -- in the launch)
      d.hgroups = histogram ? units[f] : 0u;
      d.kept_base = trellis ? kept_base[f] : 0u;
      for (uint32_t k = 0; k < units[f]; ++k) maps[l.map + base + k] = static_cast<uint32_t>(f - l.f0);
      base += units[f];
    }
  }
  if (int rc0 = ragged_ordered(e, st)) return rc0;   // (pipelined mode: the call runs ordered, behind the engine's stitch)
  size_t n_part = 0;
  for (const Launch& l : launches) n_part = std::max(n_part, static_cast<size_t>(l.units) * part_words);
  int rc;
  if ((rc = e->ragged.ensure(blob.size())) || (rc = e->partial.ensure(n_part))) return rc;
  if ((rc = upload(e, e->ragged.p, blob.data(), blob_bytes, st))) return rc;
  if ((rc = sync_uploads(e, st))) return rc;
  const uint8_t* const db = reinterpret_cast<const uint8_t*>(e->ragged.p);
  for (const Launch& l : launches) {
    a.tables = histogram ? nullptr : reinterpret_cast<const DevTables*>(db + off_tab) + (tables_per_frame ? l.f0 : 0);
    a.tables_stride = tables_per_frame ? 1 : 0;
    a.partial = e->partial.p;
    a.ablate = e->ablate;
    a.rframes = reinterpret_cast<const RaggedFrame*>(db) + l.f0;
    a.rmap = reinterpret_cast<const uint32_t*>(db + off_map) + l.map;
    if (histogram) rc = launch_scan<kKindHistoRagged>(yuv_mode, cls, dim3(l.units), st, a);
    else if (error) rc = launch_scan<kKindErrorRagged>(yuv_mode, cls, dim3(l.units), st, a);
    else if (trellis) {
      a.replay = kept;                               // (every frame's own place: RaggedFrame::kept_base)
      rc = launch_scan<kKindStatsTrellisRagged>(yuv_mode, cls, dim3(l.units), st, a);
    } else rc = launch_scan<kKindStatsRagged>(yuv_mode, cls, dim3(l.units), st, a);
    if (rc) return rc;
    if (error) {                                     // one workgroup per frame sums its segments' partials
      hipLaunchKernelGGL((reduce_error<true, const RaggedFrame*>), dim3(l.nf), dim3(kThreads), 0, st,
                         reinterpret_cast<const unsigned long long*>(e->partial.p), 0,
                         reinterpret_cast<unsigned long long*>(d_out) + l.f0, a.rframes);
      HIP_TRY(hipGetLastError());
      continue;
    }
    // the reduce: slices of the partials as the uniform pass takes them (scan_statistics), for the launch's largest frame
    uint32_t* const out = d_out + static_cast<size_t>(l.f0) * words;
    const int xblocks = histogram ? 32 : (words + kThreads - 1) / kThreads;
    int slices = std::min(32, 4096 / (xblocks * l.nf));
    if (histogram) slices = std::min(slices, static_cast<int>((l.max_units + 255) / 256));
    else if (l.max_units < 64) slices = 1;
    slices = std::max(slices, 1);
    if (!(histogram && slices == 1)) {               // (one slice stores, several add)
      HIP_TRY(hipMemsetAsync(out, 0, static_cast<size_t>(l.nf) * words * sizeof(uint32_t), st));
    }
    const dim3 grid(xblocks, l.nf, slices);
    if (histogram) {
      hipLaunchKernelGGL((reduce_partials16<true, const RaggedFrame*>), grid, dim3(kThreads), 0, st, reinterpret_cast<const uint4*>(e->partial.p), 0, out, a.rframes);
    } else {
      hipLaunchKernelGGL((reduce_partials<true, const RaggedFrame*>), grid, dim3(kThreads), 0, st, e->partial.p, 0, words, out, a.rframes);
    }
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

namespace {

// the checks every ragged analysis entry point starts with; the frames' geometry in *geo
int ragged_analysis_args(const std::string& who, sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                         const sjpeg_hip_ragged_frame* frames, const void* d_out, std::vector<FrameGeo>* geo) {
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (frames == nullptr || d_out == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": frames or the output == NULL");
  if (nframes < 1 || nframes > 65535) return fail(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
  if (int rc = ragged_format(who, format, yuv_mode)) return rc;
  return ragged_frames(who, format, yuv_mode, nframes, frames, false, geo);
}

// the tables of a ragged analysis or count: present, and none with a flag ragged batches do not take
int ragged_tables_ok(const std::string& who, const sjpeg_hip_scan_tables* tables, int ntab) {
  if (tables == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": tables == NULL");
  constexpr uint32_t kNotRagged = SJPEG_HIP_QUANT_TRELLIS | SJPEG_HIP_QUANT_KEEP | SJPEG_HIP_QUANT_REPLAY | SJPEG_HIP_RESTART_MARKERS;
  for (int t = 0; t < ntab; ++t) {
    if (tables[t].flags & kNotRagged) {
      return fail(SJPEG_HIP_EINVAL, who + ": tables[" + std::to_string(t) +
                                        "]: trellis, keep / replay and restart-marker flags are not taken by ragged batches");
    }
  }
  return 0;
}

// The segment scratch a count plans for a frame: the host API's first capacity for its size pass, or the frame's worst
// case (sjpeg_hip_frame_bound)
size_t count_capacity(int W, int H, int yuv_mode, bool bound) {
  const size_t worst = sjpeg_hip_frame_bound(W, H, yuv_mode, 0);
  return bound ? worst : sjpeg_host::FirstCapacity(W, H, yuv_mode, 0, worst);
}

// the counted bits of checked frames, no host wait: ~0 for a frame that did not fit the plan
int counted_bits_launch(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                        const sjpeg_hip_ragged_frame* frames, const std::vector<FrameGeo>& geo,
                        const sjpeg_hip_scan_tables* tables, int tables_per_frame, bool bound, uint64_t* d_bits,
                        hipStream_t st) {
  std::vector<sjpeg_hip_ragged_frame> planned(frames, frames + nframes);
  for (sjpeg_hip_ragged_frame& fr : planned) {
    fr.out_offset = 0;
    fr.out_capacity = count_capacity(fr.width, fr.height, yuv_mode, bound);
  }
  return ragged_encode(e, format, yuv_mode, nframes, planned.data(), geo, tables, tables_per_frame, nullptr, nullptr,
                       0, 0, nullptr, nullptr, st, reinterpret_cast<unsigned long long*>(d_bits));
}

int counted_bits_args(const std::string& who, sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                      const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_scan_tables* tables, int tables_per_frame,
                      const uint64_t* d_bits, std::vector<FrameGeo>* geo) {
  if (int rc = ragged_analysis_args(who, e, format, yuv_mode, nframes, frames, d_bits, geo)) return rc;
  return ragged_tables_ok(who, tables, tables_per_frame ? nframes : 1);
}

}  // namespace

extern "C" {

int sjpeg_hip_scan_histogram_ragged_src(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                        const sjpeg_hip_ragged_frame* frames, uint32_t* d_hist, void* stream) {
  std::vector<FrameGeo> geo;
  if (int rc = ragged_analysis_args("sjpeg_hip_scan_histogram_ragged_src", e, format, yuv_mode, nframes, frames, d_hist, &geo)) return rc;
  try {
    return ragged_analysis(e, kPassHisto, format, yuv_mode, nframes, frames, geo, nullptr, 0, d_hist, static_cast<hipStream_t>(stream));
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

int sjpeg_hip_scan_symbol_stats_ragged_src(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                           const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_scan_tables* tables,
                                           int tables_per_frame, uint32_t* d_freq, void* stream) {
  static const std::string who = "sjpeg_hip_scan_symbol_stats_ragged_src";
  std::vector<FrameGeo> geo;
  if (int rc = ragged_analysis_args(who, e, format, yuv_mode, nframes, frames, d_freq, &geo)) return rc;
  if (int rc = ragged_tables_ok(who, tables, tables_per_frame ? nframes : 1)) return rc;
  try {
    return ragged_analysis(e, kPassStats, format, yuv_mode, nframes, frames, geo, tables, tables_per_frame, d_freq, static_cast<hipStream_t>(stream));
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

int sjpeg_hip_scan_quant_error_ragged_src(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                          const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_scan_tables* tables,
                                          int tables_per_frame, uint64_t* d_err, void* stream) {
  static const std::string who = "sjpeg_hip_scan_quant_error_ragged_src";
  std::vector<FrameGeo> geo;
  if (int rc = ragged_analysis_args(who, e, format, yuv_mode, nframes, frames, d_err, &geo)) return rc;
  if (int rc = ragged_tables_ok(who, tables, tables_per_frame ? nframes : 1)) return rc;
  try {
    return ragged_analysis(e, kPassError, format, yuv_mode, nframes, frames, geo, tables, tables_per_frame,
                           reinterpret_cast<uint32_t*>(d_err), static_cast<hipStream_t>(stream));
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

int sjpeg_hip_scan_counted_bits_ragged_src(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                           const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_scan_tables* tables,
                                           int tables_per_frame, uint64_t* d_bits, void* stream) {
  static const std::string who = "sjpeg_hip_scan_counted_bits_ragged_src";
  std::vector<FrameGeo> geo;
  if (int rc = counted_bits_args(who, e, format, yuv_mode, nframes, frames, tables, tables_per_frame, d_bits, &geo)) {
    return rc;
  }
  try {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = counted_bits_launch(e, format, yuv_mode, nframes, frames, geo, tables, tables_per_frame, false, d_bits, st)) return rc;
    // the frames whose segments overflowed the first plan: counted again, with their worst case, in one more launch
    std::vector<uint64_t> got(nframes);
    HIP_TRY(hipMemcpyAsync(got.data(), d_bits, nframes * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<int> again;
    for (int f = 0; f < nframes; ++f) if (got[f] == ~0ull) again.push_back(f);
    if (again.empty()) return 0;
    if (int rc = sjpeg_internal::counted_bits_recount(e, format, yuv_mode, frames, tables, tables_per_frame, again, d_bits, st)) {
      return rc;
    }
    // (a count is never silently wrong: a frame past even its worst-case plan is an error, as in the host API)
    HIP_TRY(hipMemcpyAsync(got.data(), d_bits, nframes * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int f : again) {
      if (got[f] == ~0ull) return fail(SJPEG_HIP_ERUNTIME, who + ": frame " + std::to_string(f) + ": the count overran its worst-case plan");
    }
    return 0;
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

}  // extern "C"

namespace sjpeg_internal {

int counted_bits_recount(sjpeg_hip_engine* e, int format, int yuv_mode, const sjpeg_hip_ragged_frame* frames,
                         const sjpeg_hip_scan_tables* tables, int tables_per_frame, const std::vector<int>& which,
                         uint64_t* d_bits, hipStream_t st) {
  static const std::string who = "sjpeg_hip_scan_counted_bits_ragged_src";
  const int n = static_cast<int>(which.size());
  std::vector<sjpeg_hip_ragged_frame> sub(n);
  std::vector<sjpeg_hip_scan_tables> subt(tables_per_frame ? n : 1);
  for (int k = 0; k < n; ++k) {
    sub[k] = frames[which[k]];
    if (tables_per_frame) subt[k] = tables[which[k]];
  }
  if (!tables_per_frame) subt[0] = tables[0];
  std::vector<FrameGeo> geo;
  if (int rc = ragged_analysis_args(who, e, format, yuv_mode, n, sub.data(), d_bits, &geo)) return rc;
  if (int rc = e->auto_buf.ensure((static_cast<size_t>(n) * 8 + 15) / 16)) return rc;
  uint64_t* const tmp = reinterpret_cast<uint64_t*>(e->auto_buf.p);
  if (int rc = counted_bits_launch(e, format, yuv_mode, n, sub.data(), geo, subt.data(), tables_per_frame, true, tmp, st)) return rc;
  for (int k = 0; k < n; ++k) {
    HIP_TRY(hipMemcpyAsync(d_bits + which[k], tmp + k, sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  }
  return 0;
}

int counted_bits_first(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes, const sjpeg_hip_ragged_frame* frames,
                       const sjpeg_hip_scan_tables* tables, int tables_per_frame, uint64_t* d_bits, hipStream_t st) {
  static const std::string who = "sjpeg_hip_scan_counted_bits_ragged_src";
  std::vector<FrameGeo> geo;
  if (int rc = counted_bits_args(who, e, format, yuv_mode, nframes, frames, tables, tables_per_frame, d_bits, &geo)) {
    return rc;
  }
  return counted_bits_launch(e, format, yuv_mode, nframes, frames, geo, tables, tables_per_frame, false, d_bits, st);
}

MetaCtx* engine_meta(const sjpeg_hip_engine* e) { return e->meta; }
void engine_set_meta(sjpeg_hip_engine* e, MetaCtx* ctx) { e->meta = ctx; }

bool append_frame_header(int width, int height, int yuv_mode, const uint8_t quant[2][64], const sjpeg_hip_huffman_spec* specs,
                         const FrameMeta* fm, std::vector<uint8_t>* headers) {
  if (width <= 0 || height <= 0 || width > 65535 || height > 65535) return false;
  const sjpeg_host::HuffSpec* dc[2] = {&sjpeg_host::DefaultHuff(0, 0), &sjpeg_host::DefaultHuff(0, 1)};
  const sjpeg_host::HuffSpec* ac[2] = {&sjpeg_host::DefaultHuff(1, 0), &sjpeg_host::DefaultHuff(1, 1)};
  if (specs != nullptr) {
    const int ntables = (yuv_mode == SJPEG_HIP_YUV400) ? 1 : 2;
    for (int t = 0; t < ntables; ++t) { dc[t] = &specs[t]; ac[t] = &specs[2 + t]; }
  }
  return sjpeg_host::AppendHeadersBlock(width, height, yuv_mode, quant, dc, ac, fm != nullptr ? fm->block.data() : nullptr,
                                        fm != nullptr ? fm->block.size() : 0, headers);
}

int ragged_check(const std::string& who, int format, int yuv_mode, int nframes, const sjpeg_hip_ragged_frame* frames, int esz) {
  std::vector<FrameGeo> geo;
  if (int rc = ragged_format(who, format, yuv_mode)) return rc;
  return ragged_frames(who, format, yuv_mode, nframes, frames, true, &geo, esz);
}
size_t engine_scratch_limit(const sjpeg_hip_engine* e) { return e->scratch_limit; }
int engine_device(const sjpeg_hip_engine* e) { return e->device; }

int engine_search_sizes(sjpeg_hip_engine* e, size_t n, uint64_t** d_sizes) {
  if (int rc = e->search_sizes.ensure(n)) return rc;
  *d_sizes = e->search_sizes.p;
  return 0;
}

uint64_t* engine_full_stats(sjpeg_hip_engine* e) { return e->full_stats; }

int engine_kept_blocks(sjpeg_hip_engine* e, size_t segs) {
  if (int rc = e->replay.ensure(segs * kKeptSegWords)) return rc;
  e->replay_w = e->replay_h = e->replay_mode = e->replay_nframes = 0;      // (no uniform call's kept blocks any more)
  return 0;
}

int engine_arena(sjpeg_hip_engine* e, size_t bytes, uint8_t** p) {
  if (int rc = e->sharp_arena.ensure(bytes / 16 + 1)) return rc;
  *p = reinterpret_cast<uint8_t*>(e->sharp_arena.p);
  return 0;
}

int trellis_stats_ragged(sjpeg_hip_engine* e, const std::string& who, int format, int yuv_mode, int nframes,
                         const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_scan_tables* tables, const uint32_t* kept_base,
                         uint32_t* d_freq, hipStream_t st) {
  std::vector<FrameGeo> geo;
  if (int rc = ragged_analysis_args(who, e, format, yuv_mode, nframes, frames, d_freq, &geo)) return rc;
  for (int f = 0; f < nframes; ++f) {                // (the kept blocks of every frame lie inside the engine's buffer)
    if ((static_cast<size_t>(kept_base[f]) + geo[f].nseg) * kKeptSegWords > e->replay.cap) return fail(SJPEG_HIP_EINVAL, who + ": internal: kept base past the kept blocks");
  }
  return ragged_analysis(e, kPassStatsTrellis, format, yuv_mode, nframes, frames, geo, tables, 1, d_freq, st, e->replay.p, kept_base);
}

int replay_encode_ragged(sjpeg_hip_engine* e, const std::string& who, int format, int yuv_mode, int nframes,
                         const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_scan_tables* tables, const uint32_t* kept_base,
                         const void* headers, const size_t* header_offsets, void* d_out, uint64_t* d_sizes, hipStream_t st,
                         const PackedSink* sink) {
  std::vector<FrameGeo> geo;
  if (int rc = ragged_format(who, format, yuv_mode)) return rc;
  if (int rc = ragged_frames(who, format, yuv_mode, nframes, frames, true, &geo)) return rc;
  for (int f = 0; f < nframes; ++f) {
    if ((static_cast<size_t>(kept_base[f]) + geo[f].nseg) * kKeptSegWords > e->replay.cap) return fail(SJPEG_HIP_EINVAL, who + ": internal: kept base past the kept blocks");
  }
  return ragged_encode(e, format, yuv_mode, nframes, frames, geo, tables, 1, headers, header_offsets, header_offsets[nframes],
                       /*append_eoi=*/1, d_out, d_sizes, st, nullptr, e->replay.p, sink, kept_base);
}

// adapt_sums_kernel / adapt_decide_kernel over n consecutive frames, each from its own starting matrices
int adapt_ragged(const uint32_t* d_hist, const uint8_t* d_quant_in, int n, const uint8_t* min_quant, int ntab,
                 int qdelta_max_luma, int qdelta_max_chroma, int64_t* d_sums, int32_t* d_totlast, uint8_t* d_quant_out,
                 hipStream_t st) {
  AdaptArgs s;
  s.hist = d_hist;
  s.sums = reinterpret_cast<long long*>(d_sums);
  s.totlast = d_totlast;
  memset(s.quant, 0, sizeof(s.quant));
  if (min_quant != nullptr) memcpy(s.min_quant, min_quant, sizeof(s.min_quant)); else memset(s.min_quant, 1, sizeof(s.min_quant));
  s.quant_f = d_quant_in;
  hipLaunchKernelGGL(adapt_sums_kernel<true>, dim3(64, 2, n), dim3(64), 0, st, s);
  HIP_TRY(hipGetLastError());
  DecideArgs d;
  d.sums = s.sums; d.totlast = s.totlast;
  d.quant_out = d_quant_out;
  memset(d.quant_in, 0, sizeof(d.quant_in));
  d.last_step[0] = qdelta_max_luma + 12;
  d.last_step[1] = qdelta_max_chroma + 12;
  d.quant_f = d_quant_in;
  hipLaunchKernelGGL(adapt_decide_kernel<true>, dim3(ntab, n), dim3(64), 0, st, d);
  HIP_TRY(hipGetLastError());
  return 0;
}

// adapt_decide_kernel behind sjpeg_hip_adapt_sums on the same stream: d_quant_out[nframes][2][64]
int adapt_decide(const int64_t* d_sums, const int32_t* d_totlast, int nframes, const uint8_t quant[2][64], int ntables,
                 int qdelta_max_luma, int qdelta_max_chroma, uint8_t* d_quant_out, hipStream_t st) {
  DecideArgs a;
  a.quant_f = nullptr;
  a.sums = reinterpret_cast<const long long*>(d_sums);
  a.totlast = d_totlast;
  a.quant_out = d_quant_out;
  memcpy(a.quant_in, quant, sizeof(a.quant_in));
  a.last_step[0] = qdelta_max_luma + 12;
  a.last_step[1] = qdelta_max_chroma + 12;
  hipLaunchKernelGGL(adapt_decide_kernel<>, dim3(ntables, nframes), dim3(64), 0, st, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace sjpeg_internal

extern "C" {
namespace {
__global__ __launch_bounds__(256) void scatter_sizes_kernel(const unsigned long long* sizes, const uint32_t* index, int n,
                                                            unsigned long long* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[index[i]] = sizes[i];
}
// (a frame's share of the flows' scratch -- ragged_aux.h -- against what the kernels leave)
static_assert(kKeptSegBytes == kKeptSegWords * sizeof(uint32_t), "a segment's kept blocks");
static_assert(kHistPartial == kHistoPartialWords * sizeof(uint32_t) && kStatsPartial == kStatsWords * sizeof(uint32_t), "a workgroup's partials");
}  // namespace
}  // extern "C"

int sjpeg_internal::scatter_sizes(const unsigned long long* d_sizes, const uint32_t* d_index, int n, unsigned long long* d_out, hipStream_t st) {
  hipLaunchKernelGGL(scatter_sizes_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, st, d_sizes, d_index, n, d_out);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" {

// ---- one frame over several GPUs: bands of consecutive segments ----------

int sjpeg_hip_segment_count(int width, int height, int yuv_mode) {
  FrameGeo g;
  if (!frame_geo(width, height, yuv_mode, &g)) return fail(SJPEG_HIP_EINVAL, "bad geometry / yuv_mode");
  return g.nseg;
}

int sjpeg_hip_restart_interval(int yuv_mode) {
  switch (yuv_mode) {
    case SJPEG_HIP_YUV420: return Geo<SJPEG_HIP_YUV420>::kSegMcus;
    case SJPEG_HIP_YUV444: return Geo<SJPEG_HIP_YUV444>::kSegMcus;
    case SJPEG_HIP_YUV400: return Geo<SJPEG_HIP_YUV400>::kSegMcus;
    default: return 0;
  }
}

size_t sjpeg_hip_header_add_restart(uint8_t* header, size_t size, size_t cap, int yuv_mode) {
  const int ri = sjpeg_hip_restart_interval(yuv_mode);
  if (header == nullptr || ri == 0 || size < 4 || cap < size + 6) return 0;
  size_t sos = size;                               // the SOS segment: the last FF DA of the header
  while (sos >= 2 && !(header[sos - 2] == 0xff && header[sos - 1] == 0xda)) --sos;
  if (sos < 2) return 0;
  sos -= 2;
  memmove(header + sos + 6, header + sos, size - sos);
  const uint8_t dri[6] = {0xff, 0xdd, 0x00, 0x04, static_cast<uint8_t>(ri >> 8), static_cast<uint8_t>(ri)};
  memcpy(header + sos, dri, 6);
  return size + 6;
}

size_t sjpeg_hip_band_bound(int width, int height, int yuv_mode, int seg_begin, int seg_end) {
  FrameGeo g;
  if (!frame_geo(width, height, yuv_mode, &g)) return 0;
  if (seg_begin < 0 || seg_end > g.nseg || seg_begin >= seg_end) return 0;
  return (static_cast<size_t>(seg_end - seg_begin) * g.slot_words + kChunkWords + 3) & ~size_t(3);
}

int sjpeg_hip_encode_band_src(sjpeg_hip_engine* e, const sjpeg_hip_source* src, int width, int height,
                              int yuv_mode, const sjpeg_hip_scan_tables* tables, int seg_begin,
                              int seg_end, uint32_t* d_words, size_t cap_words, uint64_t* d_nbits,
                              void* stream) {
  if (d_words == nullptr || d_nbits == nullptr) return fail(SJPEG_HIP_EINVAL, "d_words/d_nbits == NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  FrameGeo g;
  ScanArgs a;
  int cls = 0;
  SegPlan plan;
  int rc = prepare_scan(e, src, width, height, yuv_mode, 1, tables, st, &g, &a, &cls, false, false, SIZE_MAX, &plan);
  if (rc) return rc;
  if (seg_begin < 0 || seg_end > g.nseg || seg_begin >= seg_end) return fail(SJPEG_HIP_EINVAL, "bad segment range");
  a.rst = 0;                                       // (bands are stitched at bit granularity: the exact mode)
  HIP_TRY(hipMemsetAsync(a.pool_ctr, 0, 2 * sizeof(uint32_t), st));
  e->ctr_clean_at[0] = nullptr;                    // (no K4 in this path)
  const int nloc = seg_end - seg_begin;
  const size_t need = sjpeg_hip_band_bound(width, height, yuv_mode, seg_begin, seg_end);
  if (cap_words < need) {
    return fail(SJPEG_HIP_ECAPACITY, "band buffer of " + std::to_string(cap_words) + " words, need " + std::to_string(need));
  }
  a.nseg = nloc;
  a.seg_first = seg_begin;
  const uint32_t max_chunks = static_cast<uint32_t>((cap_words + kChunkWords - 1) / kChunkWords);
  if ((rc = e->seg_off.ensure(static_cast<size_t>(nloc) + 1))) return rc;
  if ((rc = e->chunk_ff.ensure(max_chunks))) return rc;
  StitchArgs s;
  memset(&s, 0, sizeof(s));
  s.nseg = nloc; s.nframes = 1;
  s.seg_nbits = e->seg_nbits.p; s.seg_off = e->seg_off.p;
  s.seg_words = e->seg_words.p; s.slot_words = plan.slot_words;
  s.pool = a.pool; s.pool_words = plan.pool_words; s.seg_xbase = a.seg_xbase; s.pool_ctr = a.pool_ctr;
  s.ubuf = d_words; s.ubuf_words = cap_words;
  s.chunk_ff = e->chunk_ff.p; s.max_chunks = max_chunks;
  s.total_bits_out = reinterpret_cast<unsigned long long*>(d_nbits);
  s.subs = 1;
  if (tables->flags & SJPEG_HIP_QUANT_TRELLIS) rc = launch_scan<kKindEncodeTrellis>(yuv_mode, cls, dim3(nloc, 1), st, a);
  else rc = launch_scan<kKindEncode>(yuv_mode, cls, dim3(nloc, 1), st, a);
  if (rc) return rc;
  hipLaunchKernelGGL(scan_seg_offsets<>, dim3(1), dim3(kThreads), 0, st, s);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(place_segments<false>, dim3((nloc + 3) / 4, 1), dim3(kThreads), 0, st, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

int sjpeg_hip_stitch_bands(sjpeg_hip_engine* e, int nbands, const uint32_t* d_words,
                           size_t band_stride_words, const uint64_t* d_nbits, const void* header,
                           size_t header_size, int append_eoi, void* d_out, size_t out_cap,
                           uint64_t* d_size, void* stream) {
  if (e == nullptr || d_words == nullptr || d_nbits == nullptr || d_out == nullptr || d_size == nullptr) {
    return fail(SJPEG_HIP_EINVAL, "null argument");
  }
  if (nbands <= 0 || nbands > 65535) return fail(SJPEG_HIP_EINVAL, "nbands out of range");
  if (band_stride_words < 4 || band_stride_words >= (size_t(1) << 27)) {
    return fail(SJPEG_HIP_EINVAL, "band_stride_words out of range (a band is shorter than 2^32 bits)");
  }
  if (header == nullptr) header_size = 0;
  if (out_cap < header_size + 2 + 64) return fail(SJPEG_HIP_ECAPACITY, "out_cap too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(e->device));
  if (int rc0 = order_on_stream(e, st)) return rc0;
  int rc;
  const size_t ubuf_words = (static_cast<size_t>(nbands) * band_stride_words + kChunkWords + 3) & ~size_t(3);
  const uint32_t max_chunks = static_cast<uint32_t>((ubuf_words + kChunkWords - 1) / kChunkWords);
  if ((rc = e->seg_off.ensure(static_cast<size_t>(nbands) + 1))) return rc;
  if ((rc = e->ubuf.ensure(ubuf_words))) return rc;
  if ((rc = e->chunk_ff.ensure(max_chunks))) return rc;
  if ((rc = e->chunk_off.ensure(max_chunks))) return rc;
  if ((rc = e->header.ensure(header_size > 0 ? header_size : 1))) return rc;
  e->header_held_at = nullptr;                     // (this path does not track what it uploads)
  if (header_size > 0) { if (int rcu = upload(e, e->header.p, header, header_size, st)) return rcu; }
  StitchArgs s;
  memset(&s, 0, sizeof(s));
  s.nseg = nbands; s.nframes = 1;
  s.seg_nbits64 = reinterpret_cast<const unsigned long long*>(d_nbits);
  s.seg_off = e->seg_off.p;
  s.seg_words = d_words; s.slot_words = static_cast<uint32_t>(band_stride_words);
  s.ubuf = e->ubuf.p; s.ubuf_words = ubuf_words;
  s.chunk_ff = e->chunk_ff.p; s.chunk_off = e->chunk_off.p; s.max_chunks = max_chunks;
  s.header = e->header.p; s.header_size = static_cast<uint32_t>(header_size);
  s.append_eoi = append_eoi;
  s.out = static_cast<uint8_t*>(d_out); s.out_stride = out_cap;
  s.sizes = reinterpret_cast<unsigned long long*>(d_size);
  const uint32_t per_wave = kSpec * kPlaceLanes;
  s.subs = static_cast<uint32_t>((band_stride_words + per_wave - 1) / per_wave);
  e->last_nseg = nbands; e->last_nframes = 1;
  hipLaunchKernelGGL(scan_seg_offsets<>, dim3(1), dim3(kThreads), 0, st, s);
  HIP_TRY(hipGetLastError());
  const uint32_t units = static_cast<uint32_t>(nbands) * s.subs;
  hipLaunchKernelGGL(place_segments<false>, dim3((units + 3) / 4, 1), dim3(kThreads), 0, st, s);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(scan_chunk_offsets<>, dim3(1), dim3(kThreads), 0, st, s);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(stuff_chunks_wave, dim3((max_chunks + 3u) / 4u, 1), dim3(kThreads), 0, st, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

int sjpeg_hip_adapt_decide(const int64_t* d_sums, const int32_t* d_totlast, int nframes, const uint8_t quant[2][64],
                           int yuv_mode, int qdelta_max_luma, int qdelta_max_chroma, uint8_t* d_quant_out, void* stream) {
  if (d_sums == nullptr || d_totlast == nullptr || quant == nullptr || d_quant_out == nullptr || nframes <= 0 || nframes > 65535) {
    return fail(SJPEG_HIP_EINVAL, "null argument or bad nframes");
  }
  if (qdelta_max_luma < -12 || qdelta_max_luma > 12 || qdelta_max_chroma < -12 || qdelta_max_chroma > 12) {
    return fail(SJPEG_HIP_EINVAL, "qdelta_max outside -12 .. 12");
  }
  return adapt_decide(d_sums, d_totlast, nframes, quant, yuv_mode == SJPEG_HIP_YUV400 ? 1 : 2, qdelta_max_luma, qdelta_max_chroma,
                      d_quant_out, static_cast<hipStream_t>(stream));
}

int sjpeg_hip_adapt_sums(const uint32_t* d_hist, int nframes, const uint8_t quant[2][64],
                         const uint8_t* min_quant, int64_t* d_sums, int32_t* d_totlast, void* stream) {
  if (d_hist == nullptr || quant == nullptr || d_sums == nullptr || d_totlast == nullptr || nframes <= 0 || nframes > 65535) {
    return fail(SJPEG_HIP_EINVAL, "null argument or bad nframes");
  }
  AdaptArgs a;
  a.quant_f = nullptr;
  a.hist = d_hist;
  a.sums = reinterpret_cast<long long*>(d_sums);
  a.totlast = d_totlast;
  memcpy(a.quant, quant, sizeof(a.quant));
  if (min_quant != nullptr) memcpy(a.min_quant, min_quant, sizeof(a.min_quant)); else memset(a.min_quant, 1, sizeof(a.min_quant));
  hipLaunchKernelGGL(adapt_sums_kernel<>, dim3(64, 2, nframes), dim3(64), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
