// scan_engine.hip -- the MI355X (gfx950 / CDNA4) scan engine behind include/sjpeg_hip.h.
//
// Replaces the reference's per-MCU hot loop (Encoder::SinglePassScan,
// /root/reference/src/enc.cc:276-307) for whole frames / batches of frames resident in HBM.
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
//
// The reference never emits restart markers, so bit-exactness needs exactly this
// bit-level stitching.
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
#include "ragged_aux.h"

using namespace sjpeg_internal;      // (the shared sizes, SjpegYUVMode and the mode groups)

namespace {

#include "scan_device.h"
#include "scan_segments.h"
#include "scan_reduce.h"
#include "stitch_kernels.h"

// ------------------------------------------------------------------------------------
// host side

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    const hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess) {                                                             \
      return fail(e_ == hipErrorOutOfMemory ? SJPEG_HIP_ENOMEM : SJPEG_HIP_ERUNTIME,    \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                   \
    }                                                                                   \
  } while (0)

struct FrameGeo {
  int bpm, px, seg_mcus, mb_w, mb_h, n_mcus, nseg;
  uint32_t slot_words;
};

bool frame_geo(int W, int H, int mode, FrameGeo* g) {
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

// measurement aid (SJPEG_HIP_BATCH_DEBUG=1): microseconds since this thread's previous mark, on stderr -- which runtime
// call of a launch sequence the host spent its time in (tools/slow_call_timeline.py)
inline void dbg_mark(const char* what) {
  static const int level = getenv("SJPEG_HIP_BATCH_DEBUG") != nullptr ? atoi(getenv("SJPEG_HIP_BATCH_DEBUG")) : 0;
  if (level < 2) return;
  static thread_local std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  const auto now = std::chrono::steady_clock::now();
  const double us = std::chrono::duration<double, std::micro>(now - last).count();
  if (us > (level >= 3 ? 6.0 : 200.0)) fprintf(stderr, "    step %-28s %9.1f us\n", what, us);   // (3: every step over 6 us)
  last = now;
}

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;     // elements
  int ensure(size_t n) {
    if (n <= cap) return 0;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
    if (e != hipSuccess) {
      return fail(SJPEG_HIP_ENOMEM, std::string("hipMalloc(") + std::to_string(n * sizeof(T)) +
                                        "): " + hipGetErrorString(e));
    }
    cap = n;
    return 0;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

}  // namespace

struct sjpeg_hip_engine {
  int device = 0;
  int cu_count = 256;                  // compute units of the device (the persistent histogram kind sizes its grid by it)
  int histo_slots = 0;                 // SJPEG_HIP_HISTO_SLOTS, read when the engine is made: workgroups of a histogram launch (tests: many trips)
  DevBuf<DevTables> tables;
  DevBuf<uint8_t> header;
  // what the two buffers hold, and the stream that put it there: a call with the same tables /
  // header on the same stream skips the upload (two of the ~6 runtime calls of a small encode)
  std::vector<DevTables> tables_held;
  // Host-to-device uploads of more than a few KB (the tables and headers of a batch) go through pinned blocks the
  // engine owns: hipMemcpyAsync from pageable memory pins the caller's pages for the length of the copy -- tens of
  // microseconds of host time per upload and, now and then, several milliseconds (seen as one call in twenty of a
  // 32-frame default-parameter batch taking 8 ms instead of 1.6).
  struct Stage { void* p = nullptr; void* dp = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool busy = false; } stage[4];
  int stage_next = 0;
  std::vector<uint8_t> header_held;
  const void* tables_held_at = nullptr; const void* header_held_at = nullptr;
  hipStream_t tables_stream = nullptr, header_stream = nullptr;
  DevBuf<uint32_t> seg_words, seg_nbits, pool, pool_ctr, seg_xbase, ubuf, chunk_ff, partial, replay;
  DevBuf<uint32_t> frame_flags;        // K2's copy of every frame's "overran its pool" flag (stitch_kernels.h)
  int replay_w = 0, replay_h = 0, replay_mode = 0, replay_nframes = 0;   // what `replay` holds (0 = nothing)
  // A batch coded in parts (sjpeg_hip_encode_batch_src): the statistics / replay calls of a part address the
  // kept blocks of frames [replay_first, replay_first + nframes) of a buffer for replay_total frames.
  int replay_first = 0, replay_total = 0;
  // ... and when the call runs a histogram pass in front of its statistics pass (the adaptive methods with
  // optimized Huffman tables), the histogram pass leaves every block's DCT coefficients in `replay` and the
  // statistics pass starts from them (kKindStatsCoef): set by sjpeg_hip_encode_batch_src for the length of the call
  bool coefs_keep = false, coefs_use = false;
  // ... and their per-workgroup partial statistics likewise live in a buffer for replay_total frames, summed on
  // `reduce_stream` (behind an event) instead of the call's stream: the sums of one part run under the device
  // pass of the next
  hipStream_t reduce_stream = nullptr;
  hipEvent_t reduce_ev = nullptr;
  // ... and its uploads (a part's tables, headers, header offsets) leave EARLY, on `up_stream`, the moment the host has
  // them -- the call's stream only waits for the event behind the last one (sync_uploads) in front of the kernel that
  // reads them.  In the call's own stream every upload was a copy kernel between two dependent launches plus the marker
  // of its pinned block: ~80 us of an idle device per 32-frame call (rocprofv3 trace, round 5).  What makes it safe:
  // the parts' tables / headers lie side by side (part_first_frame()), and the host only has a part's data once the pass
  // in front -- hence everything older on the call's stream -- is done (the sums / counts it waited for say so).
  hipStream_t up_stream = nullptr;
  hipEvent_t up_wait = nullptr;          // the event behind the last early upload nobody waited for yet (one of stage[].ev)
  // The two streams of a batch in parts, made WITH the engine: a stream made late in the life of a process -- behind
  // the first asynchronous copy, it seems; bench.py's batch lines came a minute in -- shares the hardware queue of
  // an older one, the caller's as it turned out: the side stream's sums then queue behind the next part's pass, the
  // early uploads behind the kernel they should run under, and the call takes what it takes with everything in one
  // stream (1.33 ms against 1.19 for 32 4K frames; not the number of hardware queues -- GPU_MAX_HW_QUEUES 8 / 16 the
  // same --, not their priority -- the greatest made it 1.46).  Streams made when the engine is, early, keep queues of
  // their own (bisected in bench.py, round 5; profiles/HISTORY.md).
  hipStream_t batch_side = nullptr, batch_up = nullptr;
  // LANES of the batch path (round 6): a large default-parameter batch is cut into jobs of about eight 4K frames, every
  // job a complete histogram -> statistics -> encode sequence of its own, and the jobs run on up to four streams at once
  // -- lane 0 is this engine on the caller's stream, lanes 1..3 are child engines (their own scratch) on streams the
  // engine owns (batch_side and batch_up, made WITH the engine, see above; the fourth on demand: two lanes are the default).  The three passes have different
  // bottlenecks -- the histogram kind is latency-bound with the VALU 60 % busy, the statistics kind is the memory's, the
  // replay kind the VALU's --: side by side they fill each other's gaps, one after the other (the two parts of round 5)
  // they cannot.  Measured with independent calls from several host threads first (tools/two_stream_batch.py).
  static constexpr int kLanes = 4;
  sjpeg_hip_engine* lane[kLanes] = {nullptr, nullptr, nullptr, nullptr};   // [0] unused (this engine)
  hipStream_t batch_lane3 = nullptr;
  hipEvent_t lane_in = nullptr, lane_done[kLanes] = {nullptr, nullptr, nullptr, nullptr};
  bool is_lane = false;                // a child engine: no streams or lanes of its own
  // the pixel transform of the float source formats (sjpeg_hip_engine_set_pixel_transform): byte = fmaf(x, scale, bias),
  // rounded to even and saturated; sticky, read by no other format; the lanes take the parent's with every call
  float pscale[3] = {255.0f, 255.0f, 255.0f}, pbias[3] = {0.0f, 0.0f, 0.0f};
  DevBuf<unsigned long long> seg_off, chunk_off, stamps;
  DevBuf<uint32_t> hdr_off;
  bool want_stamps = false;
  int stamp_mode = 0;              // SJPEG_HIP_STAMPS, parsed ONCE when the engine is made (1 cycle counter, 2 device clock, 3 + segment bits)
  int last_nseg = 0, last_nframes = 0;   // geometry of the last encode call (entropy_bits)
  size_t stamps_n = 0;
  bool timing = false;
  int ablate = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ev_valid = false;
  // Pipelined mode (sjpeg_hip_engine_set_pipelined): K1 on the caller's stream, K2..K5 on the
  // engine's own stream, two sets of segment buffers -- the stitch of call i (HBM-bound, little
  // ALU) runs under the K1 of call i + 1 (ALU-bound, little HBM).
  // the scratch buffers are shared by all calls: a call on another stream than the previous one
  // waits for that one's work first
  hipStream_t last_stream = nullptr;
  bool last_stream_valid = false;
  hipEvent_t cross_ev = nullptr;
  bool pipelined = false;
  size_t scratch_limit = static_cast<size_t>(16) << 30;   // segment scratch of ONE launch (SJPEG_HIP_SCRATCH_LIMIT_BYTES): larger batches go in several
  hipStream_t side = nullptr;
  DevBuf<uint32_t> seg_words2, seg_nbits2, pool2, pool_ctr2, seg_xbase2;
  // K4 leaves the pool counters of the frames it saw at zero, so an encode call only clears them
  // itself when the previous user of the set did not get that far (or was larger / another buffer)
  const void* ctr_clean_at[2] = {nullptr, nullptr};
  size_t ctr_clean_n[2] = {0, 0};
  int set = 0;                                   // buffer set of the NEXT call
  hipEvent_t k1_done = nullptr, side_done = nullptr, k3_done[2] = {nullptr, nullptr};
  bool k3_pending[2] = {false, false}, side_pending = false;
  // ragged batches (sjpeg_hip_encode_ragged_src): the call's frame descriptors, tables, workgroup -> frame maps, header
  // offsets and header bytes, uploaded as one blob -- buffers of its own, so that nothing the uniform calls hold or
  // upload on the stitch stream is touched
  DevBuf<uint4> ragged;
  // ... but the header bytes: a frame with metadata has a header of up to megabytes, so the headers of ONE launch at a
  // time are staged here (counted against the scratch limit; below 4 GiB: the kernels address them with 32-bit offsets)
  DevBuf<uint4> hdr_stage;
  // the metadata of the ragged call the engine is running (ragged_aux.h; NULL: none)
  sjpeg_internal::MetaCtx* meta = nullptr;
  // ragged calls with SJPEG_YUV_AUTO / SJPEG_YUV_SHARP (sjpeg_hip_encode_ragged_auto_src): the riskiness table of this
  // device (uploaded again when sjpeg_hip_set_riskiness_table changes it), the riskiness descriptors and sums, the sizes
  // of the mode groups before they go back to the caller's order, and the sharp frames' planes and workspace
  DevBuf<uint8_t> risk_table;
  int risk_generation = -1;
  DevBuf<uint4> auto_buf;
  DevBuf<uint4> sharp_arena;
  // reduced or resized pictures (sjpeg_hip_encode_ragged_reduced_src, _resized_src): the uint8 pictures the reduce or the
  // resize kernel makes for the inner encode, ONE allocation of their own -- not the arena above, which the inner flow lays its sharp planes and kept
  // blocks out in --, and the kernel's frame descriptors.  A later call writes them behind everything the earlier one
  // queued: the engine's ordering, as for every scratch buffer.
  DevBuf<uint4> reduced, reduce_desc;
  // ... and the descriptors of the colour launch that may follow the resize launch of the same call (yuv_colour.hip): a
  // buffer of their own, so that their upload never lands on descriptors the resize kernel is still to read
  DevBuf<uint4> colour_desc;
  // the batch search (sjpeg_hip_encode_ragged_search_src): the sizes of its sub-calls on their way to the caller's
  // order -- the engine's, as everything a call leaves queued on its stream
  DevBuf<uint64_t> search_sizes;
  // packed output of a ragged call (sjpeg_hip_encode_ragged_packed_src): where the next frame starts -- zeroed once by
  // the call, advanced by place_ragged_frames of every launch, group and part of it (bit 63: a frame was dropped)
  DevBuf<unsigned long long> pack_cursor;
  // what the most recent sjpeg_hip_encode_ragged_full_*_src call cost (sjpeg_hip_engine_search_stats): host values
  uint64_t full_stats[6] = {0, 0, 0, 0, 0, 0};
  // side_done is recorded LAZILY, by whoever is about to wait on it (side_mark): an event record is a packet in the
  // queue and about 5 us of host time, and a loop of pipelined calls needs none -- one frame per call was bound by the
  // HOST at five event calls per call (36-46 us against 35 of device time, `tools/one_frame_piped.py`)
  bool side_recorded = false;
};

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

// the event behind everything the engine has put on its own (stitch) stream so far
int side_mark(sjpeg_hip_engine* e) {
  if (e->side_pending && !e->side_recorded) {
    HIP_TRY(hipEventRecord(e->side_done, e->side));
    e->side_recorded = true;
  }
  return 0;
}

// Orders this call after everything the engine was asked to do on another stream.
int order_on_stream(sjpeg_hip_engine* e, hipStream_t st) {
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

// bytes between two places the DEVICE can address (device memory, mapped pinned host memory), by that kernel; the
// runtime's copy where the addresses do not allow 16-byte accesses
int copy_by_kernel(void* dst, const void* src, size_t bytes, hipStream_t st, hipMemcpyKind fallback_kind, const void* fallback_src, void* fallback_dst) {
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
int upload(sjpeg_hip_engine* e, void* dst, const void* src, size_t bytes, hipStream_t st) {
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
int sync_uploads(sjpeg_hip_engine* e, hipStream_t st) {
  if (e->up_wait != nullptr) {
    HIP_TRY(hipStreamWaitEvent(st, e->up_wait, 0));
    e->up_wait = nullptr;
  }
  return 0;
}

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
  e->reduced.release(); e->reduce_desc.release(); e->colour_desc.release();
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
  e->reduced.release(); e->reduce_desc.release(); e->colour_desc.release();
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
         b(e->risk_table) + b(e->auto_buf) + b(e->sharp_arena) + b(e->search_sizes) + b(e->pack_cursor) + b(e->reduced) + b(e->reduce_desc) + b(e->colour_desc);
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
  else hipLaunchKernelGGL(stuff_chunks<0>, dim3(gx, nframes), dim3(kThreads), 0, hs, s);
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
int ragged_format(const std::string& who, int format, int yuv_mode, ScanArgs* a, int* cls, const SourceLayout** layout) {
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

// Every frame of a ragged call of a known format checked (the message names the frame); its geometry into (*geo)[f].
// out_ranges: the frames' output ranges are checked too (the encodes; the analysis passes ignore them).
int ragged_frames(const std::string& who, int format, int yuv_mode, int nframes,
                  const sjpeg_hip_ragged_frame* frames, bool out_ranges, std::vector<FrameGeo>* geo, int esz = 0) {
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

// a frame's planes (the kernels' three out of the caller's: layout_planes) and geometry in its descriptor
void ragged_geometry(const SourceLayout& L, const sjpeg_hip_ragged_frame& fr, const FrameGeo& g, RaggedFrame* d) {
  layout_planes(L, fr.plane, fr.row_stride, nullptr, d->plane, d->row_stride, nullptr);
  d->W = fr.width; d->H = fr.height; d->mb_w = g.mb_w; d->n_mcus = g.n_mcus; d->nseg = g.nseg;
  d->has_clip = (fr.width % g.px != 0) || (fr.height % g.px != 0);
}

int ragged_encode(sjpeg_hip_engine* e, int yuv_mode, int cls, ScanArgs a, const SourceLayout* layout, int nframes,
                  const sjpeg_hip_ragged_frame* frames, const std::vector<FrameGeo>& geo,
                  const sjpeg_hip_scan_tables* tables, int tables_per_frame, const void* headers,
                  const size_t* header_offsets, size_t header_size, int append_eoi, void* d_out, uint64_t* d_sizes,
                  hipStream_t st, unsigned long long* d_bits, uint32_t* kept = nullptr,
                  const sjpeg_internal::PackedSink* sink = nullptr, const uint32_t* kept_base = nullptr);

}  // namespace

int sjpeg_hip_encode_ragged_src(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
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
  // the layout of the format (as prepare_scan): planes, source class, the kernel's per-format fields
  ScanArgs a;
  int cls = kSrcPlanes;
  const SourceLayout* layout = nullptr;
  if (int rcf = ragged_format(kWhoEncode, format, yuv_mode, &a, &cls, &layout)) return rcf;
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
    return ragged_encode(e, yuv_mode, cls, a, layout, nframes, frames, geo, tables, tables_per_frame, headers, header_offsets,
                         header_size, append_eoi, d_out, d_sizes, static_cast<hipStream_t>(stream), nullptr);
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

namespace {

// The ragged encode of checked frames (ragged_frames, ragged_format): K1 kKindEncodeRagged, K2 .. K5.  d_bits != NULL:
// a count without output (sjpeg_hip_scan_counted_bits_ragged_src) -- K1 .. K3, then counted_bits_ragged instead of
// K4 and K5, no header, nothing written to d_out or d_sizes; the frames' out_capacity plans the segment scratch only.
// kept != NULL: K1 is kKindEncodeReplayRagged -- it codes the blocks a trellis statistics pass left at `kept` and reads no
// pixel; frame f's lie kept_base[f] segments behind `kept`, kKeptSegWords a segment (ragged_analysis, kPassStatsTrellis:
// the same table, so a frame's blocks have one place whichever frames a launch covers).
// sink != NULL: packed output -- d_out and the frames' out_offset are not used; per launch K4 leaves the sizes only,
// place_ragged_frames puts the launch's frames behind the engine's cursor (each start into its descriptor, where K5
// takes it from, and into the caller's offsets), pack_ragged_edges writes header, EOI and padding (stitch_kernels.h).
int ragged_encode(sjpeg_hip_engine* e, int yuv_mode, int cls, ScanArgs a, const SourceLayout* layout, int nframes,
                  const sjpeg_hip_ragged_frame* frames, const std::vector<FrameGeo>& geo,
                  const sjpeg_hip_scan_tables* tables, int tables_per_frame, const void* headers,
                  const size_t* header_offsets, size_t header_size, int append_eoi, void* d_out, uint64_t* d_sizes,
                  hipStream_t st, unsigned long long* d_bits, uint32_t* kept, const sjpeg_internal::PackedSink* sink,
                  const uint32_t* kept_base) {
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
  HIP_TRY(hipSetDevice(e->device));
  if (int rc0 = order_on_stream(e, st)) return rc0;
  if (e->side_pending) {                             // (pipelined mode: the call runs ordered, behind the engine's stitch)
    if (int rcm = side_mark(e)) return rcm;
    HIP_TRY(hipStreamWaitEvent(st, e->side_done, 0));
  }
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

enum RaggedPass { kPassHisto, kPassStats, kPassError, kPassStatsTrellis };

// The analysis passes over a ragged batch: the histogram (kKindHistoRagged, persistent groups), the symbol statistics
// (kKindStatsRagged, a workgroup per segment) or the quantization error (kKindErrorRagged, a workgroup per segment) of
// frames [0, nframes), then their ragged reduce -- d_out[f] = [2][64][128] or [2][272] words, or one 64-bit total: what
// the uniform pass makes of frame f alone.  The frames have been checked (ragged_frames); `a` holds the format's fields
// (ragged_format).  The partials of a launch stay inside the engine's scratch limit: a larger batch goes in several
// launches over consecutive frames.  kPassStatsTrellis: the statistics with trellis quantization (kKindStatsTrellisRagged;
// tables with SJPEG_HIP_QUANT_TRELLIS); its quantized blocks stay behind at `kept`, frame f's kept_base[f] segments in
// (kKeptSegWords a segment), whatever the launches and whichever frames the call covers -- for ragged_encode to replay.
int ragged_analysis(sjpeg_hip_engine* e, RaggedPass pass, int yuv_mode, int cls, ScanArgs a, const SourceLayout* layout, int nframes,
                    const sjpeg_hip_ragged_frame* frames, const std::vector<FrameGeo>& geo,
                    const sjpeg_hip_scan_tables* tables, int tables_per_frame, uint32_t* d_out, hipStream_t st,
                    uint32_t* kept = nullptr, const uint32_t* kept_base = nullptr) {
  const bool histogram = pass == kPassHisto, error = pass == kPassError, trellis = pass == kPassStatsTrellis;
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
  HIP_TRY(hipSetDevice(e->device));
  if (int rc0 = order_on_stream(e, st)) return rc0;
  if (e->side_pending) {                             // (pipelined mode: the call runs ordered, behind the engine's stitch)
    if (int rcm = side_mark(e)) return rcm;
    HIP_TRY(hipStreamWaitEvent(st, e->side_done, 0));
  }
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

// the checks every ragged analysis entry point starts with; the format's fields in *a, the frames' geometry in *geo
int ragged_analysis_args(const std::string& who, sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                         const sjpeg_hip_ragged_frame* frames, const void* d_out, ScanArgs* a, int* cls, const SourceLayout** layout,
                         std::vector<FrameGeo>* geo) {
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (frames == nullptr || d_out == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": frames or the output == NULL");
  if (nframes < 1 || nframes > 65535) return fail(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
  if (int rc = ragged_format(who, format, yuv_mode, a, cls, layout)) return rc;
  return ragged_frames(who, format, yuv_mode, nframes, frames, false, geo);
}

}  // namespace

int sjpeg_hip_scan_histogram_ragged_src(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                        const sjpeg_hip_ragged_frame* frames, uint32_t* d_hist, void* stream) {
  ScanArgs a;
  int cls = 0;
  const SourceLayout* layout = nullptr;
  std::vector<FrameGeo> geo;
  if (int rc = ragged_analysis_args("sjpeg_hip_scan_histogram_ragged_src", e, format, yuv_mode, nframes, frames, d_hist, &a, &cls, &layout, &geo)) return rc;
  try {
    return ragged_analysis(e, kPassHisto, yuv_mode, cls, a, layout, nframes, frames, geo, nullptr, 0, d_hist, static_cast<hipStream_t>(stream));
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

int sjpeg_hip_scan_symbol_stats_ragged_src(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                           const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_scan_tables* tables,
                                           int tables_per_frame, uint32_t* d_freq, void* stream) {
  static const std::string who = "sjpeg_hip_scan_symbol_stats_ragged_src";
  ScanArgs a;
  int cls = 0;
  const SourceLayout* layout = nullptr;
  std::vector<FrameGeo> geo;
  if (int rc = ragged_analysis_args(who, e, format, yuv_mode, nframes, frames, d_freq, &a, &cls, &layout, &geo)) return rc;
  if (tables == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": tables == NULL");
  constexpr uint32_t kNotRagged = SJPEG_HIP_QUANT_TRELLIS | SJPEG_HIP_QUANT_KEEP | SJPEG_HIP_QUANT_REPLAY | SJPEG_HIP_RESTART_MARKERS;
  for (int t = 0; t < (tables_per_frame ? nframes : 1); ++t) {
    if (tables[t].flags & kNotRagged) {
      return fail(SJPEG_HIP_EINVAL, who + ": tables[" + std::to_string(t) +
                                        "]: trellis, keep / replay and restart-marker flags are not taken by ragged batches");
    }
  }
  try {
    return ragged_analysis(e, kPassStats, yuv_mode, cls, a, layout, nframes, frames, geo, tables, tables_per_frame, d_freq, static_cast<hipStream_t>(stream));
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

namespace {

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
int counted_bits_launch(sjpeg_hip_engine* e, int yuv_mode, int cls, const ScanArgs& a, const SourceLayout* layout, int nframes,
                        const sjpeg_hip_ragged_frame* frames, const std::vector<FrameGeo>& geo,
                        const sjpeg_hip_scan_tables* tables, int tables_per_frame, bool bound, uint64_t* d_bits,
                        hipStream_t st) {
  std::vector<sjpeg_hip_ragged_frame> planned(frames, frames + nframes);
  for (sjpeg_hip_ragged_frame& fr : planned) {
    fr.out_offset = 0;
    fr.out_capacity = count_capacity(fr.width, fr.height, yuv_mode, bound);
  }
  return ragged_encode(e, yuv_mode, cls, a, layout, nframes, planned.data(), geo, tables, tables_per_frame, nullptr, nullptr,
                       0, 0, nullptr, nullptr, st, reinterpret_cast<unsigned long long*>(d_bits));
}

int counted_bits_args(const std::string& who, sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                      const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_scan_tables* tables, int tables_per_frame,
                      const uint64_t* d_bits, ScanArgs* a, int* cls, const SourceLayout** layout, std::vector<FrameGeo>* geo) {
  if (int rc = ragged_analysis_args(who, e, format, yuv_mode, nframes, frames, d_bits, a, cls, layout, geo)) return rc;
  return ragged_tables_ok(who, tables, tables_per_frame ? nframes : 1);
}

}  // namespace

int sjpeg_hip_scan_quant_error_ragged_src(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                          const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_scan_tables* tables,
                                          int tables_per_frame, uint64_t* d_err, void* stream) {
  static const std::string who = "sjpeg_hip_scan_quant_error_ragged_src";
  ScanArgs a;
  int cls = 0;
  const SourceLayout* layout = nullptr;
  std::vector<FrameGeo> geo;
  if (int rc = ragged_analysis_args(who, e, format, yuv_mode, nframes, frames, d_err, &a, &cls, &layout, &geo)) return rc;
  if (int rc = ragged_tables_ok(who, tables, tables_per_frame ? nframes : 1)) return rc;
  try {
    return ragged_analysis(e, kPassError, yuv_mode, cls, a, layout, nframes, frames, geo, tables, tables_per_frame,
                           reinterpret_cast<uint32_t*>(d_err), static_cast<hipStream_t>(stream));
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

int sjpeg_hip_scan_counted_bits_ragged_src(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                           const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_scan_tables* tables,
                                           int tables_per_frame, uint64_t* d_bits, void* stream) {
  static const std::string who = "sjpeg_hip_scan_counted_bits_ragged_src";
  ScanArgs a;
  int cls = 0;
  const SourceLayout* layout = nullptr;
  std::vector<FrameGeo> geo;
  if (int rc = counted_bits_args(who, e, format, yuv_mode, nframes, frames, tables, tables_per_frame, d_bits, &a, &cls, &layout, &geo)) {
    return rc;
  }
  try {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = counted_bits_launch(e, yuv_mode, cls, a, layout, nframes, frames, geo, tables, tables_per_frame, false, d_bits, st)) return rc;
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
  ScanArgs a;
  int cls = 0;
  const SourceLayout* layout = nullptr;
  std::vector<FrameGeo> geo;
  if (int rc = ragged_analysis_args(who, e, format, yuv_mode, n, sub.data(), d_bits, &a, &cls, &layout, &geo)) return rc;
  if (int rc = e->auto_buf.ensure((static_cast<size_t>(n) * 8 + 15) / 16)) return rc;
  uint64_t* const tmp = reinterpret_cast<uint64_t*>(e->auto_buf.p);
  if (int rc = counted_bits_launch(e, yuv_mode, cls, a, layout, n, sub.data(), geo, subt.data(), tables_per_frame, true, tmp, st)) return rc;
  for (int k = 0; k < n; ++k) {
    HIP_TRY(hipMemcpyAsync(d_bits + which[k], tmp + k, sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  }
  return 0;
}

int counted_bits_first(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes, const sjpeg_hip_ragged_frame* frames,
                       const sjpeg_hip_scan_tables* tables, int tables_per_frame, uint64_t* d_bits, hipStream_t st) {
  static const std::string who = "sjpeg_hip_scan_counted_bits_ragged_src";
  ScanArgs a;
  int cls = 0;
  const SourceLayout* layout = nullptr;
  std::vector<FrameGeo> geo;
  if (int rc = counted_bits_args(who, e, format, yuv_mode, nframes, frames, tables, tables_per_frame, d_bits, &a, &cls, &layout, &geo)) {
    return rc;
  }
  return counted_bits_launch(e, yuv_mode, cls, a, layout, nframes, frames, geo, tables, tables_per_frame, false, d_bits, st);
}

int set_error(int code, const std::string& msg) { return fail(code, msg); }

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
  ScanArgs a;
  int cls = 0;
  const SourceLayout* layout = nullptr;
  std::vector<FrameGeo> geo;
  if (int rc = ragged_format(who, format, yuv_mode, &a, &cls, &layout)) return rc;
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
  ScanArgs a;
  int cls = 0;
  const SourceLayout* layout = nullptr;
  std::vector<FrameGeo> geo;
  if (int rc = ragged_analysis_args(who, e, format, yuv_mode, nframes, frames, d_freq, &a, &cls, &layout, &geo)) return rc;
  for (int f = 0; f < nframes; ++f) {                // (the kept blocks of every frame lie inside the engine's buffer)
    if ((static_cast<size_t>(kept_base[f]) + geo[f].nseg) * kKeptSegWords > e->replay.cap) return fail(SJPEG_HIP_EINVAL, who + ": internal: kept base past the kept blocks");
  }
  return ragged_analysis(e, kPassStatsTrellis, yuv_mode, cls, a, layout, nframes, frames, geo, tables, 1, d_freq, st, e->replay.p, kept_base);
}

int replay_encode_ragged(sjpeg_hip_engine* e, const std::string& who, int format, int yuv_mode, int nframes,
                         const sjpeg_hip_ragged_frame* frames, const sjpeg_hip_scan_tables* tables, const uint32_t* kept_base,
                         const void* headers, const size_t* header_offsets, void* d_out, uint64_t* d_sizes, hipStream_t st,
                         const PackedSink* sink) {
  ScanArgs a;
  int cls = 0;
  const SourceLayout* layout = nullptr;
  std::vector<FrameGeo> geo;
  if (int rc = ragged_format(who, format, yuv_mode, &a, &cls, &layout)) return rc;
  if (int rc = ragged_frames(who, format, yuv_mode, nframes, frames, true, &geo)) return rc;
  for (int f = 0; f < nframes; ++f) {
    if ((static_cast<size_t>(kept_base[f]) + geo[f].nseg) * kKeptSegWords > e->replay.cap) return fail(SJPEG_HIP_EINVAL, who + ": internal: kept base past the kept blocks");
  }
  return ragged_encode(e, yuv_mode, cls, a, layout, nframes, frames, geo, tables, 1, headers, header_offsets, header_offsets[nframes],
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

}  // namespace sjpeg_internal

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
  uint32_t gx = 4096u;
  if (gx > max_chunks) gx = max_chunks;
  hipLaunchKernelGGL(stuff_chunks<false>, dim3(gx, 1), dim3(kThreads), 0, st, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

namespace {
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
}  // namespace

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

// ---- a whole batch with the reference's per-picture analysis (methods 0..6), device-resident ----
// What Encoder::Encode does for ONE picture with adaptive quantization and optimised Huffman
// codes (src/enc.cc:391-448: CollectHistograms + AnalyseHisto, the statistics half of
// SinglePassScanOptimized, headers, the scan), done for nframes pictures with one launch per
// device pass and the per-picture float / Huffman work on the host in between.
namespace {
// (a frame's share of the batch scratch -- kHist, kSums, kTot, kFreq: ragged_aux.h)
static_assert(sjpeg_internal::kKeptSegBytes == kKeptSegWords * sizeof(uint32_t), "a segment's kept blocks");

struct BatchScratch {                 // per host thread: device scratch of sjpeg_hip_encode_batch_src
  void* d_hist = nullptr; size_t hist_cap = 0;
  void* d_sums = nullptr; size_t sums_cap = 0;
  void* d_freq = nullptr; size_t freq_cap = 0;
  void* h_pinned = nullptr; size_t pinned_cap = 0;   // where the device's matrices / counts land on the host
  void* d_pinned = nullptr;                          // ... as the device addresses it
  int device = -1;
  void Drop() {
    if (d_hist) (void)hipFree(d_hist);
    if (d_sums) (void)hipFree(d_sums);
    if (d_freq) (void)hipFree(d_freq);
    if (h_pinned) (void)hipHostFree(h_pinned);
    if (pass_done) (void)hipEventDestroy(pass_done);
    if (call_begin) (void)hipEventDestroy(call_begin);
    pass_done = nullptr; call_begin = nullptr;
    for (auto& e : job_ev) if (e) (void)hipEventDestroy(e);
    job_ev.clear();
    d_hist = d_sums = d_freq = h_pinned = d_pinned = nullptr; hist_cap = sums_cap = freq_cap = pinned_cap = 0;
  }
  hipEvent_t pass_done = nullptr;
  hipEvent_t call_begin = nullptr;                 // on the call's stream before anything of the call: the early uploads wait for it
  std::vector<hipEvent_t> job_ev;                  // one per part or job: behind its last read-back
  bool EnsureJobEvents(size_t n) {
    while (job_ev.size() < n) {
      hipEvent_t e = nullptr;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
      job_ev.push_back(e);
    }
    return true;
  }
  bool EnsureEvents() {
    if (pass_done == nullptr && hipEventCreateWithFlags(&pass_done, hipEventDisableTiming) != hipSuccess) { pass_done = nullptr; return false; }
    if (call_begin == nullptr && hipEventCreateWithFlags(&call_begin, hipEventDisableTiming) != hipSuccess) { call_begin = nullptr; return false; }
    return true;
  }
  bool EnsurePinned(size_t need) {
    if (need <= pinned_cap) return true;
    if (h_pinned) (void)hipHostFree(h_pinned);
    h_pinned = nullptr; d_pinned = nullptr; pinned_cap = 0;
    if (hipHostMalloc(&h_pinned, need, hipHostMallocMapped) != hipSuccess) return false;
    pinned_cap = need;
    // (the address the device writes the block at: the read-backs are kernels too, see stage_copy_kernel)
    if (hipHostGetDevicePointer(&d_pinned, h_pinned, 0) != hipSuccess) { (void)hipGetLastError(); d_pinned = nullptr; }
    return true;
  }
  // device -> h_dst in the pinned block, on stream s: a kernel writes it over the bus (no runtime copy: stage_copy_kernel)
  int ReadBack(hipStream_t s, void* h_dst, const void* d_src, size_t bytes) const {
    void* const dv = d_pinned == nullptr ? nullptr : static_cast<uint8_t*>(d_pinned) + (static_cast<uint8_t*>(h_dst) - static_cast<uint8_t*>(h_pinned));
    return copy_by_kernel(dv, d_src, bytes, s, hipMemcpyDeviceToHost, d_src, h_dst);
  }
  ~BatchScratch() { if (device >= 0) { (void)hipSetDevice(device); Drop(); } }
  bool Ensure(void** p, size_t* cap, size_t need) {
    if (need <= *cap) return true;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    if (hipMalloc(p, need) != hipSuccess) return false;
    *cap = need;
    return true;
  }
};
thread_local BatchScratch g_batch;

// frames f0 .. f0 + nf - 1 take the adapted matrices that came back to h_q ([frame][128]), and the tables of them
void adopt_matrices(const uint8_t* h_q, size_t f0, size_t nf, int yuv_mode, const uint8_t* min_quant, int q_bias,
                    uint8_t* quant, sjpeg_hip_scan_tables* tables) {
  const size_t ntab = yuv_mode == SJPEG_HIP_YUV400 ? 1 : 2;
  for (size_t f = f0; f < f0 + nf; ++f) {
    memcpy(&quant[f * 128], h_q + f * 128, ntab * 64);
    sjpeg_hip_finalize_quant(reinterpret_cast<uint8_t(*)[64]>(&quant[f * 128]), min_quant, q_bias, &tables[f]);
  }
}

// the headers of frames f0 .. f0 + nf - 1 back to back, frame f0 + k's at (*offs)[k] .. (*offs)[k + 1]; dims(k) is its
// width and height.  quant: [frame][128]; specs: [frame][4], or NULL for the default codes; meta (may be empty): meta(k)
// is its metadata, or NULL
int batch_headers(const std::string& who, const std::function<std::pair<int, int>(size_t)>& dims, size_t f0, size_t nf, int yuv_mode, const uint8_t* quant,
                  const sjpeg_hip_huffman_spec* specs, std::vector<uint8_t>* headers, std::vector<size_t>* offs,
                  const std::function<const sjpeg_internal::FrameMeta*(size_t)>& meta = {}) {
  headers->clear();
  offs->assign(nf + 1, 0);
  for (size_t k = 0; k < nf; ++k) {
    const size_t f = f0 + k;
    const std::pair<int, int> wh = dims(k);
    if (!sjpeg_internal::append_frame_header(wh.first, wh.second, yuv_mode, reinterpret_cast<const uint8_t(*)[64]>(quant + f * 128),
                                             specs != nullptr ? specs + f * 4 : nullptr, meta ? meta(k) : nullptr, headers)) {
      return fail(SJPEG_HIP_EINVAL, who + ": header generation failed");
    }
    (*offs)[k + 1] = headers->size();
  }
  return 0;
}

// One call of sjpeg_hip_encode_batch_src: its arguments, and what its steps hand each other frame by frame
struct BatchCall {
  const sjpeg_hip_source* src;
  int width, height, yuv_mode;
  size_t n;
  const uint8_t* min_quant;
  int q_bias, qdelta_max_luma, qdelta_max_chroma;
  bool optimize;
  uint8_t* d_out; size_t out_stride; uint64_t* d_sizes;
  BatchScratch& sc;
  uint8_t* h_q;                                  // [n][128]: the adapted matrices come back here (sc's pinned block) ...
  uint8_t* h_freq;                               // ... and [n][kFreq]: the symbol counts
  uint8_t q_start[2][64];                        // the matrices every frame starts from
  std::vector<uint8_t> quant;                    // [n][128]: every frame's own, adapted range by range
  std::vector<sjpeg_hip_scan_tables> tables;     // [n]
  std::vector<sjpeg_hip_huffman_spec> specs;     // [n][4]: the optimised codes
  std::vector<uint8_t> headers;                  // one range's at a time (batch_headers)
  std::vector<size_t> offs;
};

// frames f0 .. f0 + nf - 1 of a call -- a part, or a job of a lane -- and where their steps go
struct FrameRange {
  size_t f0, nf;
  sjpeg_hip_engine* e;                           // runs the passes
  hipStream_t pass;                              // ... on this stream
  hipStream_t side;                              // the analysis sums and the read-backs
  hipEvent_t ev;                                 // behind the range's latest read-back
};

sjpeg_hip_source range_source(const BatchCall& b, size_t f0) {
  sjpeg_hip_source s = *b.src;
  for (int i = 0; i < 3; ++i) {
    if (s.plane[i] != nullptr) s.plane[i] = static_cast<const uint8_t*>(s.plane[i]) + static_cast<int64_t>(f0) * s.frame_stride[i];
  }
  return s;
}

// The five steps of a range; the first, third and fifth end with launches, and the second and fourth need what the
// event behind the previous one's read-back brought.
// 1. the histogram pass, the analysis sums, the regression on the device (adapt_decide_kernel) -- 128 bytes a frame come
// back instead of the sums' 52 KB, and the host has no float work between the range's histogram pass and its statistics
// launch
int range_analysis(BatchCall& b, const FrameRange& r) {
  const sjpeg_hip_source ps = range_source(b, r.f0);
  const int nf = static_cast<int>(r.nf);
  uint32_t* const d_hist = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(b.sc.d_hist) + r.f0 * kHist);
  if (int rc = sjpeg_hip_scan_histogram_src(r.e, &ps, b.width, b.height, b.yuv_mode, nf, d_hist, r.pass)) return rc;
  uint8_t* const d_grp = static_cast<uint8_t*>(b.sc.d_sums) + r.f0 * (kSums + kTot);      // [nf][kSums] then [nf][kTot]
  int64_t* const d_sums = reinterpret_cast<int64_t*>(d_grp);
  int32_t* const d_tot = reinterpret_cast<int32_t*>(d_grp + r.nf * kSums);
  if (int rc = sjpeg_hip_adapt_sums(d_hist, nf, b.q_start, b.min_quant, d_sums, d_tot, r.side)) return rc;
  uint8_t* const d_q = static_cast<uint8_t*>(b.sc.d_sums) + b.n * (kSums + kTot) + r.f0 * 128;
  if (int rc = adapt_decide(d_sums, d_tot, nf, b.q_start, b.yuv_mode == SJPEG_HIP_YUV400 ? 1 : 2, b.qdelta_max_luma,
                            b.qdelta_max_chroma, d_q, r.side)) return rc;
  if (int rc = b.sc.ReadBack(r.side, b.h_q + r.f0 * 128, d_q, r.nf * 128)) return rc;
  HIP_TRY(hipEventRecord(r.ev, r.side));
  return 0;
}

// 2. the adapted matrices and their tables
void range_adopt(BatchCall& b, const FrameRange& r) {
  adopt_matrices(b.h_q, r.f0, r.nf, b.yuv_mode, b.min_quant, b.q_bias, b.quant.data(), b.tables.data());
}

// 3. the statistics pass -- it leaves its quantized blocks behind (144 B each) and the encode pass replays them: no second
// colour conversion / DCT / quantization (the reference's stored run/levels, src/enc.cc:121-129,374-386) -- and the
// symbol counts back
int range_statistics(BatchCall& b, const FrameRange& r) {
  for (size_t f = r.f0; f < r.f0 + r.nf; ++f) b.tables[f].flags |= SJPEG_HIP_QUANT_KEEP;
  r.e->coefs_use = r.e->coefs_keep;
  const sjpeg_hip_source ps = range_source(b, r.f0);
  uint32_t* const d_freq = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(b.sc.d_freq) + r.f0 * kFreq);
  if (int rc = sjpeg_hip_scan_symbol_stats_multi(r.e, &ps, b.width, b.height, b.yuv_mode, static_cast<int>(r.nf), &b.tables[r.f0],
                                                 d_freq, r.pass)) return rc;
  if (int rc = b.sc.ReadBack(r.side, b.h_freq + r.f0 * kFreq, d_freq, r.nf * kFreq)) return rc;
  dbg_mark("batch: counts read back");
  HIP_TRY(hipEventRecord(r.ev, r.side));
  dbg_mark("batch: event recorded");
  return 0;
}

// 4. the optimised Huffman codes
void range_codes(BatchCall& b, const FrameRange& r) {
  for (size_t f = r.f0; f < r.f0 + r.nf; ++f) {
    b.tables[f].flags = (b.tables[f].flags & ~SJPEG_HIP_QUANT_KEEP) | SJPEG_HIP_QUANT_REPLAY;
    sjpeg_hip_optimize_huffman(reinterpret_cast<const uint32_t*>(b.h_freq + f * kFreq), b.yuv_mode, &b.specs[f * 4], &b.tables[f]);
  }
}

// 5. the headers and the encode pass
int range_encode(BatchCall& b, const FrameRange& r) {
  static const std::string who = "sjpeg_hip_encode_batch_src";
  if (int rc = batch_headers(who, [&](size_t) { return std::make_pair(b.width, b.height); }, r.f0, r.nf, b.yuv_mode,
                             b.quant.data(), b.optimize ? b.specs.data() : nullptr, &b.headers, &b.offs)) return rc;
  const sjpeg_hip_source ps = range_source(b, r.f0);
  return sjpeg_hip_encode_scan_multi(r.e, &ps, b.width, b.height, b.yuv_mode, static_cast<int>(r.nf), &b.tables[r.f0], b.headers.data(),
                                     b.offs.data(), /*append_eoi=*/1, b.d_out + r.f0 * b.out_stride, b.out_stride, b.d_sizes + r.f0, r.pass);
}

}  // namespace

int sjpeg_hip_encode_batch_src(sjpeg_hip_engine* engine, const sjpeg_hip_source* src,
                                          int width, int height, int yuv_mode, int nframes,
                                          const uint8_t quant_in[2][64], const uint8_t* min_quant, int q_bias,
                                          int method, int qdelta_max_luma, int qdelta_max_chroma,
                                          void* d_out, size_t out_stride, uint64_t* d_sizes, void* stream) {
  if (engine == nullptr || src == nullptr || quant_in == nullptr || nframes <= 0) {
    return fail(SJPEG_HIP_EINVAL, "null argument or nframes <= 0");
  }
  if (d_out == nullptr || d_sizes == nullptr) return fail(SJPEG_HIP_EINVAL, "d_out/d_sizes == NULL");
  if (method < 0) method = 0;
  if (method > 6) return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_encode_batch_src: methods 0..6 (trellis goes through the host API)");
  struct PartsGuard {                              // the engine addresses whole calls again when this returns
    sjpeg_hip_engine* e;
    ~PartsGuard() { e->replay_first = 0; e->replay_total = 0; e->reduce_stream = nullptr; e->reduce_ev = nullptr; e->coefs_keep = e->coefs_use = false; e->up_stream = nullptr; e->up_wait = nullptr; }
  } parts_guard{engine};
  try {
    const bool adaptive = method >= 3, optimize = (method != 0) && (method != 3);
    hipStream_t st = static_cast<hipStream_t>(stream);
    BatchScratch& sc = g_batch;
    const int device = engine->device;
    if (sc.device != device) { if (sc.device >= 0) { (void)hipSetDevice(sc.device); sc.Drop(); } sc.device = device; }
    HIP_TRY(hipSetDevice(device));
    const size_t n = static_cast<size_t>(nframes);
    if (adaptive && (!sc.Ensure(&sc.d_hist, &sc.hist_cap, n * kHist) || !sc.Ensure(&sc.d_sums, &sc.sums_cap, n * (kSums + kTot + 128)))) {
      return fail(SJPEG_HIP_ENOMEM, "hipMalloc(batch scratch) failed");
    }
    if (optimize && !sc.Ensure(&sc.d_freq, &sc.freq_cap, n * kFreq)) return fail(SJPEG_HIP_ENOMEM, "hipMalloc(batch scratch) failed");
    if (!sc.EnsurePinned(n * (128 + kFreq)) || !sc.EnsureEvents()) return fail(SJPEG_HIP_ENOMEM, "hipHostMalloc / hipEventCreate(batch scratch) failed");
    uint8_t* const h_q = static_cast<uint8_t*>(sc.h_pinned);
    BatchCall b{src, width, height, yuv_mode, n, min_quant, q_bias, qdelta_max_luma, qdelta_max_chroma, optimize,
                static_cast<uint8_t*>(d_out), out_stride, d_sizes, sc, h_q, h_q + n * 128};
    {
      sjpeg_hip_scan_tables t0;
      memset(&t0, 0, sizeof(t0));
      memcpy(b.q_start, quant_in, sizeof(b.q_start));
      sjpeg_hip_finalize_quant(b.q_start, min_quant, q_bias, &t0);
      sjpeg_hip_default_huffman(&t0);
      b.tables.assign(n, t0);
      b.quant.resize(n * 128);
      for (size_t f = 0; f < n; ++f) memcpy(&b.quant[f * 128], b.q_start, 128);
      b.specs.resize(optimize ? n * 4 : 0);
    }
    // ---- LANES (round 6): jobs of about eight 4K frames, each a complete sequence of passes, on up to four streams at once
    // (sjpeg_hip_engine::lane).  One host thread drives them: a job's next step is taken when the event behind its
    // read-back has passed (polled -- the caller would block in hipEventSynchronize otherwise), whichever job that is.
    static const int lanes_env = getenv("SJPEG_HIP_BATCH_LANES") ? atoi(getenv("SJPEG_HIP_BATCH_LANES")) : -1;   // (A/B: 0 = the two parts of round 5)
    static const double job_px = getenv("SJPEG_HIP_BATCH_JOB_MPIX") ? atof(getenv("SJPEG_HIP_BATCH_JOB_MPIX")) * 1e6 : 66.4e6;
    const double total_px = static_cast<double>(n) * width * height;
    size_t njobs = static_cast<size_t>(total_px / job_px + 0.5);
    if (getenv("SJPEG_HIP_BATCH_JOB_MPIX") == nullptr) njobs = total_px >= 90e6 ? 2 : 1;     // (the sweep: DESIGN.md section 4)
    if (njobs > n) njobs = n;
    if (njobs > 64) njobs = 64;
    // (method 0 in lanes: 0.817 against 0.808 ms for 32 4K frames -- one K1 launch fills the chip by itself, and calls
    // back to back overlap their stitch with the next K1 anyway)
    if (lanes_env != 0 && njobs >= 2 && (adaptive || optimize) && !engine->is_lane) {
      const int nlanes = static_cast<int>(std::min<size_t>(njobs, lanes_env > 0 ? std::min(lanes_env, static_cast<int>(sjpeg_hip_engine::kLanes)) : sjpeg_hip_engine::kLanes));
      if (nlanes == 4 && engine->batch_lane3 == nullptr) HIP_TRY(hipStreamCreateWithFlags(&engine->batch_lane3, hipStreamNonBlocking));
      hipStream_t lane_st[sjpeg_hip_engine::kLanes] = {st, engine->batch_side, engine->batch_up, engine->batch_lane3};
      sjpeg_hip_engine* lane_e[sjpeg_hip_engine::kLanes] = {engine, nullptr, nullptr, nullptr};
      for (int l = 1; l < nlanes; ++l) {
        if (engine->lane[l] == nullptr) {
          sjpeg_hip_engine* c = new (std::nothrow) sjpeg_hip_engine;
          if (c == nullptr) return fail(SJPEG_HIP_ENOMEM, "host allocation failed");
          c->device = engine->device; c->cu_count = engine->cu_count; c->histo_slots = engine->histo_slots;
          c->scratch_limit = engine->scratch_limit; c->ablate = engine->ablate; c->is_lane = true;
          engine->lane[l] = c;
        }
        if (engine->lane_done[l] == nullptr) HIP_TRY(hipEventCreateWithFlags(&engine->lane_done[l], hipEventDisableTiming));
        lane_e[l] = engine->lane[l];
        for (int c = 0; c < 3; ++c) { lane_e[l]->pscale[c] = engine->pscale[c]; lane_e[l]->pbias[c] = engine->pbias[c]; }
      }
      if (engine->lane_in == nullptr) HIP_TRY(hipEventCreateWithFlags(&engine->lane_in, hipEventDisableTiming));
      if (!sc.EnsureJobEvents(njobs)) return fail(SJPEG_HIP_ENOMEM, "hipEventCreate(batch scratch) failed");
      // the lanes' streams start behind everything the caller has put on its own (the pixels, the previous call)
      if (int rco = order_on_stream(engine, st)) return rco;
      HIP_TRY(hipEventRecord(engine->lane_in, st));
      for (int l = 1; l < nlanes; ++l) HIP_TRY(hipStreamWaitEvent(lane_st[l], engine->lane_in, 0));
      // however the call ends from here on, failed or thrown: the caller's stream ends behind every lane (what was launched
      // reads the caller's buffers), and the child engines address whole calls again
      struct LanesGuard {
        sjpeg_hip_engine* e; const hipStream_t* st; int n;
        ~LanesGuard() {
          for (int l = 1; l < n; ++l) {
            if (hipEventRecord(e->lane_done[l], st[l]) == hipSuccess) (void)hipStreamWaitEvent(st[0], e->lane_done[l], 0);
            else (void)hipStreamSynchronize(st[l]);
            e->lane[l]->coefs_keep = e->lane[l]->coefs_use = false;
          }
        }
      } lanes_guard{engine, lane_st, nlanes};
      for (int l = 0; l < nlanes; ++l) lane_e[l]->coefs_keep = adaptive && optimize;
      std::vector<FrameRange> jobs(njobs);
      std::vector<int> phase(njobs, 0);     // 0 not started, 1 matrices on their way, 2 counts on their way, 3 encode launched
      for (size_t j = 0; j < njobs; ++j) {
        const size_t l = j % static_cast<size_t>(nlanes);
        jobs[j] = FrameRange{(n * j) / njobs, (n * (j + 1)) / njobs - (n * j) / njobs, lane_e[l], lane_st[l], lane_st[l], sc.job_ev[j]};
      }
      // a job's next step: at its start, or when the event behind its read-back has passed
      auto advance = [&](size_t j) -> int {
        const FrameRange& r = jobs[j];
        int& ph = phase[j];
        if (ph == 0 && adaptive) { ph = 1; return range_analysis(b, r); }
        if (ph == 1) range_adopt(b, r);
        if (ph < 2 && optimize) { ph = 2; return range_statistics(b, r); }
        if (ph == 2) range_codes(b, r);
        ph = 3;
        return range_encode(b, r);
      };
      static const bool lanes_debug = getenv("SJPEG_HIP_BATCH_DEBUG") != nullptr;    // (measurement aid: the host's timeline on stderr)
      const auto t_lanes = std::chrono::steady_clock::now();
      auto lmark = [&](const char* what, size_t j) {
        if (lanes_debug) fprintf(stderr, "lanes %-22s job %zu  %8.1f us\n", what, j, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_lanes).count());
      };
      size_t done = 0;
      std::vector<size_t> lane_next(static_cast<size_t>(nlanes));      // the next job of a lane that has not started
      for (int l = 0; l < nlanes; ++l) lane_next[static_cast<size_t>(l)] = static_cast<size_t>(l);
      std::vector<long long> lane_busy(static_cast<size_t>(nlanes), -1);   // the job a lane is working on
      int rc_lanes = 0;
      while (done < njobs && rc_lanes == 0) {
        bool moved = false;
        for (int l = 0; l < nlanes && rc_lanes == 0; ++l) {
          const size_t ls = static_cast<size_t>(l);
          if (lane_busy[ls] < 0) {
            if (lane_next[ls] < njobs) {      // (a lane's jobs follow each other: the engine's scratch is one job's)
              lane_busy[ls] = static_cast<long long>(lane_next[ls]);
              lane_next[ls] += static_cast<size_t>(nlanes);
              rc_lanes = advance(static_cast<size_t>(lane_busy[ls]));
              lmark("started", static_cast<size_t>(lane_busy[ls]));
              moved = true;
            }
          } else {
            const size_t j = static_cast<size_t>(lane_busy[ls]);
            const hipError_t q = hipEventQuery(sc.job_ev[j]);
            if (q == hipSuccess) {
              lmark(phase[j] == 1 ? "sums here" : "counts here", j);
              rc_lanes = advance(j);
              lmark(phase[j] == 2 ? "statistics launched" : "encode launched", j);
              moved = true;
            } else if (q != hipErrorNotReady) {
              (void)hipGetLastError();
              rc_lanes = fail(SJPEG_HIP_ERUNTIME, std::string("hipEventQuery: ") + hipGetErrorString(q));
            } else {
              (void)hipGetLastError();
            }
          }
          if (rc_lanes == 0 && lane_busy[ls] >= 0 && phase[static_cast<size_t>(lane_busy[ls])] == 3) { lane_busy[ls] = -1; ++done; moved = true; }
        }
        if (!moved) __builtin_ia32_pause();
      }
      return rc_lanes;
    }
    // ---- PARTS (round 5; two halves from 24 frames on): every device pass of a part is one launch, and the host analysis
    // a part needs between two passes -- the Huffman table builder (10 us a frame) -- runs while the device is busy with
    // the other part's pass instead of leaving it idle.  Everything goes to the caller's stream in order; the host waits
    // on events behind the read-backs only.
    // (measured: 32 4K frames 1.84 -> 1.61 ms in two parts, 16 frames 1.13 -> 1.21: parts of fewer than a dozen
    // frames lose more to their smaller launches than the overlap gives)
    // (round 5, with the persistent histogram kind, early uploads and the fit on the device: 4K frames -- 8 frames 0.40 ms
    // in one part, 0.44 in two; 12 frames 0.54 / 0.55; 16 frames 0.68 / 0.66; 20 frames 0.80 / 0.79; 24 frames 0.99 / 0.89:
    // two parts from 125 Mpixels on.  With the regression on the host it was 80: 12 frames 0.64 / 0.57)
    const bool big = n >= 2 && static_cast<double>(n) * width * height >= 125e6;
    const int nparts = ((n >= 24 || big) && (adaptive || optimize)) ? 2 : 1;
    if (!sc.EnsureJobEvents(static_cast<size_t>(nparts))) return fail(SJPEG_HIP_ENOMEM, "hipEventCreate(batch scratch) failed");
    // (in parts: the sums of a part and their read-back go to the side stream, behind the pass that made
    // the partials, so that the next part's pass starts right behind this one's)
    hipStream_t rs = st;
    if (nparts > 1) {
      engine->reduce_stream = engine->batch_side; engine->reduce_ev = sc.pass_done;
      engine->replay_total = nframes;
      rs = engine->batch_side;
      // The early uploads overwrite what the PREVIOUS call's kernels may still be reading -- its per-frame tables (K1 on
      // its stream), its headers and header offsets (the stitch kernels; the engine's side stream in pipelined mode).  An
      // adaptive call's first upload follows a host wait on its own histogram pass, which sits behind that work on the
      // call's stream; a call with optimised tables alone (methods 1, 2) uploads at once, and the side stream is behind
      // nobody's wait: the upload stream is put behind both before anything goes to it (two asynchronous
      // method-1 batches back to back: test_back_to_back_batches_without_a_host_wait).
      if (int rco = order_on_stream(engine, st)) return rco;
      HIP_TRY(hipEventRecord(sc.call_begin, st));
      HIP_TRY(hipStreamWaitEvent(engine->batch_up, sc.call_begin, 0));
      if (engine->side_pending) {
        if (int rcs = side_mark(engine)) return rcs;
        HIP_TRY(hipStreamWaitEvent(engine->batch_up, engine->side_done, 0));
      }
      engine->up_stream = engine->batch_up;
    }
    engine->coefs_keep = adaptive && optimize;
    std::vector<FrameRange> parts(static_cast<size_t>(nparts));
    for (int p = 0; p < nparts; ++p) {               // (the larger parts first: the engine scratch is sized once)
      const size_t f0 = (n * p + nparts - 1) / nparts;
      parts[p] = FrameRange{f0, (n * (p + 1) + nparts - 1) / nparts - f0, engine, st, rs, sc.job_ev[p]};
    }
    if (adaptive) {
      for (const FrameRange& r : parts) {
        engine->replay_first = static_cast<int>(r.f0);
        if (int rc = range_analysis(b, r)) return rc;
      }
    }
    static const bool batch_debug = getenv("SJPEG_HIP_BATCH_DEBUG") != nullptr;      // (measurement aid: host timeline on stderr)
    const auto t_start = std::chrono::steady_clock::now();
    auto mark = [&](const char* what, int p) {
      static const auto t_epoch = std::chrono::steady_clock::now();
      if (batch_debug) fprintf(stderr, "batch %-18s part %d  %8.1f us  (abs %10.1f)\n", what, p, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count(),
                               std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_epoch).count());
    };
    mark("hist launched", -1);
    // (part p's matrices are adopted while the device works on the histogram of part p + 1 / the statistics of part p - 1)
    for (int p = 0; p < nparts; ++p) {
      const FrameRange& r = parts[p];
      if (adaptive) {
        mark("wait sums", p);
        HIP_TRY(hipEventSynchronize(r.ev));
        mark("sums here", p);
        range_adopt(b, r);
      }
      mark("adapted", p);
      if (optimize) {
        engine->replay_total = nframes; engine->replay_first = static_cast<int>(r.f0);
        if (int rc = range_statistics(b, r)) return rc;
        mark("stats launched", p);
      }
    }
    // (part p's table builder runs while the device counts the symbols of part p + 1 / codes part p - 1)
    for (int p = 0; p < nparts; ++p) {
      const FrameRange& r = parts[p];
      if (optimize) {
        mark("wait freq", p);
        HIP_TRY(hipEventSynchronize(r.ev));
        mark("freq here", p);
        range_codes(b, r);
        engine->replay_total = nframes; engine->replay_first = static_cast<int>(r.f0);
      }
      mark("tables built", p);
      if (engine->replay_total > 0) engine->replay_first = static_cast<int>(r.f0);     // (where this part's tables / headers lie)
      if (int rc = range_encode(b, r)) return rc;
      mark("encode launched", p);
    }
    return 0;
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

// ---- a ragged batch with the reference's per-picture analysis (methods 0..6) ----
// The flow of sjpeg_hip_encode_batch_src over frames of different sizes: the ragged histogram, the adaptation kernels with
// a starting matrix per frame, one read-back and wait; the tables; the ragged statistics, one read-back and wait; the
// Huffman codes and the headers on the host; the ragged encode.  No lanes, no parts, no coefficients kept between passes
// -- but for methods 7 and 8 (sjpeg_hip_encode_ragged_trellis_src), the reference's trellis: their statistics step
// quantizes with the trellis, priced with the standard AC code lengths, and leaves its blocks in the engine's `replay`
// buffer (group after group, frame after frame, kKeptSegWords a segment); their encode step replays them.
// The frames come in MODE GROUPS (sjpeg_hip_encode_ragged_auto_src: RGB 4:2:0, 4:4:4, 4:0:0 and the sharp frames' planar
// 4:2:0 -- K1 is templated on the mode, so a group is a grid of its own): every pass runs over all groups before its
// one wait, so the host waits do not grow with the number of groups.  sjpeg_hip_encode_ragged_batch_src is one group.
namespace {

struct RaggedGroup {
  int format = 0, yuv_mode = 0;                   // SJPEG_HIP_SRC_*, SJPEG_HIP_YUV*
  std::vector<sjpeg_hip_ragged_frame> frames;     // in group order
  std::vector<int> index;                         // the caller's number of each frame
  ScanArgs a;                                     // the format's fields (ragged_format)
  int cls = kSrcPlanes;
  const SourceLayout* layout = nullptr;
  std::vector<FrameGeo> geo;
};

__global__ __launch_bounds__(256) void scatter_sizes_kernel(const unsigned long long* sizes, const uint32_t* index, int n,
                                                            unsigned long long* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[index[i]] = sizes[i];
}

// The method 0..6 flow over the groups (their frames checked, their format fields and geometry set).  d_sizes: the
// caller's sizes; with more than one group, or frames out of the caller's order, the groups' sizes land in the engine's
// auto_buf first and one kernel scatters them.  last_ready (may be empty): enqueues what the LAST group's frames are
// made of (the sharp conversion), right in front of the first kernel that reads them -- behind the other groups' first
// pass, so that the few uploads between it and the pass's wait never have to wait for it on the host (the engine's
// staging ring holds four uploads).
int ragged_batch_groups(sjpeg_hip_engine* e, const std::string& who, std::vector<RaggedGroup>& groups,
                        const uint8_t (*quant_in)[2][64], int quant_per_frame, const uint8_t* min_quant, int q_bias,
                        int method, int qdelta_max_luma, int qdelta_max_chroma, void* d_out, uint64_t* d_sizes,
                        hipStream_t st, const std::function<int()>& last_ready = {},
                        const sjpeg_internal::PackedSink* sink = nullptr) {
  const bool adaptive = method >= 3, optimize = (method != 0) && (method != 3), trellis = method >= 7;
  size_t n = 0;
  std::vector<size_t> gbase;
  for (const RaggedGroup& g : groups) { gbase.push_back(n); n += g.frames.size(); }
  if (n == 0) return 0;
  // (trellis) the first kept segment of every group, and of every frame inside its group
  // (trellis) every frame's first kept segment: the prefix sums over the groups' frames, handed to the statistics and the
  // replay through the one table both kinds address the kept blocks by
  std::vector<std::vector<uint32_t>> fkept(groups.size());
  size_t kept_segs = 0;
  for (size_t gi = 0; trellis && gi < groups.size(); ++gi) {
    for (const FrameGeo& fg : groups[gi].geo) { fkept[gi].push_back(static_cast<uint32_t>(kept_segs)); kept_segs += static_cast<size_t>(fg.nseg); }
  }
  if (kept_segs > 0xffffffffull) return fail(SJPEG_HIP_EINVAL, who + ": too many segments for the kept blocks");
  bool last_made = !last_ready;
  auto ready = [&](size_t gi) -> int {
    if (last_made || gi + 1 != groups.size()) return 0;
    last_made = true;
    return last_ready();
  };
  // every frame's starting matrices and tables, as sjpeg_hip_encode_batch_src makes them of its one matrix; frame k of
  // group g is frame gbase[g] + k of the call here
  std::vector<sjpeg_hip_scan_tables> tables(n);
  std::vector<uint8_t> quant(n * 128);
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    for (size_t k = 0; k < groups[gi].frames.size(); ++k) {
      const size_t f = gbase[gi] + k;
      uint8_t* const q = &quant[f * 128];
      memcpy(q, quant_in[quant_per_frame ? groups[gi].index[k] : 0], 128);
      memset(&tables[f], 0, sizeof(tables[f]));
      sjpeg_hip_finalize_quant(reinterpret_cast<uint8_t(*)[64]>(q), min_quant, q_bias, &tables[f]);
      sjpeg_hip_default_huffman(&tables[f]);
      if (trellis) {
        // the rate of the trellis is priced with the STANDARD AC code lengths (InitCodes(true), src/enc.cc:330-334),
        // whatever codes the stream ends with
        tables[f].flags |= SJPEG_HIP_QUANT_TRELLIS;
        for (int t = 0; t < 2; ++t) {
          for (int sym = 0; sym < 256; ++sym) tables[f].trellis_len[t][sym] = static_cast<uint8_t>(tables[f].ac_codes[t][sym] & 0xff);
        }
      }
    }
  }
  static const bool batch_debug = getenv("SJPEG_HIP_BATCH_DEBUG") != nullptr;      // (measurement aid: host timeline on stderr)
  const auto t_start = std::chrono::steady_clock::now();
  auto mark = [&](const char* what) {
    if (batch_debug) fprintf(stderr, "ragged %-18s %8.1f us\n", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count());
  };
  // the analysis goes in chunks of consecutive frames of a group whose scratch -- the pass's partials (the histogram's
  // at most one per segment) and the per-frame results -- stays inside the engine's limit
  auto chunks_of = [&](const RaggedGroup& g, size_t per_seg, size_t per_frame) {
    std::vector<std::pair<size_t, size_t>> c;      // (first frame, frames)
    const size_t ng = g.frames.size();
    size_t f0 = 0, bytes = 0;
    for (size_t f = 0; f < ng; ++f) {
      const size_t b = static_cast<size_t>(g.geo[f].nseg) * per_seg + per_frame;
      if (f > f0 && bytes + b > e->scratch_limit) { c.emplace_back(f0, f - f0); f0 = f; bytes = 0; }
      bytes += b;
    }
    c.emplace_back(f0, ng - f0);
    return c;
  };
  BatchScratch& sc = g_batch;
  if (sc.device != e->device) { if (sc.device >= 0) { (void)hipSetDevice(sc.device); sc.Drop(); } sc.device = e->device; }
  HIP_TRY(hipSetDevice(e->device));
  if (!sc.EnsurePinned(n * (adaptive ? 128 : 0) + (optimize ? n * kFreq : 0) + 16) || !sc.EnsureEvents()) {
    return fail(SJPEG_HIP_ENOMEM, "hipHostMalloc / hipEventCreate(batch scratch) failed");
  }
  uint8_t* const h_q = static_cast<uint8_t*>(sc.h_pinned);                     // [n][128]
  uint8_t* const h_freq = h_q + (adaptive ? n * 128 : 0);                       // [n][kFreq]
  if (adaptive) {
    // 1. histograms, the adaptation with each frame's own starting matrices, the adapted matrices back
    std::vector<std::vector<std::pair<size_t, size_t>>> chunks;
    size_t most = 0;
    for (const RaggedGroup& g : groups) {
      chunks.push_back(chunks_of(g, kHistoPartialWords * sizeof(uint32_t), kHist + kSums + kTot));
      for (const auto& c : chunks.back()) most = std::max(most, c.second);
    }
    // d_sums: [chunk][kSums] | [chunk][kTot] | the starting matrices [n][128] | the adapted ones [n][128]
    if (!sc.Ensure(&sc.d_hist, &sc.hist_cap, most * kHist) || !sc.Ensure(&sc.d_sums, &sc.sums_cap, most * (kSums + kTot) + n * 256)) {
      return fail(SJPEG_HIP_ENOMEM, "hipMalloc(batch scratch) failed");
    }
    uint8_t* const d_qs = static_cast<uint8_t*>(sc.d_sums) + most * (kSums + kTot);
    uint8_t* const d_qa = d_qs + n * 128;
    if (int rc = order_on_stream(e, st)) return rc;
    if (int rc = upload(e, d_qs, quant.data(), n * 128, st)) return rc;
    if (int rc = sync_uploads(e, st)) return rc;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      const RaggedGroup& g = groups[gi];
      const int ntab = g.yuv_mode == SJPEG_HIP_YUV400 ? 1 : 2;
      if (int rc = ready(gi)) return rc;
      for (const auto& c : chunks[gi]) {
        uint32_t* const d_hist = static_cast<uint32_t*>(sc.d_hist);
        if (int rc = ragged_analysis(e, kPassHisto, g.yuv_mode, g.cls, g.a, g.layout, static_cast<int>(c.second), g.frames.data() + c.first,
                                     std::vector<FrameGeo>(g.geo.begin() + c.first, g.geo.begin() + c.first + c.second),
                                     nullptr, 0, d_hist, st)) return rc;
        AdaptArgs s;
        s.hist = d_hist;
        s.sums = static_cast<long long*>(sc.d_sums);
        s.totlast = reinterpret_cast<int*>(static_cast<uint8_t*>(sc.d_sums) + c.second * kSums);
        memset(s.quant, 0, sizeof(s.quant));
        if (min_quant != nullptr) memcpy(s.min_quant, min_quant, sizeof(s.min_quant)); else memset(s.min_quant, 1, sizeof(s.min_quant));
        s.quant_f = d_qs + (gbase[gi] + c.first) * 128;
        hipLaunchKernelGGL(adapt_sums_kernel<true>, dim3(64, 2, c.second), dim3(64), 0, st, s);
        HIP_TRY(hipGetLastError());
        DecideArgs d;
        d.sums = s.sums; d.totlast = s.totlast;
        d.quant_out = d_qa + (gbase[gi] + c.first) * 128;
        memset(d.quant_in, 0, sizeof(d.quant_in));
        d.last_step[0] = qdelta_max_luma + 12;
        d.last_step[1] = qdelta_max_chroma + 12;
        d.quant_f = s.quant_f;
        hipLaunchKernelGGL(adapt_decide_kernel<true>, dim3(ntab, c.second), dim3(64), 0, st, d);
        HIP_TRY(hipGetLastError());
      }
    }
    if (int rc = sc.ReadBack(st, h_q, d_qa, n * 128)) return rc;
    HIP_TRY(hipEventRecord(sc.pass_done, st));
    mark("hist launched");
    HIP_TRY(hipEventSynchronize(sc.pass_done));
    mark("matrices here");
    // 2. the tables of the adapted matrices
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      adopt_matrices(h_q, gbase[gi], groups[gi].frames.size(), groups[gi].yuv_mode, min_quant, q_bias, quant.data(), tables.data());
    }
  }
  std::vector<sjpeg_hip_huffman_spec> specs(optimize ? n * 4 : 0);
  if (optimize) {
    // 3. the symbol counts with each frame's tables, back to the host
    std::vector<std::vector<std::pair<size_t, size_t>>> chunks;
    size_t most = 0;
    for (const RaggedGroup& g : groups) {
      chunks.push_back(chunks_of(g, kStatsWords * sizeof(uint32_t), kFreq));
      for (const auto& c : chunks.back()) most = std::max(most, c.second);
    }
    if (!sc.Ensure(&sc.d_freq, &sc.freq_cap, most * kFreq)) return fail(SJPEG_HIP_ENOMEM, "hipMalloc(batch scratch) failed");
    if (trellis) {
      if (int rc = e->replay.ensure(kept_segs * kKeptSegWords)) return rc;
      e->replay_w = e->replay_h = e->replay_mode = e->replay_nframes = 0;      // (no uniform call's kept blocks any more)
    }
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      const RaggedGroup& g = groups[gi];
      if (int rc = ready(gi)) return rc;
      for (const auto& c : chunks[gi]) {
        uint32_t* const d_freq = static_cast<uint32_t*>(sc.d_freq);
        if (int rc = ragged_analysis(e, trellis ? kPassStatsTrellis : kPassStats, g.yuv_mode, g.cls, g.a, g.layout, static_cast<int>(c.second),
                                     g.frames.data() + c.first,
                                     std::vector<FrameGeo>(g.geo.begin() + c.first, g.geo.begin() + c.first + c.second),
                                     &tables[gbase[gi] + c.first], 1, d_freq, st,
                                     trellis ? e->replay.p : nullptr, trellis ? &fkept[gi][c.first] : nullptr)) return rc;
        if (int rc = sc.ReadBack(st, h_freq + (gbase[gi] + c.first) * kFreq, d_freq, c.second * kFreq)) return rc;
      }
    }
    HIP_TRY(hipEventRecord(sc.pass_done, st));
    mark("stats launched");
    HIP_TRY(hipEventSynchronize(sc.pass_done));
    mark("counts here");
    // 4. the optimised codes (the host's share that grows with the batch)
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      for (size_t f = gbase[gi]; f < gbase[gi] + groups[gi].frames.size(); ++f) {
        sjpeg_hip_optimize_huffman(reinterpret_cast<const uint32_t*>(h_freq + f * kFreq), groups[gi].yuv_mode, &specs[f * 4], &tables[f]);
      }
    }
  }
  // where the groups' sizes go: the caller's array when there is one group in the caller's order, else auto_buf
  bool in_order = groups.size() == 1;
  for (size_t k = 0; in_order && k < groups[0].index.size(); ++k) in_order = groups[0].index[k] == static_cast<int>(k);
  unsigned long long* d_gsizes = reinterpret_cast<unsigned long long*>(d_sizes);
  uint32_t* d_index = nullptr;
  if (!in_order) {
    if (int rc = e->auto_buf.ensure((n * 12 + 15) / 16 + 1)) return rc;
    d_gsizes = reinterpret_cast<unsigned long long*>(e->auto_buf.p);
    d_index = reinterpret_cast<uint32_t*>(d_gsizes + n);
    std::vector<uint32_t> index(n);
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      for (size_t k = 0; k < groups[gi].index.size(); ++k) index[gbase[gi] + k] = static_cast<uint32_t>(groups[gi].index[k]);
    }
    if (int rc = upload(e, d_index, index.data(), n * 4, st)) return rc;
    if (int rc = sync_uploads(e, st)) return rc;
  }
  // 4. (all methods) the headers, each frame's own; 5. the ragged encode of every group, asynchronous on the stream
  const bool one_table = !quant_per_frame && !adaptive && !optimize;
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    RaggedGroup& g = groups[gi];
    const size_t ng = g.frames.size();
    std::vector<uint8_t> headers;
    std::vector<size_t> offs;
    if (int rc = batch_headers(who, [&](size_t k) { return std::make_pair(g.frames[k].width, g.frames[k].height); }, gbase[gi], ng,
                               g.yuv_mode, quant.data(), optimize ? specs.data() : nullptr, &headers, &offs,
                               [&](size_t k) { return sjpeg_internal::frame_meta(e, g.index[k]); })) return rc;
    if (gi + 1 == groups.size()) mark("tables built");
    if (int rc = ready(gi)) return rc;
    if (sink != nullptr) {               // packed output: the group's frames under the caller's numbers
      sjpeg_internal::PackedSink gs = *sink;
      std::vector<int> gidx(ng);
      for (size_t k = 0; k < ng; ++k) gidx[k] = sink->index != nullptr ? sink->index[g.index[k]] : g.index[k];
      gs.index = gidx.data();
      if (int rc = ragged_encode(e, g.yuv_mode, g.cls, g.a, g.layout, static_cast<int>(ng), g.frames.data(), g.geo, &tables[gbase[gi]],
                                 (trellis || !one_table) ? 1 : 0, headers.data(), offs.data(), offs[ng], /*append_eoi=*/1, nullptr,
                                 reinterpret_cast<uint64_t*>(d_gsizes + gbase[gi]), st, nullptr,
                                 trellis ? e->replay.p : nullptr, &gs, trellis ? fkept[gi].data() : nullptr)) return rc;
      continue;
    }
    const int rc = trellis ? ragged_encode(e, g.yuv_mode, g.cls, g.a, g.layout, static_cast<int>(ng), g.frames.data(), g.geo, &tables[gbase[gi]],
                                           1, headers.data(), offs.data(), offs[ng], /*append_eoi=*/1, d_out,
                                           reinterpret_cast<uint64_t*>(d_gsizes + gbase[gi]), st, nullptr,
                                           e->replay.p, nullptr, fkept[gi].data())
                           : sjpeg_hip_encode_ragged_src(e, g.format, g.yuv_mode, static_cast<int>(ng), g.frames.data(), &tables[gbase[gi]],
                                                         one_table ? 0 : 1, headers.data(), offs.data(), /*append_eoi=*/1, d_out,
                                                         reinterpret_cast<uint64_t*>(d_gsizes + gbase[gi]), st);
    if (rc) return rc;
  }
  if (!in_order) {
    hipLaunchKernelGGL(scatter_sizes_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, st,
                       d_gsizes, d_index, static_cast<int>(n), reinterpret_cast<unsigned long long*>(d_sizes));
    HIP_TRY(hipGetLastError());
  }
  mark("encode launched");
  return 0;
}

}  // namespace

}  // extern "C"

// sjpeg_hip_encode_ragged_batch_src; sink != NULL: packed output (ragged_aux.h)
int sjpeg_internal::ragged_batch_flow(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                      const sjpeg_hip_ragged_frame* frames, const uint8_t (*quant_in)[2][64],
                                      int quant_per_frame, const uint8_t* min_quant, int q_bias, int method,
                                      int qdelta_max_luma, int qdelta_max_chroma, void* d_out, uint64_t* d_sizes,
                                      void* stream, const PackedSink* sink) {
  static const std::string who = "sjpeg_hip_encode_ragged_batch_src";
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (frames == nullptr || quant_in == nullptr || d_out == nullptr || d_sizes == nullptr) {
    return fail(SJPEG_HIP_EINVAL, who + ": frames, quant, d_out or d_sizes == NULL");
  }
  if (method < 0 || method > 6) return fail(SJPEG_HIP_EINVAL, who + ": methods 0..6 (trellis goes through the host API)");
  if (qdelta_max_luma < -12 || qdelta_max_luma > 12 || qdelta_max_chroma < -12 || qdelta_max_chroma > 12) {
    return fail(SJPEG_HIP_EINVAL, who + ": qdelta_max outside -12 .. 12");
  }
  if (nframes < 1 || nframes > 65535) return fail(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
  std::vector<RaggedGroup> groups(1);
  RaggedGroup& g = groups[0];
  if (int rc = ragged_format(who, format, yuv_mode, &g.a, &g.cls, &g.layout)) return rc;
  if (int rc = ragged_frames(who, format, yuv_mode, nframes, frames, true, &g.geo)) return rc;
  try {
    g.format = format; g.yuv_mode = yuv_mode;
    g.frames.assign(frames, frames + nframes);
    g.index.resize(nframes);
    for (int f = 0; f < nframes; ++f) g.index[f] = f;
    return ragged_batch_groups(e, who, groups, quant_in, quant_per_frame, min_quant, q_bias, method, qdelta_max_luma,
                               qdelta_max_chroma, d_out, d_sizes, static_cast<hipStream_t>(stream), {}, sink);
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

extern "C" {

int sjpeg_hip_encode_ragged_batch_src(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                      const sjpeg_hip_ragged_frame* frames, const uint8_t (*quant_in)[2][64],
                                      int quant_per_frame, const uint8_t* min_quant, int q_bias, int method,
                                      int qdelta_max_luma, int qdelta_max_chroma, void* d_out, uint64_t* d_sizes,
                                      void* stream) {
  return sjpeg_internal::ragged_batch_flow(e, format, yuv_mode, nframes, frames, quant_in, quant_per_frame, min_quant, q_bias,
                                           method, qdelta_max_luma, qdelta_max_chroma, d_out, d_sizes, stream, nullptr);
}

// ---- ragged batches with SJPEG_YUV_AUTO / SJPEG_YUV_SHARP ----
namespace {

// the engine's upload for the sharp conversion's descriptors (sharp_yuv.hip)
int engine_upload(void* ctx, void* d_dst, const void* src, size_t bytes, hipStream_t st) {
  sjpeg_hip_engine* const e = static_cast<sjpeg_hip_engine*>(ctx);
  if (int rc = upload(e, d_dst, src, bytes, st)) return rc;
  return sync_uploads(e, st);
}

// every frame of a ragged call of an RGB-like format (source_layout.h) checked (the message names the frame)
int rgb_ragged_frames(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames) {
  const SourceLayout* const L = source_layout(format);
  if (L == nullptr || !L->rgb_like) {
    return fail(SJPEG_HIP_EINVAL, who + ": SJPEG_YUV_AUTO, SJPEG_YUV_SHARP and the riskiness take RGB, BGRA or RGBA (packed) or planar RGB sources");
  }
  if (nframes < 1 || nframes > 65535) return fail(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
  std::vector<FrameGeo> geo;
  return ragged_frames(who, format, SJPEG_HIP_YUV444, nframes, frames, false, &geo);
}

// the ragged riskiness: descriptors into auto_buf (which holds nframes * 3 sums behind them as well), then the launch;
// d_sums == NULL: the sums go to auto_buf, *sums_at says where
int risk_ragged(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames, const uint8_t* d_table,
                uint64_t* d_sums, hipStream_t st, uint64_t** sums_at) {
  std::vector<sjpeg_internal::RiskFrame> desc(nframes);
  unsigned long long total = 0;
  for (int f = 0; f < nframes; ++f) {
    sjpeg_internal::RiskFrame& d = desc[f];
    memset(&d, 0, sizeof(d));
    d.rgb = static_cast<const uint8_t*>(frames[f].plane[0]);
    d.row_stride = frames[f].row_stride[0];
    layout_rgb_offsets(*source_layout(format), frames[f].plane, &d.g_off, &d.b_off);
    sjpeg_internal::risk_frame_plan(frames[f].width, frames[f].height, &d);
    d.wg_base = static_cast<unsigned>(total);
    total += static_cast<unsigned long long>(d.bands) * static_cast<unsigned long long>(d.cols);
  }
  if (total > 0x7fffffffull) return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_riskiness_ragged_src: the batch has too many workgroups");
  const size_t desc_bytes = align16(sizeof(sjpeg_internal::RiskFrame) * nframes);
  const size_t need = (desc_bytes + static_cast<size_t>(nframes) * 24 + 15) / 16;
  if (int rc = e->auto_buf.ensure(std::max(need, e->auto_buf.cap))) return rc;
  uint8_t* const base = reinterpret_cast<uint8_t*>(e->auto_buf.p);
  if (d_sums == nullptr) d_sums = reinterpret_cast<uint64_t*>(base + desc_bytes);
  if (sums_at != nullptr) *sums_at = d_sums;
  if (int rc = upload(e, base, desc.data(), sizeof(sjpeg_internal::RiskFrame) * nframes, st)) return rc;
  if (int rc = sync_uploads(e, st)) return rc;
  if (sjpeg_internal::risk_ragged_launch(format, e->pscale, e->pbias, reinterpret_cast<const sjpeg_internal::RiskFrame*>(base), nframes,
                                         static_cast<unsigned>(total), d_table, d_sums, st) != 0) {
    return fail(SJPEG_HIP_ERUNTIME, std::string("risk_scan_ragged launch failed: ") + hipGetErrorString(hipGetLastError()));
  }
  return 0;
}

// the call is ordered behind the engine's earlier work (another stream, pipelined mode's stitch stream)
int ragged_ordered(sjpeg_hip_engine* e, hipStream_t st) {
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = order_on_stream(e, st)) return rc;
  if (e->side_pending) {
    if (int rc = side_mark(e)) return rc;
    HIP_TRY(hipStreamWaitEvent(st, e->side_done, 0));
  }
  return 0;
}

}  // namespace

}  // extern "C"

namespace sjpeg_internal {
bool RiskTableSnapshot(int* generation, std::vector<uint8_t>* table, std::string* err);   // host_api.cc
}

extern "C" {

// The riskiness table the host API uses (installed, SJPEG_HIP_RISKINESS_TABLE, riskiness.bin beside the library), in the
// engine's device copy: uploaded once, and again when sjpeg_hip_set_riskiness_table() changes it.
static int engine_risk_table(sjpeg_hip_engine* e, const std::string& who, hipStream_t st, const uint8_t** d_table) {
  std::string err;
  std::vector<uint8_t> tab;
  int gen = e->risk_table.p != nullptr ? e->risk_generation : -1;
  if (!sjpeg_internal::RiskTableSnapshot(&gen, &tab, &err)) return fail(SJPEG_HIP_EINVAL, who + ": " + err);
  if (!tab.empty()) {
    if (int rc = e->risk_table.ensure(SJPEG_HIP_RISKINESS_TABLE_SIZE)) return rc;
    if (int rc = upload(e, e->risk_table.p, tab.data(), SJPEG_HIP_RISKINESS_TABLE_SIZE, st)) return rc;
    if (int rc = sync_uploads(e, st)) return rc;
    e->risk_generation = gen;
  }
  *d_table = e->risk_table.p;
  return 0;
}

int sjpeg_hip_riskiness_ragged_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                   const uint8_t* d_table, uint64_t* d_sums, void* stream) {
  static const std::string who = "sjpeg_hip_riskiness_ragged_src";
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (frames == nullptr || d_sums == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": frames or d_sums == NULL");
  try {
    if (int rc = rgb_ragged_frames(who, format, nframes, frames)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = ragged_ordered(e, st)) return rc;
    if (d_table == nullptr) {                        // the table the host API uses
      if (int rc = engine_risk_table(e, who, st, &d_table)) return rc;
    }
    return risk_ragged(e, format, nframes, frames, d_table, d_sums, st, nullptr);
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

int sjpeg_hip_sharp_yuv_ragged(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                               uint8_t* const* d_y, uint8_t* const* d_u, uint8_t* const* d_v, void* d_workspace,
                               size_t workspace_size, void* stream) {
  static const std::string who = "sjpeg_hip_sharp_yuv_ragged";
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  try {
    hipStream_t st = static_cast<hipStream_t>(stream);
    std::string err;
    const SourceLayout* const L = source_layout(format);
    if (L == nullptr || !L->rgb_like) {
      return fail(SJPEG_HIP_EINVAL, who + ": the sharp conversion takes RGB, BGRA or RGBA (packed) or planar RGB sources");
    }
    if (int rc = ragged_ordered(e, st)) return rc;
    if (int rc = sjpeg_internal::sharp_ragged_run(format, e->pscale, e->pbias, nframes, frames, d_y, d_u, d_v, d_workspace, workspace_size, st,
                                                  engine_upload, e, &err)) {
      return fail(rc, who + ": " + err);
    }
    return 0;
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

// The flow of the ragged calls that take a SjpegYUVMode (frames, format and arguments checked): the ragged riskiness and ONE
// read-back (AUTO only), the verdicts on the host, the sharp frames converted into the engine's planes arena, then the
// method's flow over up to four mode groups (ragged_batch_groups; a fixed mode 1 / 3 / 4 is one group of the caller's
// format).  The sharp planes and workspace -- and, methods 7 and 8, the kept blocks of the trellis, 36 864 bytes a segment
// -- count against the scratch limit: past it the call goes in parts of consecutive frames, each a complete flow.
static int ragged_modes_flow(sjpeg_hip_engine* e, const std::string& who, int format, int yuv_mode, int nframes,
                             const sjpeg_hip_ragged_frame* frames, const uint8_t (*quant_in)[2][64], int quant_per_frame,
                             const uint8_t* min_quant, int q_bias, int method, int qdelta_max_luma, int qdelta_max_chroma,
                             void* d_out, uint64_t* d_sizes, int* modes, void* stream,
                             const sjpeg_internal::PackedSink* sink = nullptr) {
  const bool trellis = method >= 7;
  static const bool batch_debug = getenv("SJPEG_HIP_BATCH_DEBUG") != nullptr;      // (measurement aid: host timeline on stderr)
  const auto t_start = std::chrono::steady_clock::now();
  auto mark = [&](const char* what) {
    if (batch_debug) fprintf(stderr, "auto   %-18s %8.1f us\n", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count());
  };
  const size_t n = static_cast<size_t>(nframes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = ragged_ordered(e, st)) return rc;
  // the auto_buf of the whole call, once: riskiness descriptors and sums, then the groups' sizes and frame numbers
  if (int rc = e->auto_buf.ensure(std::max((align16(sizeof(sjpeg_internal::RiskFrame) * n) + n * 24 + 15) / 16 + 1, (n * 12 + 15) / 16 + 1))) return rc;
  std::vector<int> mode(n, yuv_mode == kYuvAuto ? kYuvSharp : yuv_mode);
  if (yuv_mode == kYuvAuto) {
    // 1. the riskiness of every frame (the table on this device, uploaded again when it changed), one read-back
    const uint8_t* d_table = nullptr;
    if (int rc = engine_risk_table(e, who, st, &d_table)) return rc;
    uint64_t* d_sums = nullptr;
    if (int rc = risk_ragged(e, format, nframes, frames, d_table, nullptr, st, &d_sums)) return rc;
    std::vector<uint64_t> sums(n * 3);
    HIP_TRY(hipMemcpyAsync(sums.data(), d_sums, n * 24, hipMemcpyDeviceToHost, st));
    mark("risk launched");
    HIP_TRY(hipStreamSynchronize(st));
    mark("sums here");
    // 2. the verdicts, as the host API makes them
    for (size_t f = 0; f < n; ++f) mode[f] = sjpeg_hip_riskiness_verdict(&sums[f * 3], frames[f].width, frames[f].height, nullptr);
  }
  if (modes != nullptr) for (size_t f = 0; f < n; ++f) modes[f] = mode[f];
  // parts of consecutive frames whose sharp planes and workspace (and kept blocks, with the trellis) stay inside the
  // scratch limit (one frame at least)
  std::vector<std::pair<size_t, size_t>> parts;    // [first, end)
  size_t arena = 0;
  {
    size_t f0 = 0, bytes = 0, counted = 0;         // (counted: frames of the open part that take any of it)
    std::vector<sjpeg_hip_ragged_frame> sharp;
    auto kept_bytes = [&](size_t f) -> size_t {
      FrameGeo g;
      return frame_geo(frames[f].width, frames[f].height, hip_yuv_mode(mode[f]), &g) ? static_cast<size_t>(g.nseg) * kKeptSegBytes : 0;
    };
    auto close = [&](size_t end) {
      const size_t ws = sharp.empty() ? 0 : sjpeg_internal::sharp_ragged_workspace(static_cast<int>(sharp.size()), sharp.data());
      size_t planes = 0;
      for (const auto& fr : sharp) planes += planes_bytes(fr);
      arena = std::max(arena, align16(planes) + ws);
      parts.emplace_back(f0, end);
      sharp.clear();
      counted = 0;
    };
    for (size_t f = 0; f < n; ++f) {
      const bool is_sharp = mode[f] == kYuvSharp;
      if (!is_sharp && !trellis) continue;
      const size_t b = (is_sharp ? planes_bytes(frames[f]) + sjpeg_internal::sharp_ragged_workspace(1, &frames[f]) : 0) +
                       (trellis ? kept_bytes(f) : 0);
      if (counted > 0 && bytes + b > e->scratch_limit) { close(f); f0 = f; bytes = 0; }
      if (is_sharp) sharp.push_back(frames[f]);
      ++counted;
      bytes += b;
    }
    close(n);
  }
  if (arena > 0) {
    if (int rc = e->sharp_arena.ensure(arena / 16 + 1)) return rc;
  }
  for (const auto& part : parts) {
    // 3. the sharp frames of the part go into the arena: Y, U, V tightly packed, then the workspace
    std::vector<sjpeg_hip_ragged_frame> sharp, planar;
    std::vector<uint8_t*> yuv[3];
    for (size_t f = part.first; f < part.second; ++f) if (mode[f] == kYuvSharp) sharp.push_back(frames[f]);
    uint8_t* const ws = place_sharp_planes(reinterpret_cast<uint8_t*>(e->sharp_arena.p), sharp, &planar, yuv);
    // (enqueued by ragged_batch_groups in front of the first kernel that reads the sharp group, its last)
    auto convert = [&]() -> int {
      const size_t wsz = sjpeg_internal::sharp_ragged_workspace(static_cast<int>(sharp.size()), sharp.data());
      std::string err;
      if (int rc = sjpeg_internal::sharp_ragged_run(format, e->pscale, e->pbias, static_cast<int>(sharp.size()), sharp.data(), yuv[0].data(), yuv[1].data(),
                                                    yuv[2].data(), ws, wsz, st, engine_upload, e, &err)) {
        return fail(rc, who + ": " + err);
      }
      mark("sharp launched");
      return 0;
    };
    // 4. the mode groups: 4:2:0, 4:4:4, 4:0:0 of the caller's format, then the sharp frames as planar 4:2:0
    std::vector<RaggedGroup> groups;
    for (int kind : kGroupKinds) {
      RaggedGroup g;
      g.format = group_format(kind, format);
      g.yuv_mode = hip_yuv_mode(kind);
      for (size_t f = part.first; f < part.second; ++f) {
        if (mode[f] != kind) continue;
        g.frames.push_back(kind == kYuvSharp ? planar[g.frames.size()] : frames[f]);
        g.index.push_back(static_cast<int>(f));
      }
      if (g.frames.empty()) continue;
      if (int rc = ragged_format(who, g.format, g.yuv_mode, &g.a, &g.cls, &g.layout)) return rc;
      if (int rc = ragged_frames(who, g.format, g.yuv_mode, static_cast<int>(g.frames.size()), g.frames.data(), true, &g.geo)) return rc;
      groups.push_back(std::move(g));
    }
    if (int rc = ragged_batch_groups(e, who, groups, quant_in, quant_per_frame, min_quant, q_bias, method, qdelta_max_luma,
                                     qdelta_max_chroma, d_out, d_sizes, st,
                                     sharp.empty() ? std::function<int()>() : std::function<int()>(convert), sink)) return rc;
  }
  mark("call done");
  return 0;
}

// sjpeg_hip.h; the flow: ragged_modes_flow
static int ragged_auto_flow(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                            const sjpeg_hip_ragged_frame* frames, const uint8_t (*quant_in)[2][64],
                            int quant_per_frame, const uint8_t* min_quant, int q_bias, int method,
                            int qdelta_max_luma, int qdelta_max_chroma, void* d_out, uint64_t* d_sizes,
                            int* modes, void* stream, const sjpeg_internal::PackedSink* sink) {
  static const std::string who = "sjpeg_hip_encode_ragged_auto_src";
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (yuv_mode < kYuvAuto || yuv_mode > kYuv400) return fail(SJPEG_HIP_EINVAL, who + ": yuv_mode outside 0..4 (SjpegYUVMode)");
  if (yuv_mode != kYuvAuto && yuv_mode != kYuvSharp) {
    const int rc = sjpeg_internal::ragged_batch_flow(e, format, yuv_mode, nframes, frames, quant_in, quant_per_frame, min_quant,
                                                     q_bias, method, qdelta_max_luma, qdelta_max_chroma, d_out, d_sizes, stream, sink);
    if (rc == 0 && modes != nullptr) for (int f = 0; f < nframes; ++f) modes[f] = yuv_mode;
    return rc;
  }
  if (frames == nullptr || quant_in == nullptr || d_out == nullptr || d_sizes == nullptr) {
    return fail(SJPEG_HIP_EINVAL, who + ": frames, quant, d_out or d_sizes == NULL");
  }
  if (method < 0 || method > 6) return fail(SJPEG_HIP_EINVAL, who + ": methods 0..6 (trellis goes through the host API)");
  if (qdelta_max_luma < -12 || qdelta_max_luma > 12 || qdelta_max_chroma < -12 || qdelta_max_chroma > 12) {
    return fail(SJPEG_HIP_EINVAL, who + ": qdelta_max outside -12 .. 12");
  }
  try {
    if (int rc = rgb_ragged_frames(who, format, nframes, frames)) return rc;
    {
      std::vector<FrameGeo> geo;                   // (the output ranges)
      if (int rc = ragged_frames(who, format, SJPEG_HIP_YUV444, nframes, frames, true, &geo)) return rc;
    }
    return ragged_modes_flow(e, who, format, yuv_mode, nframes, frames, quant_in, quant_per_frame, min_quant, q_bias, method,
                             qdelta_max_luma, qdelta_max_chroma, d_out, d_sizes, modes, stream, sink);
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

int sjpeg_hip_encode_ragged_auto_src(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                     const sjpeg_hip_ragged_frame* frames, const uint8_t (*quant_in)[2][64],
                                     int quant_per_frame, const uint8_t* min_quant, int q_bias, int method,
                                     int qdelta_max_luma, int qdelta_max_chroma, void* d_out, uint64_t* d_sizes,
                                     int* modes, void* stream) {
  return ragged_auto_flow(e, format, yuv_mode, nframes, frames, quant_in, quant_per_frame, min_quant, q_bias, method,
                          qdelta_max_luma, qdelta_max_chroma, d_out, d_sizes, modes, stream, nullptr);
}

// Methods 7 and 8 over a ragged batch (sjpeg_hip.h): ragged_modes_flow with the trellis steps of ragged_batch_groups.
static int ragged_trellis_flow(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                               const sjpeg_hip_ragged_frame* frames, const uint8_t (*quant_in)[2][64],
                               int quant_per_frame, const uint8_t* min_quant, int q_bias, int method,
                               int qdelta_max_luma, int qdelta_max_chroma, void* d_out, uint64_t* d_sizes,
                               int* modes, void* stream, const sjpeg_internal::PackedSink* sink) {
  static const std::string who = "sjpeg_hip_encode_ragged_trellis_src";
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (yuv_mode < kYuvAuto || yuv_mode > kYuv400) return fail(SJPEG_HIP_EINVAL, who + ": yuv_mode outside 0..4 (SjpegYUVMode)");
  if (frames == nullptr || quant_in == nullptr || d_out == nullptr || d_sizes == nullptr) {
    return fail(SJPEG_HIP_EINVAL, who + ": frames, quant, d_out or d_sizes == NULL");
  }
  if (method != 7 && method != 8) return fail(SJPEG_HIP_EINVAL, who + ": methods 7 and 8 (the others: sjpeg_hip_encode_ragged_auto_src)");
  if (qdelta_max_luma < -12 || qdelta_max_luma > 12 || qdelta_max_chroma < -12 || qdelta_max_chroma > 12) {
    return fail(SJPEG_HIP_EINVAL, who + ": qdelta_max outside -12 .. 12");
  }
  try {
    if (yuv_mode == kYuvAuto || yuv_mode == kYuvSharp) {
      if (int rc = rgb_ragged_frames(who, format, nframes, frames)) return rc;
      std::vector<FrameGeo> geo;                   // (the output ranges)
      if (int rc = ragged_frames(who, format, SJPEG_HIP_YUV444, nframes, frames, true, &geo)) return rc;
    } else {
      if (nframes < 1 || nframes > 65535) return fail(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
      ScanArgs a;
      int cls = 0;
      const SourceLayout* layout = nullptr;
      std::vector<FrameGeo> geo;
      if (int rc = ragged_format(who, format, yuv_mode, &a, &cls, &layout)) return rc;
      if (int rc = ragged_frames(who, format, yuv_mode, nframes, frames, true, &geo)) return rc;
    }
    return ragged_modes_flow(e, who, format, yuv_mode, nframes, frames, quant_in, quant_per_frame, min_quant, q_bias, method,
                             qdelta_max_luma, qdelta_max_chroma, d_out, d_sizes, modes, stream, sink);
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

int sjpeg_hip_encode_ragged_trellis_src(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                        const sjpeg_hip_ragged_frame* frames, const uint8_t (*quant_in)[2][64],
                                        int quant_per_frame, const uint8_t* min_quant, int q_bias, int method,
                                        int qdelta_max_luma, int qdelta_max_chroma, void* d_out, uint64_t* d_sizes,
                                        int* modes, void* stream) {
  return ragged_trellis_flow(e, format, yuv_mode, nframes, frames, quant_in, quant_per_frame, min_quant, q_bias, method,
                             qdelta_max_luma, qdelta_max_chroma, d_out, d_sizes, modes, stream, nullptr);
}

// One packed buffer for every ragged flow (sjpeg_hip.h): the frames back to back, each at a multiple of 16 -- the format
// sjpeg_hip_gather_streams takes.  The flows are the unpacked entry points' (their checks, their messages); the sink
// (ragged_aux.h) goes down to ragged_encode, whose launches place their frames behind the engine's cursor.
int sjpeg_hip_encode_ragged_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                       const sjpeg_hip_ragged_params* params, void* d_packed, size_t packed_capacity,
                                       uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                       void* stream) {
  static const std::string who = "sjpeg_hip_encode_ragged_packed_src";
  // (every argument check of this function comes before `e` is touched: the tests without a GPU rely on it)
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (params == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": params == NULL");
  if (d_offsets == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": d_offsets == NULL");
  if (frames == nullptr || d_packed == nullptr || d_sizes == nullptr) {
    return fail(SJPEG_HIP_EINVAL, who + ": frames, d_packed or d_sizes == NULL");
  }
  if ((reinterpret_cast<uintptr_t>(d_packed) & 15u) != 0) return fail(SJPEG_HIP_EINVAL, who + ": d_packed must be a multiple of 16");
  if (packed_capacity >= SJPEG_HIP_PACKED_OVERFLOW) return fail(SJPEG_HIP_EINVAL, who + ": packed_capacity must be below 2^63");
  if (nframes < 1 || nframes > 65535) return fail(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
  try {
    std::vector<sjpeg_hip_ragged_frame> fr(frames, frames + nframes);
    for (sjpeg_hip_ragged_frame& f : fr) f.out_offset = 0;       // (ignored: the placement kernel says where a frame goes)
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = ragged_ordered(e, st)) return rc;
    if (int rc = e->pack_cursor.ensure(1)) return rc;
    HIP_TRY(hipMemsetAsync(e->pack_cursor.p, 0, sizeof(unsigned long long), st));
    const sjpeg_internal::PackedSink sink = {d_packed, packed_capacity, d_offsets, nframes, nullptr};
    const sjpeg_hip_ragged_params& p = *params;
    if (p.search != nullptr) {
      const int rc = sjpeg_internal::ragged_search_flow(e, format, p.yuv_mode, nframes, fr.data(), p.quant, p.quant_per_frame,
                                                        p.min_quant, p.q_bias, p.method, p.qdelta_max_luma, p.qdelta_max_chroma,
                                                        p.search, p.search_per_frame, q_out, value_out, d_packed, d_sizes, stream, &sink);
      if (rc == 0 && modes != nullptr) for (int f = 0; f < nframes; ++f) modes[f] = p.yuv_mode;
      return rc;
    }
    for (int f = 0; f < nframes; ++f) {
      if (q_out != nullptr) q_out[f] = -1.f;
      if (value_out != nullptr) value_out[f] = -1.f;
    }
    if (p.method == 7 || p.method == 8) {
      return ragged_trellis_flow(e, format, p.yuv_mode, nframes, fr.data(), p.quant, p.quant_per_frame, p.min_quant, p.q_bias,
                                 p.method, p.qdelta_max_luma, p.qdelta_max_chroma, d_packed, d_sizes, modes, stream, &sink);
    }
    return ragged_auto_flow(e, format, p.yuv_mode, nframes, fr.data(), p.quant, p.quant_per_frame, p.min_quant, p.q_bias,
                            p.method, p.qdelta_max_luma, p.qdelta_max_chroma, d_packed, d_sizes, modes, stream, &sink);
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

}  // extern "C"

// what the search (ragged_full.cc) takes from the flows above
int sjpeg_internal::ragged_unsearched_flow(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                           const sjpeg_hip_ragged_frame* frames, const uint8_t (*quant)[2][64], int quant_per_frame,
                                           const uint8_t* min_quant, int q_bias, int method, int qdelta_max_luma,
                                           int qdelta_max_chroma, void* d_out, uint64_t* d_sizes, int* modes, void* stream,
                                           const PackedSink* sink) {
  return (method == 7 || method == 8 ? ragged_trellis_flow : ragged_auto_flow)(e, format, yuv_mode, nframes, frames, quant, quant_per_frame,
                                                                              min_quant, q_bias, method, qdelta_max_luma,
                                                                              qdelta_max_chroma, d_out, d_sizes, modes, stream, sink);
}

int sjpeg_internal::ragged_groups_flow(sjpeg_hip_engine* e, const std::string& who, const std::vector<ModeGroup>& mode_groups,
                                       const uint8_t (*quant)[2][64], const uint8_t* min_quant, int q_bias, int method,
                                       int qdelta_max_luma, int qdelta_max_chroma, void* d_out, uint64_t* d_sizes, void* stream,
                                       const PackedSink* sink) {
  try {
    std::vector<RaggedGroup> groups;
    for (const ModeGroup& m : mode_groups) {
      if (m.frames.empty()) continue;
      RaggedGroup g;
      g.format = m.format; g.yuv_mode = m.yuv_mode; g.frames = m.frames; g.index = m.index;
      if (int rc = ragged_format(who, g.format, g.yuv_mode, &g.a, &g.cls, &g.layout)) return rc;
      if (int rc = ragged_frames(who, g.format, g.yuv_mode, static_cast<int>(g.frames.size()), g.frames.data(), true, &g.geo)) return rc;
      groups.push_back(std::move(g));
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = ragged_ordered(e, st)) return rc;
    return ragged_batch_groups(e, who, groups, quant, 1, min_quant, q_bias, method, qdelta_max_luma, qdelta_max_chroma, d_out,
                               d_sizes, st, {}, sink);
  } catch (...) {
    return fail(SJPEG_HIP_ENOMEM, "out of host memory");
  }
}

int sjpeg_internal::engine_pack_begin(sjpeg_hip_engine* e, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = ragged_ordered(e, st)) return rc;
  if (int rc = e->pack_cursor.ensure(1)) return rc;
  HIP_TRY(hipMemsetAsync(e->pack_cursor.p, 0, sizeof(unsigned long long), st));
  return 0;
}

// ---- ragged reduction and resize (reduce.hip, resize.hip): the engine's half.  The two share the engine's memory for
// the pictures they make and for their descriptors; `launch` starts the kernel over the uploaded descriptors.
template <class Frame>
static void picture_rebase(Frame& d, uint8_t* base) { d.dst = base + reinterpret_cast<uintptr_t>(d.dst); }
static void picture_rebase(sjpeg_internal::YuvPlane& p, uint8_t* base) {
  p.r.dst = base + reinterpret_cast<uintptr_t>(p.r.dst);
  if (p.channels == 2) p.dst2 = base + reinterpret_cast<uintptr_t>(p.dst2);
}

template <class Frame, class Launch>
static int engine_make_pictures(sjpeg_hip_engine* e, const std::string& who, const char* what, std::vector<Frame> desc, size_t bytes,
                                uint8_t* d_pictures, uint8_t** base, void* stream, Launch launch) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = ragged_ordered(e, st)) return rc;
  if (d_pictures == nullptr) {
    if (e->reduced.ensure(bytes / 16 + 1) != 0) {
      return fail(SJPEG_HIP_ENOMEM, who + ": no device memory for " + std::to_string(bytes) + " bytes of " + what + " pictures");
    }
    d_pictures = reinterpret_cast<uint8_t*>(e->reduced.p);
  }
  if (base != nullptr) *base = d_pictures;
  for (Frame& d : desc) picture_rebase(d, d_pictures);
  const size_t desc_bytes = sizeof(Frame) * desc.size();
  if (int rc = e->reduce_desc.ensure(desc_bytes / 16 + 1)) return rc;
  if (int rc = upload(e, e->reduce_desc.p, desc.data(), desc_bytes, st)) return rc;
  if (int rc = sync_uploads(e, st)) return rc;
  return launch(reinterpret_cast<const Frame*>(e->reduce_desc.p), static_cast<int>(desc.size()), st);
}

int sjpeg_internal::engine_reduce(sjpeg_hip_engine* e, const std::string& who, const ReducePlan& plan, uint8_t* d_reduced, uint8_t** base,
                                  void* stream) {
  return engine_make_pictures(e, who, "reduced", plan.frames, plan.bytes, d_reduced, base, stream,
                              [&](const ReduceFrame* d_frames, int n, hipStream_t st) {
    if (reduce_ragged_launch(plan.format, e->pscale, e->pbias, d_frames, n, plan.tiles, st) != 0) {
      return fail(SJPEG_HIP_ERUNTIME, who + ": reduce_ragged_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
    }
    return 0;
  });
}

int sjpeg_internal::engine_resize(sjpeg_hip_engine* e, const std::string& who, const ResizePlan& plan, uint8_t* d_resized, uint8_t** base,
                                  void* stream) {
  return engine_make_pictures(e, who, "resized", plan.frames, plan.bytes, d_resized, base, stream,
                              [&](const ResizeFrame* d_frames, int n, hipStream_t st) {
    const int rc = plan.flat ? resize_ragged_flat_launch(false, plan.format, e->pscale, e->pbias, plan.flatten, d_frames, n, plan.tiles, st)
                             : resize_ragged_launch(plan.format, e->pscale, e->pbias, d_frames, n, plan.tiles, st);
    if (rc != 0) {
      return fail(SJPEG_HIP_ERUNTIME, who + ": resize_ragged_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
    }
    return 0;
  });
}

// ... and of the YUV-plane formats: a descriptor per plane, the kernel's other instantiation
int sjpeg_internal::engine_yuv_resize(sjpeg_hip_engine* e, const std::string& who, const YuvResizePlan& plan, uint8_t* d_out, uint8_t** base,
                                      void* stream) {
  return engine_make_pictures(e, who, "resized", plan.planes, plan.bytes, d_out, base, stream,
                              [&](const YuvPlane* d_planes, int n, hipStream_t st) {
    if ((plan.deep ? yuv_resize_ragged_deep_launch(false, plan.shift, d_planes, n, plan.tiles, st)
                   : yuv_resize_ragged_launch(d_planes, n, plan.tiles, st)) != 0) {
      return fail(SJPEG_HIP_ERUNTIME, who + ": resize_ragged_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
    }
    return 0;
  });
}

// ... and of the contact sheets (sheet_plan.cc): the background of every sheet, then the placed descriptors of either
// plan, both on the call's stream -- stream order is the only ordering relied on
int sjpeg_internal::engine_sheet(sjpeg_hip_engine* e, const std::string& who, const SheetPlan& plan, uint8_t* d_out, uint8_t** base,
                                 void* stream) {
  uint8_t* sheets = nullptr;
  auto fill = [&](hipStream_t st) {
    if (sheet_fill_launch(plan.fill, sheets, st) != 0) {
      return fail(SJPEG_HIP_ERUNTIME, who + ": sheet_fill_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
    }
    return 0;
  };
  int rc;
  if (plan.yuv) {
    rc = engine_make_pictures(e, who, "sheet", plan.planes.planes, plan.bytes, d_out, &sheets, stream,
                              [&](const YuvPlane* d_planes, int n, hipStream_t st) {
      if (int rcf = fill(st)) return rcf;
      if ((plan.planes.deep ? yuv_resize_ragged_deep_launch(true, plan.planes.shift, d_planes, n, plan.planes.tiles, st)
                            : yuv_resize_ragged_placed_launch(d_planes, n, plan.planes.tiles, st)) != 0) {
        return fail(SJPEG_HIP_ERUNTIME, who + ": resize_ragged_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
      }
      return 0;
    });
  } else {
    rc = engine_make_pictures(e, who, "sheet", plan.rgb.frames, plan.bytes, d_out, &sheets, stream,
                              [&](const ResizeFrame* d_frames, int n, hipStream_t st) {
      if (int rcf = fill(st)) return rcf;
      const int rcl = plan.rgb.flat ? resize_ragged_flat_launch(true, plan.format, e->pscale, e->pbias, plan.rgb.flatten, d_frames, n, plan.rgb.tiles, st)
                                    : resize_ragged_placed_launch(plan.format, e->pscale, e->pbias, d_frames, n, plan.rgb.tiles, st);
      if (rcl != 0) {
        return fail(SJPEG_HIP_ERUNTIME, who + ": resize_ragged_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
      }
      return 0;
    });
  }
  if (base != nullptr) *base = sheets;
  return rc;
}

// ... and of the video colour conversion (yuv_colour_plan.cc): the launch behind the resize launch of the same call, on
// the same stream, over the planes that one made at `base`
int sjpeg_internal::engine_yuv_colour(sjpeg_hip_engine* e, const std::string& who, const YuvColourPlan& plan, uint8_t* base, void* stream) {
  if (plan.tiles == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::vector<YuvColourFrame> desc = plan.frames;
  for (YuvColourFrame& d : desc) {
    d.y = base + reinterpret_cast<uintptr_t>(d.y);
    d.u = base + reinterpret_cast<uintptr_t>(d.u);
    d.v = base + reinterpret_cast<uintptr_t>(d.v);
  }
  const size_t desc_bytes = sizeof(YuvColourFrame) * desc.size();
  if (int rc = e->colour_desc.ensure(desc_bytes / 16 + 1)) return rc;
  if (int rc = upload(e, e->colour_desc.p, desc.data(), desc_bytes, st)) return rc;
  if (int rc = sync_uploads(e, st)) return rc;
  if (yuv_colour_launch(plan.placed, reinterpret_cast<const YuvColourFrame*>(e->colour_desc.p), static_cast<int>(desc.size()), plan.tiles, st) != 0) {
    return fail(SJPEG_HIP_ERUNTIME, who + ": yuv_colour_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
  }
  return 0;
}

extern "C" {

// ---- exchange step of the multi-device batch path: the coded frames of one call, back to back ----
// (BASELINE.json config #4; the reference is single-threaded and has no counterpart.)  One
// launch, no host round trip: every workgroup sums the (16-byte aligned) sizes of the frames in
// front of its own and copies 16 bytes per thread.

__global__ __launch_bounds__(256) void compact_streams_kernel(const uint8_t* out, size_t out_stride, const unsigned long long* sizes,
                                                              int nframes, uint8_t* packed, unsigned long long capacity,
                                                              unsigned long long* offsets) {
  const int f = blockIdx.y, tid = threadIdx.x;
  __shared__ unsigned long long part[4];
  unsigned long long s = 0;
  for (int g = tid; g < f; g += 256) s += (sizes[g] + 15ull) & ~15ull;
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  const unsigned long long off = part[0] + part[1] + part[2] + part[3];
  const unsigned long long n = sizes[f], n16 = (n + 15ull) & ~15ull;
  if (blockIdx.x == 0 && tid == 0) {
    offsets[f] = off;
    // bytes needed, whether they fit or not; bit 63 says they did not (SJPEG_HIP_PACKED_OVERFLOW: the exchange
    // reads it in the rank's row and refuses on every rank)
    if (f == nframes - 1) offsets[nframes] = (off + n16) | (off + n16 > capacity ? (1ull << 63) : 0ull);
  }
  if (off + n16 > capacity) return;                            // the caller sees it in offsets[nframes]
  const uint4* const src = reinterpret_cast<const uint4*>(out + static_cast<size_t>(f) * out_stride);
  uint4* const dst = reinterpret_cast<uint4*>(packed + off);
  const size_t nch = static_cast<size_t>(n16 >> 4);
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + tid; i < nch; i += static_cast<size_t>(gridDim.x) * 256) {
    uint4 v = src[i];
    if (i == nch - 1 && (n & 15ull) != 0ull) {                 // zero the padding behind the last byte
      uint32_t w[4] = {v.x, v.y, v.z, v.w};
      const uint32_t keep = static_cast<uint32_t>(n & 15ull);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t lo = 4u * k;
        w[k] = keep <= lo ? 0u : (keep >= lo + 4u ? w[k] : (w[k] & ((1u << (8u * (keep - lo))) - 1u)));
      }
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    dst[i] = v;
  }
}

int sjpeg_hip_compact_streams(const void* d_out, size_t out_stride, const uint64_t* d_sizes, int nframes,
                              void* d_packed, size_t packed_capacity, uint64_t* d_offsets, void* stream) {
  if (d_out == nullptr || d_sizes == nullptr || d_packed == nullptr || d_offsets == nullptr) {
    return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_compact_streams: NULL argument");
  }
  if (nframes <= 0 || nframes > 65535) return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_compact_streams: nframes must be 1 .. 65535");
  if ((reinterpret_cast<uintptr_t>(d_out) & 15u) != 0 || (reinterpret_cast<uintptr_t>(d_packed) & 15u) != 0 || (out_stride & 15u) != 0) {
    return fail(SJPEG_HIP_EINVAL, "sjpeg_hip_compact_streams: d_out, d_packed and out_stride must be multiples of 16");
  }
  hipLaunchKernelGGL(compact_streams_kernel, dim3(64, nframes), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(d_out), out_stride, reinterpret_cast<const unsigned long long*>(d_sizes), nframes,
                     static_cast<uint8_t*>(d_packed), static_cast<unsigned long long>(packed_capacity),
                     reinterpret_cast<unsigned long long*>(d_offsets));
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- measurement aid: what a read-only streaming kernel reaches on this device ------------------
// (SURVEY section 8d asks for the achieved read bandwidth beside the 8 TB/s spec figure)

__global__ __launch_bounds__(256) void stream_read_kernel(const uint4* p, size_t n, uint32_t* sink) {
  uint4 acc = make_uint4(0, 0, 0, 0);
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * 256) {
    const uint4 v = p[i];
    acc.x ^= v.x; acc.y ^= v.y; acc.z ^= v.z; acc.w ^= v.w;
  }
  const uint32_t r = acc.x ^ acc.y ^ acc.z ^ acc.w;
  if (r == 0x9e3779b9u) sink[0] = r;               // keeps the loads alive, practically never taken
}

int sjpeg_hip_debug_stream_read(const void* d_buf, size_t bytes, uint32_t* d_sink, void* stream) {
  if (d_buf == nullptr || d_sink == nullptr || bytes < 16) return SJPEG_HIP_EINVAL;
  hipLaunchKernelGGL(stream_read_kernel, dim3(256 * 16), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint4*>(d_buf), bytes / 16, d_sink);
  return hipGetLastError() == hipSuccess ? 0 : SJPEG_HIP_ERUNTIME;
}

// ---- measurement aid: cycles a wave64 VALU instruction occupies a SIMD, per issue class -----------
// (the second roofline of K1, bench.py `roofline.valu`; tools/valu_rate.hip has the table of all ops)

#define SJPEG_VALU_RATE_KERNEL(NAME, ASM)                                                              \
__global__ __launch_bounds__(256) void NAME(uint32_t a, uint32_t b, uint32_t* sink) {                  \
  uint32_t r[8];                                                                                       \
  _Pragma("unroll") for (int i = 0; i < 8; ++i) r[i] = threadIdx.x * 2654435761u + i * 40503u + a;      \
  for (int it = 0; it < 1024; ++it) {                                                                  \
    _Pragma("unroll") for (int u = 0; u < 32; ++u) asm volatile(ASM : "+v"(r[u & 7]) : "v"(a), "v"(b)); \
  }                                                                                                    \
  uint32_t x = 0;                                                                                      \
  _Pragma("unroll") for (int i = 0; i < 8; ++i) x ^= r[i];                                             \
  if (x == 0x12345u) sink[0] = 1;                                                                      \
}
SJPEG_VALU_RATE_KERNEL(valu_rate_kernel_slow, "v_perm_b32 %0, %0, %1, %2")
SJPEG_VALU_RATE_KERNEL(valu_rate_kernel_fast, "v_add_u32 %0, %0, %1")

// The shader clock as the shaders see it: a wave spins for `ticks` ticks of the device-wide 100 MHz counter and
// counts the cycles of the shader-clock counter meanwhile.  Enqueued on the stream of the work it is to describe,
// it runs right behind that work, before the clocks have come down (sysfs / rocm-smi show ~100 MHz the moment the
// queue is empty, and lag behind when it is not).
__global__ void clock_probe_kernel(unsigned long long* out, unsigned long long ticks) {
  if (threadIdx.x != 0) return;
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_readcyclecounter();
  unsigned long long r1 = r0;
  while (r1 - r0 < ticks) { __builtin_amdgcn_s_sleep(8); r1 = __builtin_amdgcn_s_memrealtime(); }
  const unsigned long long c1 = __builtin_readcyclecounter();
  out[0] = c1 - c0;
  out[1] = r1 - r0;
}

int sjpeg_hip_debug_shader_clock(float* mhz, void* stream) {
  if (mhz == nullptr) return SJPEG_HIP_EINVAL;
  unsigned long long* d = nullptr;
  unsigned long long h[2] = {0, 0};
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), sizeof(h)));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, st, d, 2000ull);      // 20 us
  const hipError_t e0 = hipGetLastError();
  const hipError_t e1 = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);
  (void)hipFree(d);
  if (e0 != hipSuccess || e1 != hipSuccess || e2 != hipSuccess || h[1] == 0) return SJPEG_HIP_ERUNTIME;
  *mhz = static_cast<float>(static_cast<double>(h[0]) / static_cast<double>(h[1]) * 100.0);
  return 0;
}

int sjpeg_hip_debug_valu_rate(float cycles[2], void* stream) {
  if (cycles == nullptr) return SJPEG_HIP_EINVAL;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  uint32_t* d_sink = nullptr;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_sink), 64));
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int wps = 8;                               // workgroups per CU = waves per SIMD (256 threads each)
  const dim3 grid(prop.multiProcessorCount * wps);
  for (int c = 0; c < 2; ++c) {
    for (int rep = 0; rep < 2; ++rep) {            // first launch warms up
      (void)hipEventRecord(e0, st);
      if (c == 0) hipLaunchKernelGGL(valu_rate_kernel_slow, grid, dim3(256), 0, st, 3u, 5u, d_sink);
      else hipLaunchKernelGGL(valu_rate_kernel_fast, grid, dim3(256), 0, st, 3u, 5u, d_sink);
      (void)hipEventRecord(e1, st);
      (void)hipEventSynchronize(e1);
    }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    cycles[c] = ms * 1e-3f * 2.4e9f / (1024.0f * 32.0f * wps);   // at the nominal 2.4 GHz
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(d_sink);
  return hipGetLastError() == hipSuccess ? 0 : SJPEG_HIP_ERUNTIME;
}

}  // extern "C"
