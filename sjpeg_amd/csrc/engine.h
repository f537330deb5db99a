// engine.h -- the engine object behind include/sjpeg_hip.h and the launch layer of scan_engine.hip, for the files that
// drive it: the batch flows (batch_flow.cc, ragged_flows.cc), the picture-making halves (engine_pictures.cc) and the
// probes.  Internal, not installed.  ragged_aux.h stays the facade for the files that do not need the struct.
//
// Two rules.  A kernel is launched only from the unit that defines it: what a flow needs of a kernel is a host function
// here.  The kernels' parameter structs (ScanArgs, StitchArgs, PackArgs, the device RaggedFrame) stay in the scan headers,
// in scan_engine.hip's anonymous namespace: the flows name a source FORMAT, the launch layer derives the rest.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <string>
#include <vector>

#include "ragged_aux.h"
#include "sjpeg_hip.h"

namespace sjpeg_internal {

// sjpeg_hip_last_error() of the calling thread; returns code
inline int fail(int code, const std::string& msg) { return set_error(code, msg); }

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    const hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess) {                                                             \
      return ::sjpeg_internal::fail(e_ == hipErrorOutOfMemory ? SJPEG_HIP_ENOMEM : SJPEG_HIP_ERUNTIME, \
                                    std::string(#expr) + ": " + hipGetErrorString(e_)); \
    }                                                                                   \
  } while (0)

struct FrameGeo {
  int bpm, px, seg_mcus, mb_w, mb_h, n_mcus, nseg;
  uint32_t slot_words;
};

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

// device copy of sjpeg_hip_scan_tables, pre-digested
// Laid out as the kernels stage it: two contiguous groups copied to LDS 16 bytes per thread (scan_device.h asserts the
// sizes).  The kernels reach it through a pointer in their arguments; the engine holds the copies it uploaded last.
struct alignas(16) DevTables {
  // group A (1152 B, lives in the idle bit window until the DC codes are done)
  uint4 q[2][32];          // per natural-order PAIR (2j, 2j+1): {iq0 | iq1<<16, bias0*iq0, bias1*iq1, q0 | q1<<16}
  uint32_t dc[2][12];
  // bits a block's AC entries (sign-magnitude pairs) must NOT have for the lean walk to be provably
  // in place: levels of n <= n_safe bits, n_safe = largest n with len(0, n') + n' <= 16 for all n' <= n
  uint32_t safe_mask[2];
  // the AC code words the lean walk needs beside the merged ones: {EOB, ZRL} per table ((code << 16) | length)
  uint32_t eob_zrl[2][2];
  uint32_t pad_a[2];
  // group B (3456 B)
  uint32_t ac[2][256];
  // Lean entropy walk, indexed [run & 15][clz(level) - 22] (level 1..1023 <=> clz 31..22):
  // (code << n) | (code length + n) << 27, i.e. everything of a run/size symbol but the n suffix
  // bits, in one word.  Run-major: the symbols a picture is made of (runs 0..3, 1..7 level bits) are
  // 28 words in a row, one LDS bank each -- size-major (rows of 16 runs) they shared eight banks.
  uint32_t acm[2][16][10];
  // 1, 2 or 3 ZRL codes as a left-aligned 64-bit pattern {high word, low word, bits, 0} (index 0 unused):
  // what the stitch puts in front of a part whose first run is 16 or longer
  uint4 zrlpat[2][4];
  uint8_t tlen[2][256];    // trellis quantization: AC code lengths the rate is priced with
};

}  // namespace sjpeg_internal

struct sjpeg_hip_engine {
  template <typename T> using DevBuf = sjpeg_internal::DevBuf<T>;
  using DevTables = sjpeg_internal::DevTables;
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
  // ... and the unsharp launch behind either (unsharp.hip), which works out of place: the FINAL pictures of an encode
  // entry -- the made ones stay in `reduced` while it reads them -- and its descriptors, again buffers of their own
  DevBuf<uint4> final_pictures, unsharp_desc;
  // ... and the tables of a resampling call (resample.hip): bounds and coefficients of every axis, once per key
  DevBuf<uint4> resample_tables;
  // ... and of Pillow's filters behind the box entries (pillow_filter.hip): the bytes between the launch along the rows
  // and the one along the columns, in the made pictures' layout, and the two launches' descriptors
  DevBuf<uint4> filter_mid, filter_desc;
  // ... and of the compose stage behind any of them (compose.hip): the canvases where the caller gave no buffer -- memory
  // of their own, so that the launch is out of place whatever made the pictures -- and the launch's descriptors
  DevBuf<uint4> composed, compose_desc;
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

// ---- the launch layer (scan_engine.hip) as the flows see it
namespace sjpeg_internal {

// false for a size or yuv_mode the engine does not take; else the frame's MCU and segment counts
bool frame_geo(int W, int H, int mode, FrameGeo* g);

// the event behind everything the engine has put on its own (stitch) stream so far
int side_mark(sjpeg_hip_engine* e);
// Orders this call after everything the engine was asked to do on another stream.
int order_on_stream(sjpeg_hip_engine* e, hipStream_t st);
// ... on the engine's device, and behind pipelined mode's stitch stream as well: what every ragged call starts with
int ragged_ordered(sjpeg_hip_engine* e, hipStream_t st);
// bytes between two places the DEVICE can address (device memory, mapped pinned host memory), by a kernel; the
// runtime's copy where the addresses do not allow 16-byte accesses
int copy_by_kernel(void* dst, const void* src, size_t bytes, hipStream_t st, hipMemcpyKind fallback_kind, const void* fallback_src, void* fallback_dst);
// dst <- src on the stream, through one of the engine's pinned blocks when the copy is not tiny (sjpeg_hip_engine::stage)
int upload(sjpeg_hip_engine* e, void* dst, const void* src, size_t bytes, hipStream_t st);
// the call's stream waits for the early uploads (sjpeg_hip_engine::up_stream) in front of the kernel that reads them
int sync_uploads(sjpeg_hip_engine* e, hipStream_t st);

// The checks of a ragged call's source format and yuv_mode.  who: the entry point, for the messages.
int ragged_format(const std::string& who, int format, int yuv_mode);
// Every frame of a ragged call of a known format checked (the message names the frame); its geometry into (*geo)[f].
// out_ranges: the frames' output ranges are checked too (the encodes; the analysis passes ignore them).
int ragged_frames(const std::string& who, int format, int yuv_mode, int nframes,
                  const sjpeg_hip_ragged_frame* frames, bool out_ranges, std::vector<FrameGeo>* geo, int esz = 0);
// The ragged encode of frames checked by the two above: K1 .. K5 (what d_bits, kept and sink change: scan_engine.hip)
int ragged_encode(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                  const sjpeg_hip_ragged_frame* frames, const std::vector<FrameGeo>& geo,
                  const sjpeg_hip_scan_tables* tables, int tables_per_frame, const void* headers,
                  const size_t* header_offsets, size_t header_size, int append_eoi, void* d_out, uint64_t* d_sizes,
                  hipStream_t st, unsigned long long* d_bits, uint32_t* kept = nullptr,
                  const PackedSink* sink = nullptr, const uint32_t* kept_base = nullptr);
// ... and the analysis passes over them, each with its ragged reduce
enum RaggedPass { kPassHisto, kPassStats, kPassError, kPassStatsTrellis };
int ragged_analysis(sjpeg_hip_engine* e, RaggedPass pass, int format, int yuv_mode, int nframes,
                    const sjpeg_hip_ragged_frame* frames, const std::vector<FrameGeo>& geo,
                    const sjpeg_hip_scan_tables* tables, int tables_per_frame, uint32_t* d_out, hipStream_t st,
                    uint32_t* kept = nullptr, const uint32_t* kept_base = nullptr);

// adapt_decide_kernel behind sjpeg_hip_adapt_sums on the same stream: d_quant_out[nframes][2][64]
int adapt_decide(const int64_t* d_sums, const int32_t* d_totlast, int nframes, const uint8_t quant[2][64], int ntables,
                 int qdelta_max_luma, int qdelta_max_chroma, uint8_t* d_quant_out, hipStream_t st);
// out[index[i]] = sizes[i], i < n: the sizes of a call's mode groups back in the caller's order
int scatter_sizes(const unsigned long long* d_sizes, const uint32_t* d_index, int n, unsigned long long* d_out, hipStream_t st);

}  // namespace sjpeg_internal
