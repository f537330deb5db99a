// batch_flow.cc -- sjpeg_hip_encode_batch_src: a batch of frames of one size with the reference's per-picture analysis,
// over the engine's uniform entries (engine.h, sjpeg_hip.h): the five steps of a frame range, and the two schedules that
// run them -- lanes (jobs on up to four streams) and parts.  Host only: every kernel is launched by the unit that defines it.
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "batch_flow.h"
#include "engine.h"

using namespace sjpeg_internal;

// ---- a whole batch with the reference's per-picture analysis (methods 0..6), device-resident ----
// What Encoder::Encode does for ONE picture with adaptive quantization and optimised Huffman
// codes (src/enc.cc:391-448: CollectHistograms + AnalyseHisto, the statistics half of
// SinglePassScanOptimized, headers, the scan), done for nframes pictures with one launch per
// device pass and the per-picture float / Huffman work on the host in between.
// (a frame's share of the batch scratch -- kHist, kSums, kTot, kFreq: ragged_aux.h)
BatchScratch& sjpeg_internal::batch_scratch() {
  static thread_local BatchScratch scratch;
  return scratch;
}

void sjpeg_internal::adopt_matrices(const uint8_t* h_q, size_t f0, size_t nf, int yuv_mode, const uint8_t* min_quant, int q_bias,
                    uint8_t* quant, sjpeg_hip_scan_tables* tables) {
  const size_t ntab = yuv_mode == SJPEG_HIP_YUV400 ? 1 : 2;
  for (size_t f = f0; f < f0 + nf; ++f) {
    memcpy(&quant[f * 128], h_q + f * 128, ntab * 64);
    sjpeg_hip_finalize_quant(reinterpret_cast<uint8_t(*)[64]>(&quant[f * 128]), min_quant, q_bias, &tables[f]);
  }
}

int sjpeg_internal::batch_headers(const std::string& who, const std::function<std::pair<int, int>(size_t)>& dims, size_t f0, size_t nf, int yuv_mode, const uint8_t* quant,
                  const sjpeg_hip_huffman_spec* specs, std::vector<uint8_t>* headers, std::vector<size_t>* offs,
                  const std::function<const FrameMeta*(size_t)>& meta) {
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

namespace {

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

extern "C" int sjpeg_hip_encode_batch_src(sjpeg_hip_engine* engine, const sjpeg_hip_source* src,
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
    BatchScratch& sc = batch_scratch();
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
