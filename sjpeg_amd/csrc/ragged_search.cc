// ragged_search.cc -- sjpeg_hip_encode_ragged_search_src: the reference's multi-pass search (Encoder::LoopScan,
// src/dichotomy.cc:113-205) over a ragged batch.  The host API runs it one picture at a time (host_api.cc,
// Encoder::Run); here every pass is one launch over the frames still searching and one wait for what it measured.
// Per frame, one sjpeg::SearchHook does the float arithmetic of the search (Setup / NextMatrix / Update); the
// measurements are the ones the host API prices a pass with (jpeg_host.h: SearchHeaderBits, EntropyBits, SearchPSNR).
// The device passes are the engine's ragged ones: histogram (kept for the whole search), adaptation, symbol
// statistics, counted bits, quantization error.  DESIGN.md section 4.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "jpeg_host.h"
#include "ragged_aux.h"
#include "sjpeg.h"
#include "sjpeg_hip.h"

namespace {

using sjpeg_internal::set_error;

constexpr size_t kHist = 2 * 64 * 128 * sizeof(uint32_t);      // a frame's kept histogram
constexpr size_t kFreq = 2 * 272 * sizeof(uint32_t);            // a frame's symbol counts
constexpr size_t kStatsPartial = 2 * 272 * sizeof(uint32_t);    // a segment's partial of the statistics pass
// a frame's adaptation sums and totals (adapt_sums_kernel: [2][64][deltas][2] int64, [2][64][2] int32)
constexpr size_t kAdaptSumsBytes = 2 * 64 * sjpeg_host::kAdaptDeltas * 2 * sizeof(int64_t);
constexpr size_t kAdaptTotBytes = 2 * 64 * 2 * sizeof(int32_t);

// device scratch of the calling thread, kept between calls
struct SearchScratch {
  int device = -1;
  void* p = nullptr;
  size_t cap = 0;
  bool Ensure(int dev, size_t need) {
    if (dev != device && p != nullptr) { (void)hipSetDevice(device); (void)hipFree(p); p = nullptr; cap = 0; }
    device = dev;
    (void)hipSetDevice(dev);
    if (need <= cap) return true;
    if (p != nullptr) (void)hipFree(p);
    p = nullptr; cap = 0;
    if (hipMalloc(&p, need) != hipSuccess) { (void)hipGetLastError(); return false; }
    cap = need;
    return true;
  }
  ~SearchScratch() { if (p != nullptr) { (void)hipSetDevice(device); (void)hipFree(p); } }
};
thread_local SearchScratch g_search;

// one searched frame: its hook and the loop state of Encoder::LoopScan
struct FrameSearch {
  int index = 0;                       // the caller's frame
  int passes = 1;
  sjpeg::SearchHook hook;
  uint8_t quant[2][64];                // the pass's matrices (after adaptation)
  uint8_t opt[2][64];                  // the best pass' matrices
  float best = 0.f, best_q = 0.f, best_result = 0.f;
  bool done = false;
};

int hip_fail(const std::string& who, const char* what) {
  const hipError_t err = hipGetLastError();
  return set_error(err == hipErrorOutOfMemory ? SJPEG_HIP_ENOMEM : SJPEG_HIP_ERUNTIME,
                   who + ": " + what + ": " + hipGetErrorString(err));
}

int read_back(const std::string& who, void* h, const void* d, size_t bytes, hipStream_t st) {
  if (hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    return hip_fail(who, "read-back");
  }
  return 0;
}

// d_sizes of a sub-call land in the caller's d_sizes: runs of consecutive caller frames go in one copy
int scatter_sizes(const std::string& who, const uint64_t* d_from, const std::vector<int>& index, uint64_t* d_sizes,
                  hipStream_t st) {
  for (size_t k = 0; k < index.size();) {
    size_t n = 1;
    while (k + n < index.size() && index[k + n] == index[k] + static_cast<int>(n)) ++n;
    if (hipMemcpyAsync(d_sizes + index[k], d_from + k, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, st) != hipSuccess) {
      return hip_fail(who, "sizes");
    }
    k += n;
  }
  return 0;
}

// The search of frames fr[0, n) (consecutive caller frames, all searched): the passes, then s[k].opt and the hooks' q
// and value hold the result.  d_scratch: kept histograms [n][kHist] | matrices in [n][128] | adapted [n][128] | sums
// [n] | totals [n] | measurements [n][kFreq].
int search_part(sjpeg_hip_engine* e, const std::string& who, int format, int yuv_mode, const sjpeg_hip_ragged_frame* fr,
                FrameSearch* s, int n, const uint8_t* min_quant, int q_bias, int method, int qdelta_max_luma,
                int qdelta_max_chroma, uint8_t* d_scratch, hipStream_t st) {
  const bool adaptive = method >= 3, optimize = method != 0 && method != 3;
  const int ntab = yuv_mode == SJPEG_HIP_YUV400 ? 1 : 2;
  const int nb_comps = yuv_mode == SJPEG_HIP_YUV400 ? 1 : 3;
  uint32_t* const d_hist = reinterpret_cast<uint32_t*>(d_scratch);
  uint8_t* const d_qin = d_scratch + (adaptive ? n * kHist : 0);
  uint8_t* const d_qout = d_qin + n * 128;
  int64_t* const d_sums = reinterpret_cast<int64_t*>(d_qout + n * 128);
  int32_t* const d_tot = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(d_sums) + n * kAdaptSumsBytes);
  uint8_t* const d_meas = reinterpret_cast<uint8_t*>(d_tot) + n * kAdaptTotBytes;
  if (adaptive) {
    if (int rc = sjpeg_hip_scan_histogram_ragged_src(e, format, yuv_mode, n, fr, d_hist, st)) return rc;
  }
  int max_passes = 0;
  for (int k = 0; k < n; ++k) max_passes = std::max(max_passes, s[k].passes);
  std::vector<uint8_t> h_q(static_cast<size_t>(n) * 128);
  std::vector<uint8_t> h_meas(static_cast<size_t>(n) * kFreq);
  std::vector<sjpeg_hip_scan_tables> tables(n);
  std::vector<sjpeg_hip_ragged_frame> afr;
  std::vector<sjpeg_hip_scan_tables> atab;
  std::vector<int> active;
  for (int p = 0; p < max_passes; ++p) {
    active.clear();
    for (int k = 0; k < n; ++k) if (!s[k].done && p < s[k].passes) active.push_back(k);
    if (active.empty()) break;
    // the pass's matrices: NextMatrix, clamped to min_quant (FinalizeQuantMatrix)
    for (int k : active) {
      s[k].hook.pass = p;
      for (int c = 0; c < 2; ++c) s[k].hook.NextMatrix(c, s[k].quant[c]);
      memset(&tables[k], 0, sizeof(tables[k]));
      sjpeg_hip_finalize_quant(s[k].quant, min_quant, q_bias, &tables[k]);
    }
    if (adaptive) {
      // AnalyseHisto of the kept histograms with these matrices: one launch per run of consecutive active frames
      for (int k : active) memcpy(&h_q[static_cast<size_t>(k) * 128], s[k].quant, 128);
      if (hipMemcpyAsync(d_qin, h_q.data(), h_q.size(), hipMemcpyHostToDevice, st) != hipSuccess) return hip_fail(who, "matrices");
      for (size_t i = 0; i < active.size();) {
        size_t m = 1;
        while (i + m < active.size() && active[i + m] == active[i] + static_cast<int>(m)) ++m;
        const size_t k0 = active[i];
        if (int rc = sjpeg_internal::adapt_ragged(d_hist + k0 * (kHist / 4), d_qin + k0 * 128, static_cast<int>(m), min_quant, ntab,
                                                  qdelta_max_luma, qdelta_max_chroma, d_sums + k0 * (kAdaptSumsBytes / 8),
                                                  d_tot + k0 * (kAdaptTotBytes / 4), d_qout + k0 * 128, st)) {
          return rc;
        }
        i += m;
      }
      if (int rc = read_back(who, h_q.data(), d_qout, h_q.size(), st)) return rc;          // (wait 1: the matrices)
      for (int k : active) {
        memcpy(s[k].quant, &h_q[static_cast<size_t>(k) * 128], static_cast<size_t>(ntab) * 64);
        sjpeg_hip_finalize_quant(s[k].quant, min_quant, q_bias, &tables[k]);
      }
    }
    // the measurement of every active frame, one launch
    const bool for_size = s[active[0]].hook.for_size;          // (one target mode per call part: see the caller)
    afr.clear(); atab.clear();
    for (int k : active) { afr.push_back(fr[k]); atab.push_back(tables[k]); }
    const int na = static_cast<int>(active.size());
    if (for_size) {
      for (sjpeg_hip_scan_tables& t : atab) sjpeg_hip_default_huffman(&t);
      if (optimize) {
        if (int rc = sjpeg_hip_scan_symbol_stats_ragged_src(e, format, yuv_mode, na, afr.data(), atab.data(), 1,
                                                            reinterpret_cast<uint32_t*>(d_meas), st)) {
          return rc;
        }
        if (int rc = read_back(who, h_meas.data(), d_meas, na * kFreq, st)) return rc;
      } else {
        uint64_t* const d_bits = reinterpret_cast<uint64_t*>(d_meas);
        if (int rc = sjpeg_internal::counted_bits_first(e, format, yuv_mode, na, afr.data(), atab.data(), 1, d_bits, st)) return rc;
        if (int rc = read_back(who, h_meas.data(), d_meas, na * sizeof(uint64_t), st)) return rc;
        std::vector<int> again;
        for (int i = 0; i < na; ++i) if (reinterpret_cast<const uint64_t*>(h_meas.data())[i] == ~0ull) again.push_back(i);
        if (!again.empty()) {                                  // (segments past the first plan: counted again)
          if (int rc = sjpeg_internal::counted_bits_recount(e, format, yuv_mode, afr.data(), atab.data(), 1, again, d_bits, st)) return rc;
          if (int rc = read_back(who, h_meas.data(), d_meas, na * sizeof(uint64_t), st)) return rc;
          for (int i : again) {
            if (reinterpret_cast<const uint64_t*>(h_meas.data())[i] == ~0ull) {
              return set_error(SJPEG_HIP_ERUNTIME, who + ": frame " + std::to_string(s[active[i]].index) +
                                                       ": the size pass overran its worst-case plan");
            }
          }
        }
      }
    } else {
      if (int rc = sjpeg_hip_scan_quant_error_ragged_src(e, format, yuv_mode, na, afr.data(), atab.data(), 1,
                                                         reinterpret_cast<uint64_t*>(d_meas), st)) {
        return rc;
      }
      if (int rc = read_back(who, h_meas.data(), d_meas, na * sizeof(uint64_t), st)) return rc;
    }
    // the hooks: each frame's result, its best pass, whether it is done (Encoder::LoopScan)
    for (int i = 0; i < na; ++i) {
      FrameSearch& f = s[active[i]];
      float result;
      if (for_size) {
        const sjpeg_hip_huffman_spec* dc[2] = {nullptr, nullptr};
        const sjpeg_hip_huffman_spec* ac[2] = {nullptr, nullptr};
        sjpeg_hip_huffman_spec specs[4];
        size_t size;
        if (optimize) {
          const uint32_t* const freq = reinterpret_cast<const uint32_t*>(h_meas.data() + static_cast<size_t>(i) * kFreq);
          sjpeg_hip_optimize_huffman(freq, yuv_mode, specs, &atab[i]);
          for (int t = 0; t < ntab; ++t) { dc[t] = &specs[t]; ac[t] = &specs[2 + t]; }
          size = sjpeg_host::SearchHeaderBits(nb_comps, ntab, dc, ac, nullptr);
          size += sjpeg_host::EntropyBits(reinterpret_cast<const uint32_t(*)[272]>(freq), ntab, &atab[i]);
        } else {
          for (int t = 0; t < ntab; ++t) { dc[t] = &sjpeg_host::DefaultHuff(0, t); ac[t] = &sjpeg_host::DefaultHuff(1, t); }
          size = sjpeg_host::SearchHeaderBits(nb_comps, ntab, dc, ac, nullptr);
          size += reinterpret_cast<const uint64_t*>(h_meas.data())[i];
        }
        result = size / 8.f;
      } else {
        const uint64_t err = reinterpret_cast<const uint64_t*>(h_meas.data())[i];
        result = sjpeg_host::SearchPSNR(err, afr[i].width, afr[i].height, yuv_mode);
      }
      const bool last_is_best = (p == 0 || fabs(result - f.hook.target) < f.best);
      if (last_is_best) {
        memcpy(f.opt, f.quant, sizeof(f.opt));
        f.best = fabs(result - f.hook.target);
        f.best_q = f.hook.q;
        f.best_result = result;
      }
      if (f.hook.Update(result)) f.done = true;
    }
  }
  return 0;
}

}  // namespace

// sjpeg_hip_encode_ragged_search_src; sink != NULL: the frames go to the packed buffer (ragged_aux.h) in the order the
// sub-calls code them -- the frames that are not searched, then every part's searched ones
int sjpeg_internal::ragged_search_flow(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                       const sjpeg_hip_ragged_frame* frames, const uint8_t (*quant)[2][64],
                                       int quant_per_frame, const uint8_t* min_quant, int q_bias, int method,
                                       int qdelta_max_luma, int qdelta_max_chroma, const sjpeg_hip_search* search,
                                       int search_per_frame, float* q_out, float* value_out, void* d_out,
                                       uint64_t* d_sizes, void* stream, const PackedSink* sink) {
  static const std::string who = "sjpeg_hip_encode_ragged_search_src";
  if (e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (search == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": search == NULL");
  if (frames == nullptr || quant == nullptr || d_out == nullptr || d_sizes == nullptr) {
    return set_error(SJPEG_HIP_EINVAL, who + ": frames, quant, d_out or d_sizes == NULL");
  }
  if (method < 0 || method > 6) return set_error(SJPEG_HIP_EINVAL, who + ": methods 0..6 (trellis goes through the host API)");
  if (qdelta_max_luma < -12 || qdelta_max_luma > 12 || qdelta_max_chroma < -12 || qdelta_max_chroma > 12) {
    return set_error(SJPEG_HIP_EINVAL, who + ": qdelta_max outside -12 .. 12");
  }
  if (nframes < 1 || nframes > 65535) return set_error(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
  for (int k = 0; k < (search_per_frame ? nframes : 1); ++k) {
    const sjpeg_hip_search& sp = search[k];
    if (sp.target_mode != 1 && sp.target_mode != 2) {
      return set_error(SJPEG_HIP_EINVAL, who + ": search[" + std::to_string(k) + "]: target_mode must be 1 (size) or 2 (PSNR)");
    }
    if (!std::isfinite(sp.target_value)) {
      return set_error(SJPEG_HIP_EINVAL, who + ": search[" + std::to_string(k) + "]: the target is not finite");
    }
  }
  if (int rc = sjpeg_internal::ragged_check(who, format, yuv_mode, nframes, frames)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  try {
    // which frames are searched (passes > 1 after the clamp of src/api.cc:169)
    std::vector<int> searched, plain;
    for (int f = 0; f < nframes; ++f) {
      const int passes = search[search_per_frame ? f : 0].passes;
      (std::min(std::max(passes, 1), 20) > 1 ? searched : plain).push_back(f);
      if (q_out != nullptr) q_out[f] = -1.f;
      if (value_out != nullptr) value_out[f] = -1.f;
    }
    if (searched.empty()) {
      return sjpeg_internal::ragged_batch_flow(e, format, yuv_mode, nframes, frames, quant, quant_per_frame, min_quant, q_bias,
                                               method, qdelta_max_luma, qdelta_max_chroma, d_out, d_sizes, stream, sink);
    }
    if (hipSetDevice(sjpeg_internal::engine_device(e)) != hipSuccess) return hip_fail(who, "hipSetDevice");
    const bool adaptive = method >= 3;
    // a sub-call over frames which[] with matrices q[k]: its sizes go through engine memory to the caller's places (the
    // encode and the copies are still queued on the stream when the call returns: never thread-local scratch)
    uint64_t* d_sub_sizes = nullptr;
    if (int rc = sjpeg_internal::engine_search_sizes(e, static_cast<size_t>(nframes), &d_sub_sizes)) return rc;
    auto sub_encode = [&](const std::vector<int>& which, const uint8_t* q, int m) -> int {
      std::vector<sjpeg_hip_ragged_frame> sub;
      for (int f : which) sub.push_back(frames[f]);
      uint64_t* const d_sub = d_sub_sizes;
      // (packed output: the sub-call's frame k is the caller's which[k])
      sjpeg_internal::PackedSink sub_sink;
      std::vector<int> sub_index;
      if (sink != nullptr) {
        sub_sink = *sink;
        for (int f : which) sub_index.push_back(sink->index != nullptr ? sink->index[f] : f);
        sub_sink.index = sub_index.data();
      }
      if (int rc = sjpeg_internal::ragged_batch_flow(e, format, yuv_mode, static_cast<int>(which.size()), sub.data(),
                                                     reinterpret_cast<const uint8_t(*)[2][64]>(q), 1, min_quant, q_bias, m,
                                                     qdelta_max_luma, qdelta_max_chroma, d_out, d_sub, stream,
                                                     sink != nullptr ? &sub_sink : nullptr)) {
        return rc;
      }
      return scatter_sizes(who, d_sub, which, d_sizes, st);
    };
    // parts of consecutive searched frames whose kept scratch stays inside the engine's limit
    const size_t limit = sjpeg_internal::engine_scratch_limit(e);
    const size_t per_frame = (adaptive ? kHist : 0) + 256 + kAdaptSumsBytes + kAdaptTotBytes + kFreq;
    std::vector<std::pair<size_t, size_t>> parts;       // (first in `searched`, count)
    {
      size_t k0 = 0, bytes = 0;
      for (size_t k = 0; k < searched.size(); ++k) {
        const sjpeg_hip_ragged_frame& fr = frames[searched[k]];
        const int nseg = sjpeg_hip_segment_count(fr.width, fr.height, yuv_mode);
        const size_t b = per_frame + static_cast<size_t>(nseg > 0 ? nseg : 1) * kStatsPartial;
        if (k > k0 && bytes + b > limit) { parts.emplace_back(k0, k - k0); k0 = k; bytes = 0; }
        bytes += b;
      }
      parts.emplace_back(k0, searched.size() - k0);
    }
    size_t most = 0;
    for (const auto& pt : parts) most = std::max(most, pt.second);
    if (!g_search.Ensure(sjpeg_internal::engine_device(e), most * per_frame)) {
      return set_error(SJPEG_HIP_ENOMEM, who + ": hipMalloc(search scratch) failed");
    }
    if (!plain.empty()) {              // the frames that are not searched: their own method and matrices
      std::vector<uint8_t> q(plain.size() * 128);
      for (size_t k = 0; k < plain.size(); ++k) memcpy(&q[k * 128], quant[quant_per_frame ? plain[k] : 0], 128);
      if (int rc = sub_encode(plain, q.data(), method)) return rc;
    }
    std::vector<FrameSearch> s(most);
    std::vector<sjpeg_hip_ragged_frame> pfr;
    for (const auto& pt : parts) {
      const int n = static_cast<int>(pt.second);
      pfr.clear();
      for (int k = 0; k < n; ++k) {
        const int f = searched[pt.first + k];
        pfr.push_back(frames[f]);
        const sjpeg_hip_search& sp = search[search_per_frame ? f : 0];
        FrameSearch& fs = s[k];
        fs = FrameSearch();
        fs.index = f;
        fs.passes = std::min(std::max(static_cast<int>(sp.passes), 1), 20);
        sjpeg::EncoderParam param;
        param.SetQuantization(quant[quant_per_frame ? f : 0]);
        param.target_mode = sp.target_mode == 1 ? sjpeg::EncoderParam::TARGET_SIZE : sjpeg::EncoderParam::TARGET_PSNR;
        param.target_value = sp.target_value;
        param.passes = fs.passes;
        param.tolerance = sp.tolerance;
        param.qmin = sp.qmin;
        param.qmax = sp.qmax;
        fs.hook.Setup(param);
      }
      // one target mode per measurement launch: the frames of the part are searched in runs of their mode
      for (int mode = 1; mode <= 2; ++mode) {
        std::vector<int> sel;
        for (int k = 0; k < n; ++k) if ((s[k].hook.for_size ? 1 : 2) == mode) sel.push_back(k);
        if (sel.empty()) continue;
        std::vector<FrameSearch> ms(sel.size());
        std::vector<sjpeg_hip_ragged_frame> mfr;
        for (size_t i = 0; i < sel.size(); ++i) { ms[i] = s[sel[i]]; mfr.push_back(pfr[sel[i]]); }
        if (int rc = search_part(e, who, format, yuv_mode, mfr.data(), ms.data(), static_cast<int>(sel.size()), min_quant, q_bias,
                                 method, qdelta_max_luma, qdelta_max_chroma, static_cast<uint8_t*>(g_search.p), st)) {
          return rc;
        }
        for (size_t i = 0; i < sel.size(); ++i) s[sel[i]] = ms[i];
      }
      // the best matrices, final (no further adaptation): method 1 (optimised codes) or 0
      std::vector<int> which(n);
      std::vector<uint8_t> best(static_cast<size_t>(n) * 128);
      for (int k = 0; k < n; ++k) {
        which[k] = s[k].index;
        for (int c = 0; c < 2; ++c) sjpeg_host::ScaleMatrix(s[k].opt[c], 100.f, &best[static_cast<size_t>(k) * 128 + 64 * c]);
        if (q_out != nullptr) q_out[s[k].index] = s[k].best_q;
        if (value_out != nullptr) value_out[s[k].index] = s[k].best_result;
      }
      const bool optimize = method != 0 && method != 3;
      if (int rc = sub_encode(which, best.data(), optimize ? 1 : 0)) return rc;
    }
    return 0;
  } catch (...) {
    return set_error(SJPEG_HIP_ENOMEM, who + ": out of host memory");
  }
}

int sjpeg_hip_encode_ragged_search_src(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                       const sjpeg_hip_ragged_frame* frames, const uint8_t (*quant)[2][64],
                                       int quant_per_frame, const uint8_t* min_quant, int q_bias, int method,
                                       int qdelta_max_luma, int qdelta_max_chroma, const sjpeg_hip_search* search,
                                       int search_per_frame, float* q_out, float* value_out, void* d_out,
                                       uint64_t* d_sizes, void* stream) {
  return sjpeg_internal::ragged_search_flow(e, format, yuv_mode, nframes, frames, quant, quant_per_frame, min_quant, q_bias,
                                            method, qdelta_max_luma, qdelta_max_chroma, search, search_per_frame, q_out,
                                            value_out, d_out, d_sizes, stream, nullptr);
}
