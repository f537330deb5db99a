// ragged_full.cc -- the reference's multi-pass search (Encoder::LoopScan, src/dichotomy.cc:113-205) over a ragged batch:
// sjpeg_hip_encode_ragged_search_src (one sampling, methods 0..6) and sjpeg_hip_encode_ragged_full[_meta][_packed]_src
// (sjpeg::Encode(EncoderParam) with EVERY combination of SjpegYUVMode 0..4, method 0..8 and a search per frame: also
// SJPEG_YUV_AUTO / SJPEG_YUV_SHARP and the trellis methods 7 and 8, each size pass one trellis quantization,
// src/dichotomy.cc:80-111 StoreRunLevels).  The entry points differ in their checks and messages; the search is ONE flow.
// The host API runs it one picture at a time (host_api.cc, Encoder::Run); here the frames of a part stand in MODE GROUPS
// (4:2:0, 4:4:4, 4:0:0 of the caller's format, the sharp frames as planar 4:2:0; a fixed sampling is one group), every
// pass launches over all groups and then waits once for what it measured.  Per frame, one sjpeg::SearchHook does the
// float arithmetic of the search (Setup / NextMatrix / Update); the measurements are the ones the host API prices a pass
// with (jpeg_host.h: SearchHeaderBits, EntropyBits, SearchPSNR).  The device passes are the engine's ragged ones:
// histogram (kept for the whole search), adaptation, symbol statistics, counted bits, quantization error.  DESIGN.md
// section 4.  The entries on pictures shaped inside the call (ragged_shaped.cc) end in full_flow() here.
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

using namespace sjpeg_internal;      // (the shared sizes, SjpegYUVMode and the mode groups: ragged_aux.h)

// device scratch of the calling thread, kept between calls: everything in it is read back before the call returns
struct FullScratch {
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
  ~FullScratch() { if (p != nullptr) { (void)hipSetDevice(device); (void)hipFree(p); } }
};
thread_local FullScratch g_full;

// one searched frame of a part: its hook, the loop state of Encoder::LoopScan and (trellis) the encoder's live rate table
struct Frame {
  int index = 0;                       // the caller's frame
  int group = 0;                       // its mode group in the part
  int passes = 1;
  sjpeg_hip_ragged_frame fr;           // as its group codes it (a sharp frame: its planes in the engine's arena)
  uint32_t kept_base = 0;              // its first kept segment, fixed for the part
  sjpeg::SearchHook hook;
  uint8_t quant[2][64];                // the pass's matrices (after adaptation)
  uint8_t opt[2][64];                  // the best pass' matrices
  float best = 0.f, best_q = 0.f, best_result = 0.f;
  bool done = false;
  bool last_best = false;              // the last pass the frame ran was its best
  uint8_t rate[2][256];                // Quantizer::codes_' lengths: the standard ones, then what every pass compiled
  sjpeg_hip_scan_tables tables;        // the pass's
  sjpeg_hip_scan_tables pass_tables;   // the last size pass' tables with the codes it compiled ...
  sjpeg_hip_huffman_spec pass_specs[4];   // ... and their specs
};

struct Group {
  int format = 0, yuv_mode = 0, ntab = 2, nb_comps = 3;
  int first = 0, count = 0;            // its frames: slots [first, first + count) of the part
};

struct Call {
  sjpeg_hip_engine* e;
  const std::string* who;
  hipStream_t st;
  const uint8_t* min_quant;
  int q_bias, method, qdelta_max_luma, qdelta_max_chroma;
  bool adaptive, optimize, trellis;
  uint64_t* stats;
  // the part's device scratch: kept histograms [n][kHist] | matrices in [n][128] | adapted [n][128] | sums [n] | totals
  // [n] | measurements [n][kFreq]
  uint32_t* d_hist;
  uint8_t *d_qin, *d_qout, *d_meas;
  int64_t* d_sums;
  int32_t* d_tot;
};

// what HeaderSize() counts of frame f's metadata (NULL: the call has none)
const sjpeg_host::Metadata* frame_metadata(const sjpeg_hip_engine* e, int f) {
  const sjpeg_internal::FrameMeta* const fm = sjpeg_internal::frame_meta(e, f);
  return fm != nullptr ? &fm->meta : nullptr;
}

int hip_fail(const std::string& who, const char* what) {
  const hipError_t err = hipGetLastError();
  return set_error(err == hipErrorOutOfMemory ? SJPEG_HIP_ENOMEM : SJPEG_HIP_ERUNTIME,
                   who + ": " + what + ": " + hipGetErrorString(err));
}

// a read-back and its host wait (counted: sjpeg_hip_engine_search_stats [2])
int read_back(const Call& c, void* h, const void* d, size_t bytes) {
  if (hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c.st) != hipSuccess || hipStreamSynchronize(c.st) != hipSuccess) {
    return hip_fail(*c.who, "read-back");
  }
  c.stats[2] += 1;
  return 0;
}

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

void standard_rate(uint8_t rate[2][256]) {          // InitCodes(true) of the standard tables (src/enc.cc:330-334)
  sjpeg_hip_scan_tables t;
  memset(&t, 0, sizeof(t));
  sjpeg_hip_default_huffman(&t);
  for (int c = 0; c < 2; ++c) for (int i = 0; i < 256; ++i) rate[c][i] = static_cast<uint8_t>(t.ac_codes[c][i] & 0xff);
}

// runs [i0, i1) of consecutive entries of `list` (slots, ascending) that lie in one group -- and, contiguous: in
// consecutive slots
template <typename F>
int for_runs(const std::vector<int>& list, const std::vector<Frame>& s, bool contiguous, F&& fn) {
  for (size_t i = 0; i < list.size();) {
    size_t m = 1;
    while (i + m < list.size() && s[list[i + m]].group == s[list[i]].group &&
           (!contiguous || list[i + m] == list[i] + static_cast<int>(m))) ++m;
    if (int rc = fn(i, i + m)) return rc;
    i += m;
  }
  return 0;
}

// The search of the part's frames with a size target (for_size) or a PSNR target: the passes.  Every pass adapts and
// measures the frames still searching, group after group, and waits once for the matrices (methods 3..8) and once for
// the measurements.
int search_kind(const Call& c, std::vector<Frame>& s, const std::vector<Group>& groups, bool for_size) {
  const std::string& who = *c.who;
  const int n = static_cast<int>(s.size());
  int max_passes = 0;
  for (const Frame& f : s) if (f.hook.for_size == for_size) max_passes = std::max(max_passes, f.passes);
  const bool stats_kind = for_size && c.optimize;          // symbol counts come back; else one 64-bit value a frame
  const bool trellis_pass = stats_kind && c.trellis;
  std::vector<uint8_t> h_q(static_cast<size_t>(n) * 128);
  std::vector<uint8_t> h_meas(static_cast<size_t>(n) * kFreq);
  std::vector<sjpeg_hip_ragged_frame> afr;
  std::vector<sjpeg_hip_scan_tables> atab;
  std::vector<uint32_t> akept;
  std::vector<int> active;
  for (int p = 0; p < max_passes; ++p) {
    active.clear();
    for (int k = 0; k < n; ++k) if (s[k].hook.for_size == for_size && !s[k].done && p < s[k].passes) active.push_back(k);
    if (active.empty()) break;
    c.stats[0] = std::max<uint64_t>(c.stats[0], static_cast<uint64_t>(p) + 1);
    // the pass's matrices: NextMatrix, clamped to min_quant (FinalizeQuantMatrix)
    for (int k : active) {
      s[k].hook.pass = p;
      for (int t = 0; t < 2; ++t) s[k].hook.NextMatrix(t, s[k].quant[t]);
      memset(&s[k].tables, 0, sizeof(s[k].tables));
      sjpeg_hip_finalize_quant(s[k].quant, c.min_quant, c.q_bias, &s[k].tables);
    }
    if (c.adaptive) {
      // AnalyseHisto of the kept histograms with these matrices: a launch per run of consecutive active frames of a group
      for (int k : active) memcpy(&h_q[static_cast<size_t>(k) * 128], s[k].quant, 128);
      if (hipMemcpyAsync(c.d_qin, h_q.data(), h_q.size(), hipMemcpyHostToDevice, c.st) != hipSuccess) return hip_fail(who, "matrices");
      if (int rc = for_runs(active, s, true, [&](size_t i0, size_t i1) -> int {
            const size_t k0 = active[i0];
            return sjpeg_internal::adapt_ragged(c.d_hist + k0 * (kHist / 4), c.d_qin + k0 * 128, static_cast<int>(i1 - i0), c.min_quant,
                                                groups[s[k0].group].ntab, c.qdelta_max_luma, c.qdelta_max_chroma,
                                                c.d_sums + k0 * (kSums / 8), c.d_tot + k0 * (kTot / 4),
                                                c.d_qout + k0 * 128, c.st);
          })) return rc;
      if (int rc = read_back(c, h_q.data(), c.d_qout, h_q.size())) return rc;                    // (wait 1: the matrices)
      for (int k : active) {
        memcpy(s[k].quant, &h_q[static_cast<size_t>(k) * 128], static_cast<size_t>(groups[s[k].group].ntab) * 64);
        sjpeg_hip_finalize_quant(s[k].quant, c.min_quant, c.q_bias, &s[k].tables);
      }
    }
    // the measurement of every active frame: a launch per group, then one wait
    afr.clear(); atab.clear(); akept.clear();
    for (int k : active) {
      afr.push_back(s[k].fr);
      atab.push_back(s[k].tables);
      sjpeg_hip_scan_tables& t = atab.back();
      if (for_size) sjpeg_hip_default_huffman(&t);
      if (trellis_pass) {                                    // priced with the frame's accumulated rate table
        t.flags |= SJPEG_HIP_QUANT_TRELLIS;
        memcpy(t.trellis_len, s[k].rate, sizeof(s[k].rate));
      }
      akept.push_back(s[k].kept_base);
    }
    const int na = static_cast<int>(active.size());
    uint64_t* const d_vals = reinterpret_cast<uint64_t*>(c.d_meas);
    if (int rc = for_runs(active, s, false, [&](size_t i0, size_t i1) -> int {
          const Group& g = groups[s[active[i0]].group];
          const int m = static_cast<int>(i1 - i0);
          c.stats[1] += 1;
          if (trellis_pass) {
            c.stats[5] += 1;
            return sjpeg_internal::trellis_stats_ragged(c.e, who, g.format, g.yuv_mode, m, &afr[i0], &atab[i0], &akept[i0],
                                                        reinterpret_cast<uint32_t*>(c.d_meas + i0 * kFreq), c.st);
          }
          if (stats_kind) {
            return sjpeg_hip_scan_symbol_stats_ragged_src(c.e, g.format, g.yuv_mode, m, &afr[i0], &atab[i0], 1,
                                                          reinterpret_cast<uint32_t*>(c.d_meas + i0 * kFreq), c.st);
          }
          if (for_size) return sjpeg_internal::counted_bits_first(c.e, g.format, g.yuv_mode, m, &afr[i0], &atab[i0], 1, d_vals + i0, c.st);
          return sjpeg_hip_scan_quant_error_ragged_src(c.e, g.format, g.yuv_mode, m, &afr[i0], &atab[i0], 1, d_vals + i0, c.st);
        })) return rc;
    if (int rc = read_back(c, h_meas.data(), c.d_meas, na * (stats_kind ? kFreq : sizeof(uint64_t)))) return rc;   // (wait 2)
    const uint64_t* const h_vals = reinterpret_cast<const uint64_t*>(h_meas.data());
    if (for_size && !stats_kind) {                           // (segments past the first plan: counted again, one more wait)
      bool any = false;
      if (int rc = for_runs(active, s, false, [&](size_t i0, size_t i1) -> int {
            const Group& g = groups[s[active[i0]].group];
            std::vector<int> again;
            for (size_t i = i0; i < i1; ++i) if (h_vals[i] == ~0ull) again.push_back(static_cast<int>(i - i0));
            if (again.empty()) return 0;
            any = true;
            c.stats[1] += 1;
            return sjpeg_internal::counted_bits_recount(c.e, g.format, g.yuv_mode, &afr[i0], &atab[i0], 1, again, d_vals + i0, c.st);
          })) return rc;
      if (any) {
        if (int rc = read_back(c, h_meas.data(), c.d_meas, na * sizeof(uint64_t))) return rc;
        for (int i = 0; i < na; ++i) {
          if (h_vals[i] == ~0ull) {
            return set_error(SJPEG_HIP_ERUNTIME, who + ": frame " + std::to_string(s[active[i]].index) +
                                                     ": the size pass overran its worst-case plan");
          }
        }
      }
    }
    // the hooks: each frame's result, its best pass, whether it is done (Encoder::LoopScan)
    for (int i = 0; i < na; ++i) {
      Frame& f = s[active[i]];
      const Group& g = groups[f.group];
      float result;
      if (for_size) {
        const sjpeg_hip_huffman_spec* dc[2] = {nullptr, nullptr};
        const sjpeg_hip_huffman_spec* ac[2] = {nullptr, nullptr};
        sjpeg_hip_huffman_spec specs[4];
        size_t size;
        if (stats_kind) {
          const uint32_t* const freq = reinterpret_cast<const uint32_t*>(h_meas.data() + static_cast<size_t>(i) * kFreq);
          sjpeg_hip_optimize_huffman(freq, g.yuv_mode, specs, &atab[i]);
          for (int t = 0; t < g.ntab; ++t) { dc[t] = &specs[t]; ac[t] = &specs[2 + t]; }
          size = sjpeg_host::SearchHeaderBits(g.nb_comps, g.ntab, dc, ac, frame_metadata(c.e, f.index));
          size += sjpeg_host::EntropyBits(reinterpret_cast<const uint32_t(*)[272]>(freq), g.ntab, &atab[i]);
          if (trellis_pass) {
            // InitCodes(true) after CompileEntropyStats (src/dichotomy.cc:152, src/entropy.cc:116-128): the lengths of the
            // symbols the pass's AC tables HAVE go over the rate table, the others stay
            for (int t = 0; t < g.ntab; ++t) {
              for (int j = 0; j < specs[2 + t].nsyms; ++j) {
                const int sym = specs[2 + t].syms[j];
                f.rate[t][sym] = static_cast<uint8_t>(atab[i].ac_codes[t][sym] & 0xff);
              }
            }
            f.pass_tables = atab[i];
            memcpy(f.pass_specs, specs, sizeof(specs));
          }
        } else {
          for (int t = 0; t < g.ntab; ++t) { dc[t] = &sjpeg_host::DefaultHuff(0, t); ac[t] = &sjpeg_host::DefaultHuff(1, t); }
          size = sjpeg_host::SearchHeaderBits(g.nb_comps, g.ntab, dc, ac, frame_metadata(c.e, f.index));
          size += h_vals[i];
        }
        result = size / 8.f;
      } else {
        result = sjpeg_host::SearchPSNR(h_vals[i], afr[i].width, afr[i].height, g.yuv_mode);
      }
      f.last_best = (p == 0 || fabs(result - f.hook.target) < f.best);
      if (f.last_best) {
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

// The end of the search for the part's trellis frames (src/dichotomy.cc:178-201).  A size-searched frame whose last pass
// was its best is not quantized again: its stream is that pass's blocks with the codes that pass compiled.  Every other
// frame gets one more trellis statistics pass with its best matrices (no adaptation) and its rate table as it stands.
// Then ONE replay launch per group covers all its frames, each at its fixed place in the kept blocks.
int finish_trellis(const Call& c, std::vector<Frame>& s, const std::vector<Group>& groups, void* d_out, uint64_t* d_sizes,
                   const sjpeg_internal::PackedSink* sink) {
  const std::string& who = *c.who;
  const int n = static_cast<int>(s.size());
  std::vector<sjpeg_hip_scan_tables> tables(n);
  std::vector<sjpeg_hip_huffman_spec> specs(static_cast<size_t>(n) * 4);
  std::vector<uint8_t> best(static_cast<size_t>(n) * 128);
  std::vector<int> again;
  for (int k = 0; k < n; ++k) {
    Frame& f = s[k];
    uint8_t(*const q)[64] = reinterpret_cast<uint8_t(*)[64]>(&best[static_cast<size_t>(k) * 128]);
    for (int t = 0; t < 2; ++t) sjpeg_host::ScaleMatrix(f.opt[t], 100.f, q[t]);
    memset(&tables[k], 0, sizeof(tables[k]));
    sjpeg_hip_finalize_quant(q, c.min_quant, c.q_bias, &tables[k]);
    if (f.hook.for_size && f.last_best) {
      tables[k] = f.pass_tables;
      memcpy(&specs[static_cast<size_t>(k) * 4], f.pass_specs, sizeof(f.pass_specs));
      c.stats[3] += 1;
      continue;
    }
    sjpeg_hip_default_huffman(&tables[k]);
    tables[k].flags |= SJPEG_HIP_QUANT_TRELLIS;
    memcpy(tables[k].trellis_len, f.rate, sizeof(f.rate));
    again.push_back(k);
    c.stats[4] += 1;
  }
  if (!again.empty()) {
    std::vector<sjpeg_hip_ragged_frame> afr;
    std::vector<sjpeg_hip_scan_tables> atab;
    std::vector<uint32_t> akept;
    for (int k : again) { afr.push_back(s[k].fr); atab.push_back(tables[k]); akept.push_back(s[k].kept_base); }
    if (int rc = for_runs(again, s, false, [&](size_t i0, size_t i1) -> int {
          const Group& g = groups[s[again[i0]].group];
          c.stats[5] += 1;
          return sjpeg_internal::trellis_stats_ragged(c.e, who, g.format, g.yuv_mode, static_cast<int>(i1 - i0), &afr[i0], &atab[i0],
                                                      &akept[i0], reinterpret_cast<uint32_t*>(c.d_meas + i0 * kFreq), c.st);
        })) return rc;
    std::vector<uint8_t> h_meas(again.size() * kFreq);
    if (int rc = read_back(c, h_meas.data(), c.d_meas, h_meas.size())) return rc;
    for (size_t i = 0; i < again.size(); ++i) {
      const int k = again[i];
      sjpeg_hip_optimize_huffman(reinterpret_cast<const uint32_t*>(h_meas.data() + i * kFreq), groups[s[k].group].yuv_mode,
                                 &specs[static_cast<size_t>(k) * 4], &tables[k]);
    }
  }
  uint64_t* d_sub = nullptr;
  if (int rc = sjpeg_internal::engine_search_sizes(c.e, static_cast<size_t>(n), &d_sub)) return rc;
  std::vector<int> which(n);
  for (int k = 0; k < n; ++k) which[k] = s[k].index;
  for (const Group& g : groups) {
    if (g.count == 0) continue;
    std::vector<uint8_t> headers;
    std::vector<size_t> offs(static_cast<size_t>(g.count) + 1, 0);
    std::vector<sjpeg_hip_ragged_frame> gfr;
    std::vector<uint32_t> gkept;
    std::vector<int> gidx;
    for (int k = g.first; k < g.first + g.count; ++k) {
      if (!sjpeg_internal::append_frame_header(s[k].fr.width, s[k].fr.height, g.yuv_mode,
                                               reinterpret_cast<const uint8_t(*)[64]>(&best[static_cast<size_t>(k) * 128]),
                                               &specs[static_cast<size_t>(k) * 4], sjpeg_internal::frame_meta(c.e, s[k].index), &headers)) {
        return set_error(SJPEG_HIP_EINVAL, who + ": header generation failed");
      }
      offs[k - g.first + 1] = headers.size();
      gfr.push_back(s[k].fr);
      gkept.push_back(s[k].kept_base);
      gidx.push_back(sink != nullptr && sink->index != nullptr ? sink->index[s[k].index] : s[k].index);
    }
    sjpeg_internal::PackedSink gs;
    if (sink != nullptr) { gs = *sink; gs.index = gidx.data(); }
    if (int rc = sjpeg_internal::replay_encode_ragged(c.e, who, g.format, g.yuv_mode, g.count, gfr.data(), &tables[g.first], gkept.data(),
                                                      headers.data(), offs.data(), d_out, d_sub + g.first, c.st,
                                                      sink != nullptr ? &gs : nullptr)) return rc;
  }
  return scatter_sizes(who, d_sub, which, d_sizes, c.st);
}

// the passes of frame f's search after the clamp of src/api.cc:169 (1: the frame is not searched)
int passes_of(const sjpeg_hip_ragged_params& P, int f) {
  return P.search == nullptr ? 1 : std::min(std::max(static_cast<int>(P.search[P.search_per_frame ? f : 0].passes), 1), 20);
}

// The flow behind every entry point of this file (arguments checked): the frames that are not searched go to the
// unsearched flow of the same method and mode, the searched ones through the passes, in parts.  stats: the six counters
// of sjpeg_hip_engine_search_stats.  sink != NULL: the frames go to the packed buffer (ragged_aux.h) in the order the
// sub-calls code them -- the frames that are not searched, then every part's searched ones.
int search_flow(const std::string& who, sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                const sjpeg_hip_ragged_params& P, void* d_out, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                void* stream, const PackedSink* sink, uint64_t* stats) {
  const int yuv_mode = P.yuv_mode, method = P.method;
  hipStream_t st = static_cast<hipStream_t>(stream);
  try {
    std::vector<int> searched, plain;
    for (int f = 0; f < nframes; ++f) {
      (passes_of(P, f) > 1 ? searched : plain).push_back(f);
      if (q_out != nullptr) q_out[f] = -1.f;
      if (value_out != nullptr) value_out[f] = -1.f;
    }
    if (searched.empty()) {
      return sjpeg_internal::ragged_unsearched_flow(e, format, yuv_mode, nframes, frames, P.quant, P.quant_per_frame, P.min_quant,
                                                    P.q_bias, method, P.qdelta_max_luma, P.qdelta_max_chroma, d_out, d_sizes, modes,
                                                    stream, sink);
    }
    const int dev = sjpeg_internal::engine_device(e);
    if (hipSetDevice(dev) != hipSuccess) return hip_fail(who, "hipSetDevice");
    Call c;
    c.e = e; c.who = &who; c.st = st; c.min_quant = P.min_quant; c.q_bias = P.q_bias; c.method = method;
    c.qdelta_max_luma = P.qdelta_max_luma; c.qdelta_max_chroma = P.qdelta_max_chroma;
    c.adaptive = method >= 3; c.optimize = method != 0 && method != 3; c.trellis = method >= 7;
    c.stats = stats;
    const size_t n_all = static_cast<size_t>(nframes);
    // 1. the modes: the riskiness of every frame, one wait, the verdicts (SJPEG_YUV_AUTO)
    std::vector<int> mode(n_all, yuv_mode);
    if (yuv_mode == kYuvAuto) {
      if (!g_full.Ensure(dev, n_all * 24)) return set_error(SJPEG_HIP_ENOMEM, who + ": hipMalloc(search scratch) failed");
      uint64_t* const d_sums = static_cast<uint64_t*>(g_full.p);
      if (int rc = sjpeg_hip_riskiness_ragged_src(e, format, nframes, frames, nullptr, d_sums, stream)) return rc;
      std::vector<uint64_t> sums(n_all * 3);
      if (int rc = read_back(c, sums.data(), d_sums, n_all * 24)) return rc;
      for (size_t f = 0; f < n_all; ++f) mode[f] = sjpeg_hip_riskiness_verdict(&sums[f * 3], frames[f].width, frames[f].height, nullptr);
    }
    if (modes != nullptr) for (size_t f = 0; f < n_all; ++f) modes[f] = mode[f];
    // 2. the frames that are not searched: the unsearched flow of the same method and mode, its own waits.  Its sizes go
    // through engine memory to the caller's places (the encode and the copies are still queued on the stream when the call
    // returns: never thread-local scratch)
    if (!plain.empty()) {
      std::vector<sjpeg_hip_ragged_frame> sub;
      std::vector<uint8_t> q(plain.size() * 128);
      std::vector<int> sub_index;
      for (size_t k = 0; k < plain.size(); ++k) {
        sub.push_back(frames[plain[k]]);
        memcpy(&q[k * 128], P.quant[P.quant_per_frame ? plain[k] : 0], 128);
        sub_index.push_back(sink != nullptr && sink->index != nullptr ? sink->index[plain[k]] : plain[k]);
      }
      sjpeg_internal::PackedSink sub_sink;
      if (sink != nullptr) { sub_sink = *sink; sub_sink.index = sub_index.data(); }
      uint64_t* d_sub = nullptr;
      if (int rc = sjpeg_internal::engine_search_sizes(e, n_all, &d_sub)) return rc;
      // (that flow numbers its frames 0 .. plain.size() - 1: their metadata is found under the caller's numbers)
      struct MetaIndex {
        sjpeg_internal::MetaCtx* m;
        MetaIndex(sjpeg_internal::MetaCtx* ctx, const int* index) : m(ctx) { if (m != nullptr) m->index = index; }
        ~MetaIndex() { if (m != nullptr) m->index = nullptr; }
      } meta_index(sjpeg_internal::engine_meta(e), plain.data());
      if (int rc = sjpeg_internal::ragged_unsearched_flow(e, format, yuv_mode, static_cast<int>(plain.size()), sub.data(),
                                                          reinterpret_cast<const uint8_t(*)[2][64]>(q.data()), 1, P.min_quant, P.q_bias,
                                                          method, P.qdelta_max_luma, P.qdelta_max_chroma, d_out, d_sub, nullptr, stream,
                                                          sink != nullptr ? &sub_sink : nullptr)) return rc;
      if (int rc = scatter_sizes(who, d_sub, plain, d_sizes, st)) return rc;
      stats[2] += (yuv_mode == kYuvAuto ? 1 : 0) + (c.adaptive ? 1 : 0) + (c.optimize ? 1 : 0);     // (that flow's, in one part)
    }
    // 3. parts of consecutive searched frames whose kept scratch -- histograms, partials, sharp planes and workspace, kept
    // blocks -- stays inside the engine's limit
    const size_t limit = sjpeg_internal::engine_scratch_limit(e);
    const size_t per_frame = (c.adaptive ? kHist : 0) + 256 + kSums + kTot + kFreq;
    std::vector<std::pair<size_t, size_t>> parts;       // (first in `searched`, count)
    size_t most = 0, most_arena = 0, most_kept = 0;
    {
      size_t k0 = 0, bytes = 0, kept = 0;
      std::vector<sjpeg_hip_ragged_frame> sharp;
      auto close = [&](size_t end) {
        size_t planes = 0;
        for (const auto& fr : sharp) planes += planes_bytes(fr);
        const size_t ws = sharp.empty() ? 0 : sjpeg_internal::sharp_ragged_workspace(static_cast<int>(sharp.size()), sharp.data());
        most_arena = std::max(most_arena, sharp.empty() ? 0 : align16(planes) + ws);
        most_kept = std::max(most_kept, kept);
        most = std::max(most, end - k0);
        parts.emplace_back(k0, end - k0);
        sharp.clear();
        kept = 0;
      };
      for (size_t k = 0; k < searched.size(); ++k) {
        const int f = searched[k];
        const sjpeg_hip_ragged_frame& fr = frames[f];
        const int nseg = std::max(sjpeg_hip_segment_count(fr.width, fr.height, hip_yuv_mode(mode[f])), 1);
        const bool is_sharp = mode[f] == kYuvSharp;
        const size_t b = per_frame + static_cast<size_t>(nseg) * kStatsPartial +
                         (is_sharp ? planes_bytes(fr) + sjpeg_internal::sharp_ragged_workspace(1, &fr) : 0) +
                         (c.trellis ? static_cast<size_t>(nseg) * kKeptSegBytes : 0);
        if (k > k0 && bytes + b > limit) { close(k); k0 = k; bytes = 0; }
        if (is_sharp) sharp.push_back(fr);
        if (c.trellis) kept += static_cast<size_t>(nseg);
        bytes += b;
      }
      close(searched.size());
    }
    if (!g_full.Ensure(dev, most * per_frame)) return set_error(SJPEG_HIP_ENOMEM, who + ": hipMalloc(search scratch) failed");
    uint8_t* d_arena = nullptr;
    if (most_arena > 0) { if (int rc = sjpeg_internal::engine_arena(e, most_arena, &d_arena)) return rc; }
    if (c.trellis) { if (int rc = sjpeg_internal::engine_kept_blocks(e, most_kept)) return rc; }
    std::vector<uint8_t> best_all;                      // (methods 0..6: the best matrices by the caller's frame number)
    if (!c.trellis) best_all.assign(n_all * 128, 0);
    for (const auto& pt : parts) {
      const int n = static_cast<int>(pt.second);
      // 4. the part's mode groups, its frames in group order: that order is their slot in every scratch array
      std::vector<Frame> s;
      std::vector<Group> groups;
      s.reserve(pt.second);
      for (int kind : kGroupKinds) {
        Group g;
        g.format = group_format(kind, format);
        g.yuv_mode = hip_yuv_mode(kind);
        g.ntab = g.yuv_mode == SJPEG_HIP_YUV400 ? 1 : 2;
        g.nb_comps = g.yuv_mode == SJPEG_HIP_YUV400 ? 1 : 3;
        g.first = static_cast<int>(s.size());
        for (int k = 0; k < n; ++k) {
          const int f = searched[pt.first + k];
          if (mode[f] != kind) continue;
          s.emplace_back();
          Frame& fs = s.back();
          fs.index = f;
          fs.group = static_cast<int>(groups.size());
          fs.fr = frames[f];
        }
        g.count = static_cast<int>(s.size()) - g.first;
        if (g.count > 0) groups.push_back(g);
      }
      // the kept bases: prefix sums over the part's frames, fixed until its replay; the sharp frames (the part's last
      // group), converted ONCE into planar 4:2:0 planes in the engine's arena
      {
        std::vector<sjpeg_hip_ragged_frame> sharp, planar;
        std::vector<uint8_t*> yuv[3];
        uint32_t kept = 0;
        for (Frame& fs : s) {
          if (c.trellis) {
            fs.kept_base = kept;
            kept += static_cast<uint32_t>(std::max(sjpeg_hip_segment_count(fs.fr.width, fs.fr.height, groups[fs.group].yuv_mode), 1));
          }
          if (mode[fs.index] == kYuvSharp) sharp.push_back(fs.fr);
        }
        if (!sharp.empty()) {
          uint8_t* const ws = place_sharp_planes(d_arena, sharp, &planar, yuv);
          const size_t wsz = sjpeg_internal::sharp_ragged_workspace(static_cast<int>(sharp.size()), sharp.data());
          if (static_cast<size_t>(ws - d_arena) + wsz > most_arena) return set_error(SJPEG_HIP_ERUNTIME, who + ": internal: the sharp planes pass their arena");
          if (int rc = sjpeg_hip_sharp_yuv_ragged(e, format, static_cast<int>(sharp.size()), sharp.data(), yuv[0].data(), yuv[1].data(),
                                                  yuv[2].data(), ws, wsz, stream)) return rc;
          for (size_t k = 0; k < planar.size(); ++k) s[s.size() - planar.size() + k].fr = planar[k];
        }
      }
      // the hooks
      for (Frame& fs : s) {
        const int f = fs.index;
        const sjpeg_hip_search& sp = P.search[P.search_per_frame ? f : 0];
        fs.passes = passes_of(P, f);
        sjpeg::EncoderParam param;
        param.SetQuantization(P.quant[P.quant_per_frame ? f : 0]);
        param.target_mode = sp.target_mode == 1 ? sjpeg::EncoderParam::TARGET_SIZE : sjpeg::EncoderParam::TARGET_PSNR;
        param.target_value = sp.target_value;
        param.passes = fs.passes;
        param.tolerance = sp.tolerance;
        param.qmin = sp.qmin;
        param.qmax = sp.qmax;
        fs.hook.Setup(param);
        if (c.trellis) standard_rate(fs.rate);
      }
      // the part's scratch; the histograms of every group, kept for the whole search
      uint8_t* const base = static_cast<uint8_t*>(g_full.p);
      c.d_hist = reinterpret_cast<uint32_t*>(base);
      c.d_qin = base + (c.adaptive ? static_cast<size_t>(n) * kHist : 0);
      c.d_qout = c.d_qin + static_cast<size_t>(n) * 128;
      c.d_sums = reinterpret_cast<int64_t*>(c.d_qout + static_cast<size_t>(n) * 128);
      c.d_tot = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(c.d_sums) + static_cast<size_t>(n) * kSums);
      c.d_meas = reinterpret_cast<uint8_t*>(c.d_tot) + static_cast<size_t>(n) * kTot;
      std::vector<sjpeg_hip_ragged_frame> gfr;
      for (const Group& g : groups) {
        if (!c.adaptive) break;
        gfr.clear();
        for (int k = g.first; k < g.first + g.count; ++k) gfr.push_back(s[k].fr);
        if (int rc = sjpeg_hip_scan_histogram_ragged_src(e, g.format, g.yuv_mode, g.count, gfr.data(),
                                                         c.d_hist + static_cast<size_t>(g.first) * (kHist / 4), stream)) return rc;
      }
      // 5. the passes: the frames with a size target, then those with a PSNR target (one kind of measurement a launch)
      for (int kind = 1; kind <= 2; ++kind) {
        bool any = false;
        for (const Frame& fs : s) any = any || (fs.hook.for_size == (kind == 1));
        if (!any) continue;
        if (int rc = search_kind(c, s, groups, kind == 1)) return rc;
      }
      for (const Frame& fs : s) {
        if (q_out != nullptr) q_out[fs.index] = fs.best_q;
        if (value_out != nullptr) value_out[fs.index] = fs.best_result;
      }
      // 6. the end of the search
      if (c.trellis) {
        if (int rc = finish_trellis(c, s, groups, d_out, d_sizes, sink)) return rc;
        continue;
      }
      // methods 0..6: the best matrices, final (no further adaptation): method 1 (optimised codes) or 0 over all groups
      std::vector<sjpeg_internal::ModeGroup> mg(groups.size());
      for (size_t gi = 0; gi < groups.size(); ++gi) { mg[gi].format = groups[gi].format; mg[gi].yuv_mode = groups[gi].yuv_mode; }
      for (const Frame& fs : s) {
        for (int t = 0; t < 2; ++t) sjpeg_host::ScaleMatrix(fs.opt[t], 100.f, &best_all[static_cast<size_t>(fs.index) * 128 + 64 * t]);
        mg[fs.group].frames.push_back(fs.fr);
        mg[fs.group].index.push_back(fs.index);
        stats[4] += 1;
      }
      if (int rc = sjpeg_internal::ragged_groups_flow(e, who, mg, reinterpret_cast<const uint8_t(*)[2][64]>(best_all.data()), P.min_quant,
                                                      P.q_bias, c.optimize ? 1 : 0, P.qdelta_max_luma, P.qdelta_max_chroma, d_out,
                                                      d_sizes, stream, sink)) return rc;
      stats[2] += c.optimize ? 1 : 0;                   // (the statistics wait of that flow)
    }
    return 0;
  } catch (...) {
    return set_error(SJPEG_HIP_ENOMEM, who + ": out of host memory");
  }
}

// what is wrong with a metadata member (jpeg_host.h: MetadataFromC names it), in words
std::string meta_fault(const char* field) {
  const std::string f = field;
  if (f == "exif") return "exif: NULL with a size, or its APP1 segment would pass 65535 bytes (at most 65527 bytes of EXIF)";
  if (f == "iccp") return "iccp: NULL with a size, or a profile of 256 chunks or more (at most 255 x 65519 bytes)";
  if (f == "xmp") {
    return "xmp: NULL with a size, or a packet above 65504 bytes (one APP1 segment) without a well-formed xmpNote:HasExtendedXMP=\" note in front of "
           "the split point, or above 2^31 bytes";
  }
  return f + ": NULL with a non-zero size";
}

}  // namespace

// the checks of a _full_ call: host only, the engine is not touched
int sjpeg_internal::full_checks(const std::string& who, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                const sjpeg_hip_ragged_params& P) {
  const int yuv_mode = P.yuv_mode, method = P.method;
  if (nframes < 1 || nframes > 65535) return set_error(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
  if (yuv_mode < kYuvAuto || yuv_mode > kYuv400) return set_error(SJPEG_HIP_EINVAL, who + ": params->yuv_mode outside 0..4 (SjpegYUVMode)");
  if (method < 0 || method > 8) return set_error(SJPEG_HIP_EINVAL, who + ": params->method outside 0..8");
  if (P.qdelta_max_luma < -12 || P.qdelta_max_luma > 12 || P.qdelta_max_chroma < -12 || P.qdelta_max_chroma > 12) {
    return set_error(SJPEG_HIP_EINVAL, who + ": params->qdelta_max outside -12 .. 12");
  }
  if (P.quant == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": params->quant == NULL");
  const bool by_mode = yuv_mode == kYuvAuto || yuv_mode == kYuvSharp;
  const SourceLayout* const L = source_layout(format);
  if (by_mode && (L == nullptr || !L->rgb_like)) {
    return set_error(SJPEG_HIP_EINVAL, who + ": SJPEG_YUV_AUTO and SJPEG_YUV_SHARP take RGB, BGRA or RGBA (packed) or planar RGB sources");
  }
  for (int k = 0; P.search != nullptr && k < (P.search_per_frame ? nframes : 1); ++k) {
    const sjpeg_hip_search& sp = P.search[k];
    if (sp.target_mode != 1 && sp.target_mode != 2) {
      return set_error(SJPEG_HIP_EINVAL, who + ": search[" + std::to_string(k) + "] (frame " + std::to_string(k) +
                                             "): target_mode must be 1 (size) or 2 (PSNR)");
    }
    if (!std::isfinite(sp.target_value)) {
      return set_error(SJPEG_HIP_EINVAL, who + ": search[" + std::to_string(k) + "] (frame " + std::to_string(k) + "): the target is not finite");
    }
  }
  return sjpeg_internal::ragged_check(who, format, by_mode ? SJPEG_HIP_YUV444 : yuv_mode, nframes, frames);
}

int sjpeg_internal::encode_prologue(const RaggedCall& c, bool has_sheet, const void* sheet, bool yuv_only) {
  // (every argument check comes before the engine is touched: the tests without a GPU rely on it)
  const std::string& who = *c.who;
  const RaggedOut& o = c.out;
  if (c.e == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (c.params == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": params == NULL");
  if (o.packed && o.d_offsets == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": d_offsets == NULL");
  if (c.frames == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": frames == NULL");
  if (has_sheet && sheet == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": sheet == NULL");
  if (o.d_out == nullptr) return set_error(SJPEG_HIP_EINVAL, who + (o.packed ? ": d_packed == NULL" : ": d_out == NULL"));
  if (o.d_sizes == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": d_sizes == NULL");
  if (o.packed && (reinterpret_cast<uintptr_t>(o.d_out) & 15u) != 0) return set_error(SJPEG_HIP_EINVAL, who + ": d_packed must be a multiple of 16");
  if (o.packed && o.packed_capacity >= SJPEG_HIP_PACKED_OVERFLOW) return set_error(SJPEG_HIP_EINVAL, who + ": packed_capacity must be below 2^63");
  if (o.strided && o.out_stride < 1) return set_error(SJPEG_HIP_EINVAL, who + ": out_stride must be at least 1");
  if (yuv_only) { if (int rc = yuv_format_check(who, c.format)) return rc; }
  if (c.nframes < 1 || c.nframes > 65535) return set_error(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
  return 0;
}

// A _full_ call behind its prologue: its checks, all of them before the engine is touched, then the search
int sjpeg_internal::full_flow(const RaggedCall& c) {
  const std::string& who = *c.who;
  const sjpeg_hip_ragged_params& P = *c.params;
  const RaggedOut& o = c.out;
  const int yuv_mode = P.yuv_mode, method = P.method;
  if (int rc = full_checks(who, c.format, c.nframes, c.frames, P)) return rc;
  const bool by_mode = yuv_mode == kYuvAuto || yuv_mode == kYuvSharp;
  const PackedSink packed = o.sink(c.nframes);
  const PackedSink* const sink = o.packed ? &packed : nullptr;
  if (sink != nullptr) { if (int rc = engine_pack_begin(c.e, o.stream)) return rc; }
  uint64_t* const stats = engine_full_stats(c.e);
  memset(stats, 0, 6 * sizeof(uint64_t));
  // a search on the ground of sjpeg_hip_encode_ragged_search_src: that entry point's messages, and the counters stay zero
  bool any_searched = false;
  for (int f = 0; f < c.nframes; ++f) any_searched = any_searched || passes_of(P, f) > 1;
  if (any_searched && !by_mode && method <= 6) {
    const int rc = ragged_search_flow(c.e, c.format, yuv_mode, c.nframes, c.frames, P.quant, P.quant_per_frame, P.min_quant, P.q_bias, method,
                                      P.qdelta_max_luma, P.qdelta_max_chroma, P.search, P.search_per_frame, o.q_out, o.value_out, o.d_out,
                                      o.d_sizes, o.stream, sink);
    if (rc == 0 && o.modes != nullptr) for (int f = 0; f < c.nframes; ++f) o.modes[f] = yuv_mode;
    return rc;
  }
  return search_flow(who, c.e, c.format, c.nframes, c.frames, P, o.d_out, o.d_sizes, o.modes, o.q_out, o.value_out, o.stream, sink, stats);
}

// The call's metadata -- one entry, or one per frame -- checked and turned into segments, before any device work
int sjpeg_internal::check_metadata(const std::string& who, int nframes, const sjpeg_hip_metadata* meta, int meta_per_frame, MetaCtx* ctx) {
  ctx->per_frame = meta_per_frame ? 1 : 0;
  ctx->entries.resize(meta_per_frame ? static_cast<size_t>(nframes) : 1);
  for (size_t k = 0; k < ctx->entries.size(); ++k) {
    const char* field = "";
    if (!sjpeg_host::MetadataFromC(&meta[k], &ctx->entries[k].meta, &ctx->entries[k].block, &field)) {
      return set_error(SJPEG_HIP_EINVAL, who + ": meta[" + std::to_string(k) + "] (frame " + std::to_string(k) + "): " + meta_fault(field));
    }
    if (ctx->entries[k].block.size() > 0xffffffffull - 4096) {
      return set_error(SJPEG_HIP_EINVAL, who + ": meta[" + std::to_string(k) + "] (frame " + std::to_string(k) + "): the metadata must stay below 4 GiB");
    }
  }
  return 0;
}

// The one body of sjpeg_hip_encode_ragged_full_src, _full_packed_src, _full_meta_src and _full_meta_packed_src: an
// optional sink (c.out.packed) and an optional metadata (c.meta)
int sjpeg_internal::full_entry(RaggedCall c) {
  static const std::string names[2][2] = {{"sjpeg_hip_encode_ragged_full_src", "sjpeg_hip_encode_ragged_full_packed_src"},
                                          {"sjpeg_hip_encode_ragged_full_meta_src", "sjpeg_hip_encode_ragged_full_meta_packed_src"}};
  c.who = &names[c.meta != nullptr][c.out.packed];
  if (int rc = encode_prologue(c)) return rc;
  try {
    MetaCtx ctx;
    if (c.meta != nullptr) { if (int rc = check_metadata(*c.who, c.nframes, c.meta, c.meta_per_frame, &ctx)) return rc; }
    std::vector<sjpeg_hip_ragged_frame> fr;
    if (c.out.packed) {
      fr.assign(c.frames, c.frames + c.nframes);
      for (sjpeg_hip_ragged_frame& f : fr) f.out_offset = 0;       // (ignored: the placement kernel says where a frame goes)
      c.frames = fr.data();
    }
    // (full_flow zeroes the engine's cursor behind its checks: they come before the engine is touched)
    const MetaScope scope(c.e, c.meta != nullptr ? &ctx : nullptr);
    return full_flow(c);
  } catch (...) {
    return set_error(SJPEG_HIP_ENOMEM, *c.who + ": out of host memory");
  }
}

// sjpeg_hip_encode_ragged_search_src (sink != NULL: packed output): one sampling, methods 0..6 -- its own checks and
// messages, then the flow above with one mode group of the caller's format.  The engine's counters are the _full_
// calls': this one counts into an array of its own.
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
  const sjpeg_hip_ragged_params P = {yuv_mode, method, quant, quant_per_frame, min_quant, q_bias, qdelta_max_luma, qdelta_max_chroma,
                                     search, search_per_frame};
  uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
  return search_flow(who, e, format, nframes, frames, P, d_out, d_sizes, nullptr, q_out, value_out, stream, sink, stats);
}

extern "C" {

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

int sjpeg_hip_encode_ragged_full_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                     const sjpeg_hip_ragged_params* params, void* d_out, uint64_t* d_sizes, int* modes,
                                     float* q_out, float* value_out, void* stream) {
  return sjpeg_internal::full_entry({nullptr, e, format, nframes, frames, params, nullptr, 0,
                                     {d_out, d_sizes, modes, q_out, value_out, stream}});
}

int sjpeg_hip_encode_ragged_full_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                            const sjpeg_hip_ragged_params* params, void* d_packed, size_t packed_capacity,
                                            uint64_t* d_offsets, uint64_t* d_sizes, int* modes, float* q_out, float* value_out,
                                            void* stream) {
  return sjpeg_internal::full_entry({nullptr, e, format, nframes, frames, params, nullptr, 0,
                                     sjpeg_internal::RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)});
}

int sjpeg_hip_encode_ragged_full_meta_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                          const sjpeg_hip_ragged_params* params, const sjpeg_hip_metadata* meta, int meta_per_frame,
                                          void* d_out, uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return sjpeg_internal::full_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                                     {d_out, d_sizes, modes, q_out, value_out, stream}});
}

int sjpeg_hip_encode_ragged_full_meta_packed_src(sjpeg_hip_engine* e, int format, int nframes, const sjpeg_hip_ragged_frame* frames,
                                                 const sjpeg_hip_ragged_params* params, const sjpeg_hip_metadata* meta,
                                                 int meta_per_frame, void* d_packed, size_t packed_capacity, uint64_t* d_offsets,
                                                 uint64_t* d_sizes, int* modes, float* q_out, float* value_out, void* stream) {
  return sjpeg_internal::full_entry({nullptr, e, format, nframes, frames, params, meta, meta_per_frame,
                                     sjpeg_internal::RaggedOut{d_packed, d_sizes, modes, q_out, value_out, stream}.packed_into(packed_capacity, d_offsets)});
}

int sjpeg_hip_metadata_size(const sjpeg_hip_metadata* meta, size_t* size) {
  static const std::string who = "sjpeg_hip_metadata_size";
  if (size == nullptr) return set_error(SJPEG_HIP_EINVAL, who + ": size == NULL");
  *size = 0;
  try {
    sjpeg_internal::FrameMeta fm;
    const char* field = "";
    if (!sjpeg_host::MetadataFromC(meta, &fm.meta, &fm.block, &field)) return set_error(SJPEG_HIP_EINVAL, who + ": " + meta_fault(field));
    *size = fm.block.size();
    return 0;
  } catch (...) {
    return set_error(SJPEG_HIP_ENOMEM, who + ": out of host memory");
  }
}

int sjpeg_hip_engine_search_stats(sjpeg_hip_engine* e, uint64_t stats[6]) {
  if (e == nullptr || stats == nullptr) return set_error(SJPEG_HIP_EINVAL, "sjpeg_hip_engine_search_stats: engine or stats == NULL");
  memcpy(stats, sjpeg_internal::engine_full_stats(e), 6 * sizeof(uint64_t));
  return 0;
}

}  // extern "C"
