// ragged_flows.cc -- the flows of the ragged batch entries over the engine's launch layer (engine.h): the per-picture
// analysis of methods 0..8, the mode groups of SJPEG_YUV_AUTO / SJPEG_YUV_SHARP, the ragged riskiness and sharp
// conversion, packed output.  Host only: every kernel is launched by the unit that defines it.
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "batch_flow.h"
#include "engine.h"

using namespace sjpeg_internal;

// ---- a ragged batch with the reference's per-picture analysis (methods 0..6) ----
// The flow of sjpeg_hip_encode_batch_src over frames of different sizes: the ragged histogram, the adaptation kernels with
// a starting matrix per frame, one read-back and wait; the tables; the ragged statistics, one read-back and wait; the
// Huffman codes and the headers on the host; the ragged encode.  No lanes, no parts, no coefficients kept between passes
// -- but for methods 7 and 8 (sjpeg_hip_encode_ragged_trellis_src), the reference's trellis: their statistics step
// quantizes with the trellis, priced with the standard AC code lengths, and leaves its blocks in the engine's `replay`
// buffer (group after group, frame after frame, kKeptSegBytes a segment); their encode step replays them.
// The frames come in MODE GROUPS (sjpeg_hip_encode_ragged_auto_src: RGB 4:2:0, 4:4:4, 4:0:0 and the sharp frames' planar
// 4:2:0 -- K1 is templated on the mode, so a group is a grid of its own): every pass runs over all groups before its
// one wait, so the host waits do not grow with the number of groups.  sjpeg_hip_encode_ragged_batch_src is one group.
namespace {

struct RaggedGroup {
  int format = 0, yuv_mode = 0;                   // SJPEG_HIP_SRC_*, SJPEG_HIP_YUV*
  std::vector<sjpeg_hip_ragged_frame> frames;     // in group order
  std::vector<int> index;                         // the caller's number of each frame
  std::vector<FrameGeo> geo;
};

// The method 0..6 flow over the groups (their format and frames checked, their geometry set).  d_sizes: the
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
  BatchScratch& sc = batch_scratch();
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
      chunks.push_back(chunks_of(g, kHistPartial, kHist + kSums + kTot));
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
        if (int rc = ragged_analysis(e, kPassHisto, g.format, g.yuv_mode, static_cast<int>(c.second), g.frames.data() + c.first,
                                     std::vector<FrameGeo>(g.geo.begin() + c.first, g.geo.begin() + c.first + c.second),
                                     nullptr, 0, d_hist, st)) return rc;
        if (int rc = adapt_ragged(d_hist, d_qs + (gbase[gi] + c.first) * 128, static_cast<int>(c.second), min_quant, ntab, qdelta_max_luma,
                                  qdelta_max_chroma, static_cast<int64_t*>(sc.d_sums),
                                  reinterpret_cast<int32_t*>(static_cast<uint8_t*>(sc.d_sums) + c.second * kSums),
                                  d_qa + (gbase[gi] + c.first) * 128, st)) return rc;
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
      chunks.push_back(chunks_of(g, kStatsPartial, kFreq));
      for (const auto& c : chunks.back()) most = std::max(most, c.second);
    }
    if (!sc.Ensure(&sc.d_freq, &sc.freq_cap, most * kFreq)) return fail(SJPEG_HIP_ENOMEM, "hipMalloc(batch scratch) failed");
    if (trellis) {
      if (int rc = engine_kept_blocks(e, kept_segs)) return rc;
    }
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      const RaggedGroup& g = groups[gi];
      if (int rc = ready(gi)) return rc;
      for (const auto& c : chunks[gi]) {
        uint32_t* const d_freq = static_cast<uint32_t*>(sc.d_freq);
        if (int rc = ragged_analysis(e, trellis ? kPassStatsTrellis : kPassStats, g.format, g.yuv_mode, static_cast<int>(c.second),
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
      if (int rc = ragged_encode(e, g.format, g.yuv_mode, static_cast<int>(ng), g.frames.data(), g.geo, &tables[gbase[gi]],
                                 (trellis || !one_table) ? 1 : 0, headers.data(), offs.data(), offs[ng], /*append_eoi=*/1, nullptr,
                                 reinterpret_cast<uint64_t*>(d_gsizes + gbase[gi]), st, nullptr,
                                 trellis ? e->replay.p : nullptr, &gs, trellis ? fkept[gi].data() : nullptr)) return rc;
      continue;
    }
    const int rc = trellis ? ragged_encode(e, g.format, g.yuv_mode, static_cast<int>(ng), g.frames.data(), g.geo, &tables[gbase[gi]],
                                           1, headers.data(), offs.data(), offs[ng], /*append_eoi=*/1, d_out,
                                           reinterpret_cast<uint64_t*>(d_gsizes + gbase[gi]), st, nullptr,
                                           e->replay.p, nullptr, fkept[gi].data())
                           : sjpeg_hip_encode_ragged_src(e, g.format, g.yuv_mode, static_cast<int>(ng), g.frames.data(), &tables[gbase[gi]],
                                                         one_table ? 0 : 1, headers.data(), offs.data(), /*append_eoi=*/1, d_out,
                                                         reinterpret_cast<uint64_t*>(d_gsizes + gbase[gi]), st);
    if (rc) return rc;
  }
  if (!in_order) {
    if (int rc = scatter_sizes(d_gsizes, d_index, static_cast<int>(n), reinterpret_cast<unsigned long long*>(d_sizes), st)) return rc;
  }
  mark("encode launched");
  return 0;
}

// The argument checks the batch, auto and trellis flows share behind their engine check, in the order their messages are
// recorded in: the pointers, the method (method_ok; `methods` says which the entry takes), the qdelta range
int flow_args(const std::string& who, const void* frames, const void* quant, const void* d_out, const void* d_sizes,
              bool method_ok, const char* methods, int qdelta_max_luma, int qdelta_max_chroma) {
  if (frames == nullptr || quant == nullptr || d_out == nullptr || d_sizes == nullptr) {
    return fail(SJPEG_HIP_EINVAL, who + ": frames, quant, d_out or d_sizes == NULL");
  }
  if (!method_ok) return fail(SJPEG_HIP_EINVAL, who + methods);
  if (qdelta_max_luma < -12 || qdelta_max_luma > 12 || qdelta_max_chroma < -12 || qdelta_max_chroma > 12) {
    return fail(SJPEG_HIP_EINVAL, who + ": qdelta_max outside -12 .. 12");
  }
  return 0;
}
constexpr const char* kMethods0to6 = ": methods 0..6 (trellis goes through the host API)";

}  // namespace

// sjpeg_hip_encode_ragged_batch_src; sink != NULL: packed output (ragged_aux.h)
int sjpeg_internal::ragged_batch_flow(sjpeg_hip_engine* e, int format, int yuv_mode, int nframes,
                                      const sjpeg_hip_ragged_frame* frames, const uint8_t (*quant_in)[2][64],
                                      int quant_per_frame, const uint8_t* min_quant, int q_bias, int method,
                                      int qdelta_max_luma, int qdelta_max_chroma, void* d_out, uint64_t* d_sizes,
                                      void* stream, const PackedSink* sink) {
  static const std::string who = "sjpeg_hip_encode_ragged_batch_src";
  if (e == nullptr) return fail(SJPEG_HIP_EINVAL, who + ": engine == NULL");
  if (int rc = flow_args(who, frames, quant_in, d_out, d_sizes, method >= 0 && method <= 6, kMethods0to6, qdelta_max_luma, qdelta_max_chroma)) return rc;
  if (nframes < 1 || nframes > 65535) return fail(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
  std::vector<RaggedGroup> groups(1);
  RaggedGroup& g = groups[0];
  if (int rc = ragged_format(who, format, yuv_mode)) return rc;
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

}  // extern "C"

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

}  // namespace

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
      if (int rc = ragged_format(who, g.format, g.yuv_mode)) return rc;
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
  if (int rc = flow_args(who, frames, quant_in, d_out, d_sizes, method >= 0 && method <= 6, kMethods0to6, qdelta_max_luma, qdelta_max_chroma)) return rc;
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
  if (int rc = flow_args(who, frames, quant_in, d_out, d_sizes, method == 7 || method == 8,
                         ": methods 7 and 8 (the others: sjpeg_hip_encode_ragged_auto_src)", qdelta_max_luma, qdelta_max_chroma)) return rc;
  try {
    if (yuv_mode == kYuvAuto || yuv_mode == kYuvSharp) {
      if (int rc = rgb_ragged_frames(who, format, nframes, frames)) return rc;
      std::vector<FrameGeo> geo;                   // (the output ranges)
      if (int rc = ragged_frames(who, format, SJPEG_HIP_YUV444, nframes, frames, true, &geo)) return rc;
    } else {
      if (nframes < 1 || nframes > 65535) return fail(SJPEG_HIP_EINVAL, who + ": nframes must be 1..65535");
      std::vector<FrameGeo> geo;
      if (int rc = ragged_format(who, format, yuv_mode)) return rc;
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
      if (int rc = ragged_format(who, g.format, g.yuv_mode)) return rc;
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
