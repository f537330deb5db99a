// batch_flow.h -- what the two batch flows (batch_flow.cc: frames of one size, lanes and parts; ragged_flows.cc: frames
// of different sizes, mode groups) share: the calling thread's device scratch, and the two host steps between their
// passes.  Internal, host only.
#pragma once
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "engine.h"

namespace sjpeg_internal {

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
BatchScratch& batch_scratch();       // the calling thread's

// frames f0 .. f0 + nf - 1 take the adapted matrices that came back to h_q ([frame][128]), and the tables of them
void adopt_matrices(const uint8_t* h_q, size_t f0, size_t nf, int yuv_mode, const uint8_t* min_quant, int q_bias,
                    uint8_t* quant, sjpeg_hip_scan_tables* tables);

// the headers of frames f0 .. f0 + nf - 1 back to back, frame f0 + k's at (*offs)[k] .. (*offs)[k + 1]; dims(k) is its
// width and height.  quant: [frame][128]; specs: [frame][4], or NULL for the default codes; meta (may be empty): meta(k)
// is its metadata, or NULL
int batch_headers(const std::string& who, const std::function<std::pair<int, int>(size_t)>& dims, size_t f0, size_t nf, int yuv_mode, const uint8_t* quant,
                  const sjpeg_hip_huffman_spec* specs, std::vector<uint8_t>* headers, std::vector<size_t>* offs,
                  const std::function<const FrameMeta*(size_t)>& meta = {});

}  // namespace sjpeg_internal
