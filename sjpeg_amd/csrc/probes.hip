// probes.hip -- measurement aids behind sjpeg_hip_debug_stream_read / _shader_clock / _valu_rate (not in the public
// header; bench.py's roofline lines and tools/ call them): what a read-only streaming kernel reaches on this device, the
// shader clock as the shaders see it, and the cycles a wave64 VALU instruction occupies a SIMD.  No part of any encode.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"

extern "C" {

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
