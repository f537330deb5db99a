// Prints sizeof(sjpeg_hip_ragged_params) and the offsets of its fields as a C++ compiler lays them out
// (tests/test_ragged_packed_host.py compares them with the ctypes structure of the Python bindings).
#include <cstddef>
#include <cstdio>

#include "sjpeg_hip.h"

int main() {
  std::printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(sjpeg_hip_ragged_params), offsetof(sjpeg_hip_ragged_params, quant),
              offsetof(sjpeg_hip_ragged_params, quant_per_frame), offsetof(sjpeg_hip_ragged_params, min_quant),
              offsetof(sjpeg_hip_ragged_params, q_bias), offsetof(sjpeg_hip_ragged_params, search),
              offsetof(sjpeg_hip_ragged_params, search_per_frame));
  return 0;
}
