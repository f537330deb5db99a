// risk_scan_body.inc -- the body of risk_scan (riskiness.hip) and of its ragged twin risk_scan_ragged, included
// INSIDE each kernel behind its prologue. It uses the kernel's names: `a` (RiskArgs of the frame), `frame`, `i` (the
// column), `j0`, `j1` (the rows of the band), the LDS array `part` and the macro RISK_INDEX(p), the cell index of the
// pixel at p (the uniform kernel: yuv_index of its bytes; the ragged one: through the element load). (Textual, not a __device__ function: the
// uniform kernel then reads its arguments exactly as before and compiles to the same code.)
  unsigned long long s_sum = 0;
  uint32_t s_num = 0, g_num = 0;
  if (i < a.W - 1 && j0 < j1) {
    const uint8_t* row = a.rgb + frame * a.frame_stride + static_cast<long long>(j0 - 1) * a.row_stride;
    const long long o0 = static_cast<long long>(i) * a.pix_step, o1 = o0 + a.pix_step;
    int idx0 = RISK_INDEX(row + o0);
    constexpr int gray = (kCells / 2) * (1 + kCells) * kCells;
    constexpr int gray_min = gray - gray % kCells;             // idx = y + 7 * (u + 7 * v): neutral chroma <=> [gray_min, gray_min + 7)
    for (int j = j0; j < j1; ++j) {
      const int idx1 = RISK_INDEX(row + o1);
      row += a.row_stride;
      const int idx2 = RISK_INDEX(row + o0);
      const int score = a.table[idx0 + kCells3 * idx1] + a.table[idx0 + kCells3 * idx2] + a.table[idx1 + kCells3 * idx2];
      if (score > kNoiseLevel) { s_sum += static_cast<unsigned long long>(score); ++s_num; }
      g_num += (idx0 >= gray_min && idx0 < gray_min + kCells) ? 1u : 0u;
      idx0 = idx2;
    }
  }
  unsigned long long n_sum = s_num, gn_sum = g_num;
  for (int d = 32; d > 0; d >>= 1) {
    s_sum += __shfl_down(s_sum, d, 64); n_sum += __shfl_down(n_sum, d, 64); gn_sum += __shfl_down(gn_sum, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6][0] = s_sum; part[threadIdx.x >> 6][1] = n_sum; part[threadIdx.x >> 6][2] = gn_sum;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const unsigned long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (v) atomicAdd(&a.out[static_cast<size_t>(frame) * 3 + threadIdx.x], v);
  }
