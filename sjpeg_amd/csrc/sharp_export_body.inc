// sharp_export_body.inc -- the body of sharp_export, included INSIDE the uniform kernel and its ragged twin
// (sharp_yuv.hip) behind their prologues. Textual, not a __device__ function: the uniform kernel then reads its
// arguments exactly as before and compiles to the same code. Names: `a`, `frame`, `c`, `ry`.
  if (c >= a.uv_w) return;
  // (pipelined sweeps: the plane the last sweep that counts wrote)
  const int plane = a.nplanes == 3 ? static_cast<int>((a.ctrl[static_cast<size_t>(frame) * a.ctrl_words + 17] + 1u) % 3u) : 0;
  const size_t pf = static_cast<size_t>(plane) * a.nframes + frame;
  const size_t uo = (pf * a.uv_h + ry) * 3 * a.uv_w;
  const int r = a.best_uv[uo + c], g = a.best_uv[uo + a.uv_w + c], b = a.best_uv[uo + 2 * a.uv_w + c];
  const int rnd = 1 << 18 >> 1;
  const int cw = (a.W + 1) >> 1;
  if (c < cw && ry < ((a.H + 1) >> 1)) {
    uint8_t* up = a.u + frame * a.uv_frame_stride + static_cast<size_t>(ry) * cw;
    uint8_t* vp = a.v + frame * a.uv_frame_stride + static_cast<size_t>(ry) * cw;
    up[c] = static_cast<uint8_t>(clip8(128 + ((-11058 * r - 21709 * g + 32768 * b + rnd) >> 18)));
    vp[c] = static_cast<uint8_t>(clip8(128 + ((32768 * r - 27439 * g - 5328 * b + rnd) >> 18)));
  }
  const size_t yo = pf * a.w * a.h;
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int x = 2 * c + cc, y = 2 * ry + rr;
      if (x < a.W && y < a.H) {
        const int Wv = a.best_y[yo + static_cast<size_t>(y) * a.w + x];
        a.y[frame * a.y_frame_stride + static_cast<size_t>(y) * a.W + x] =
            static_cast<uint8_t>(clip8((19595 * (r + Wv) + 38469 * (g + Wv) + 7471 * (b + Wv) + rnd) >> 18));
      }
    }
  }
