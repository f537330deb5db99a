// sharp_small_body.inc -- the body of sharp_small, included INSIDE the uniform kernel and its ragged twin
// (sharp_yuv.hip) behind their prologues. Textual, not a __device__ function: the uniform kernel then reads its
// arguments exactly as before and compiles to the same code. SHARP_PX(p, off, c): the sample of channel c at p + off, 0..255 (the
// uniform kernel: the byte there; the ragged one: through the element load of pixel_elem.h). Names: `a`, `frame`.
  const uint8_t* base = a.rgb + frame * a.frame_stride;
  const int cw = (a.W + 1) >> 1, ch = (a.H + 1) >> 1;
  for (int i = threadIdx.x; i < a.W * a.H; i += 64) {
    const int x = i % a.W, y = i / a.W;
    const uint8_t* p = base + y * a.row_stride + static_cast<long long>(x) * a.pix_step;
    const int v = 19595 * SHARP_PX(p, a.r_off, 0) + 38469 * SHARP_PX(p, a.g_off, 1) + 7471 * SHARP_PX(p, a.b_off, 2);
    a.y[frame * a.y_frame_stride + i] = static_cast<uint8_t>((v + (1 << 16 >> 1)) >> 16);
  }
  for (int i = threadIdx.x; i < cw * ch; i += 64) {
    const int cx = i % cw, cy = i / cw;
    const int y0 = 2 * cy, y1 = min(2 * cy + 1, a.H - 1);
    const int x0 = 2 * cx, x1 = 2 * cx + 1;
    const uint8_t* p00 = base + y0 * a.row_stride + static_cast<long long>(x0) * a.pix_step;
    const uint8_t* p10 = base + y1 * a.row_stride + static_cast<long long>(x0) * a.pix_step;
    int r, g, b;
    if (x1 < a.W) {
      const uint8_t* p01 = p00 + a.pix_step;
      const uint8_t* p11 = p10 + a.pix_step;
      r = SHARP_PX(p00, a.r_off, 0) + SHARP_PX(p01, a.r_off, 0) + SHARP_PX(p10, a.r_off, 0) + SHARP_PX(p11, a.r_off, 0);
      g = SHARP_PX(p00, a.g_off, 1) + SHARP_PX(p01, a.g_off, 1) + SHARP_PX(p10, a.g_off, 1) + SHARP_PX(p11, a.g_off, 1);
      b = SHARP_PX(p00, a.b_off, 2) + SHARP_PX(p01, a.b_off, 2) + SHARP_PX(p10, a.b_off, 2) + SHARP_PX(p11, a.b_off, 2);
    } else {
      r = 2 * (SHARP_PX(p00, a.r_off, 0) + SHARP_PX(p10, a.r_off, 0)); g = 2 * (SHARP_PX(p00, a.g_off, 1) + SHARP_PX(p10, a.g_off, 1)); b = 2 * (SHARP_PX(p00, a.b_off, 2) + SHARP_PX(p10, a.b_off, 2));
    }
    const int rnd = 1 << 18 >> 1;
    a.u[frame * a.uv_frame_stride + i] = static_cast<uint8_t>(clip8(128 + ((-11058 * r - 21709 * g + 32768 * b + rnd) >> 18)));
    a.v[frame * a.uv_frame_stride + i] = static_cast<uint8_t>(clip8(128 + ((32768 * r - 27439 * g - 5328 * b + rnd) >> 18)));
  }
