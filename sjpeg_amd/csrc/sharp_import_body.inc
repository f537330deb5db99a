// sharp_import_body.inc -- the body of sharp_import, included INSIDE the uniform kernel and its ragged twin
// (sharp_yuv.hip) behind their prologues. Textual, not a __device__ function: the uniform kernel then reads its
// arguments exactly as before and compiles to the same code. SHARP_PX(p, off, c): the sample of channel c at p + off, 0..255 (the
// uniform kernel: the byte there; the ragged one: through the element load of pixel_elem.h). Names: `a` (SharpArgs of the frame), `frame`, `c`, `ry`.
  if (c >= a.uv_w) return;
  const uint8_t* base = a.rgb + frame * a.frame_stride;
  int px[2][2][3];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int yy = min(2 * ry + r, a.H - 1);                 // bottom replication
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int xx = min(2 * c + cc, a.W - 1);               // right replication
      const uint8_t* p = base + yy * a.row_stride + static_cast<long long>(xx) * a.pix_step;
      px[r][cc][0] = (SHARP_PX(p, a.r_off, 0) << kSfix) | (1 << kSfix >> 1);
      px[r][cc][1] = (SHARP_PX(p, a.g_off, 1) << kSfix) | (1 << kSfix >> 1);
      px[r][cc][2] = (SHARP_PX(p, a.b_off, 2) << kSfix) | (1 << kSfix >> 1);
    }
  }
  int wt[2][2], uv[3];
  eval_group(a.tab->g2l, a.tab->l2g, px, wt, uv);
  const size_t yo = static_cast<size_t>(frame) * a.w * a.h;
  const size_t uo = (static_cast<size_t>(frame) * a.uv_h + ry) * 3 * a.uv_w;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const size_t o = yo + static_cast<size_t>(2 * ry + r) * a.w + 2 * c + cc;
      a.best_y[o] = static_cast<uint16_t>(gray(px[r][cc][0], px[r][cc][1], px[r][cc][2]));   // StoreGray
      a.target_y[o] = static_cast<uint16_t>(wt[r][cc]);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.target_uv[uo + k * a.uv_w + c] = static_cast<int16_t>(uv[k]);
    a.best_uv[uo + k * a.uv_w + c] = static_cast<int16_t>(uv[k]);
  }
