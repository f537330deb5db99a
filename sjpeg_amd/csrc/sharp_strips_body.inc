// sharp_strips_body.inc -- the body of sharp_sweeps_strips, included INSIDE the uniform kernel and its ragged twin
// (sharp_yuv.hip) behind their prologues. Textual, not a __device__ function: the uniform kernel then reads its
// arguments exactly as before and compiles to the same code. Names: `a`, `strip`, `nstrips`, `t`, `tid`, `frame` and
// the kernel's LDS arrays g2l, l2g, red, go, above.
  for (int i = tid; i <= kMaxY; i += kStripThreads) g2l[i] = a.tab->g2l[i];
  if (tid < kGammaTab + 2) l2g[tid] = a.tab->l2g[tid];
  const int w = a.w, h = a.h, uv_w = a.uv_w, uv_h = a.uv_h;
  const size_t ysz = static_cast<size_t>(w) * h, usz = static_cast<size_t>(uv_h) * 3 * uv_w;
  const int pin = t % 3, pout = (t + 1) % 3;
  const uint16_t* const in_y = a.best_y + (static_cast<size_t>(pin) * a.nframes + frame) * ysz;
  uint16_t* const out_y = a.best_y + (static_cast<size_t>(pout) * a.nframes + frame) * ysz;
  const int16_t* const in_uv = a.best_uv + (static_cast<size_t>(pin) * a.nframes + frame) * usz;
  int16_t* const out_uv = a.best_uv + (static_cast<size_t>(pout) * a.nframes + frame) * usz;
  const uint16_t* const target_y = a.target_y + static_cast<size_t>(frame) * ysz;
  const int16_t* const target_uv = a.target_uv + static_cast<size_t>(frame) * usz;
  uint32_t* const ctrl = a.ctrl + static_cast<size_t>(frame) * a.ctrl_words;
  uint32_t* const progress = ctrl + 32;             // [4][nstrips]
  const unsigned long long threshold = static_cast<unsigned long long>(3.0 * w * h);
  const int own0 = strip * kStripOwn, own1 = own0 + kStripOwn < uv_w ? own0 + kStripOwn : uv_w;
  const int c = own0 - kStripHalo + tid;            // this thread's chroma column
  const bool live = c >= 0 && c < uv_w;
  const bool owned = c >= own0 && c < own1;
  // the neighbours' places in the LDS row (a column at the picture's edge is its own neighbour, as in the reference;
  // one at the workgroup's edge has none -- it is the first to go invalid, whatever it reads)
  const int tl = (c > 0 && tid > 0) ? tid - 1 : tid, tr = (c < uv_w - 1 && tid < kStripThreads - 1) ? tid + 1 : tid;
  const int s_lo = strip > 0 ? strip - 1 : 0, s_hi = strip < nstrips - 1 ? strip + 1 : strip;

  struct RowData { int uv[3][3]; uint32_t wy[2], ty[2]; int tuv[3]; };
  auto load_uv = [&](int row, int (&dst)[3][3]) {
    const int cl = c > 0 ? c - 1 : 0, cr = c < uv_w - 1 ? c + 1 : uv_w - 1;
    const int16_t* r = in_uv + static_cast<size_t>(row) * 3 * uv_w;
#pragma unroll
    for (int k = 0; k < 3; ++k) { dst[k][0] = r[k * uv_w + cl]; dst[k][1] = r[k * uv_w + c]; dst[k][2] = r[k * uv_w + cr]; }
  };
  auto load_rest = [&](int ry, RowData& d) {
    d.wy[0] = reinterpret_cast<const uint32_t*>(in_y + static_cast<size_t>(2 * ry) * w)[c];
    d.wy[1] = reinterpret_cast<const uint32_t*>(in_y + static_cast<size_t>(2 * ry + 1) * w)[c];
    d.ty[0] = reinterpret_cast<const uint32_t*>(target_y + static_cast<size_t>(2 * ry) * w)[c];
    d.ty[1] = reinterpret_cast<const uint32_t*>(target_y + static_cast<size_t>(2 * ry + 1) * w)[c];
    const int16_t* tu = target_uv + static_cast<size_t>(ry) * 3 * uv_w;
#pragma unroll
    for (int k = 0; k < 3; ++k) d.tuv[k] = tu[k * uv_w + c];
  };
  // Waits until strips s_lo .. s_hi of sweep `tt` have all finished `want` row pairs (visible here), or a sweep has been
  // named the final one (returns -1).  Returns the least of the three counters.
  auto wait_strips = [&](int tt, int want, bool self_too) -> int {
    if (tid == 0) {
      int seen = 0x7fffffff;
      for (int s = s_lo; s <= s_hi && seen >= 0; ++s) {
        if (!self_too && s == strip) continue;
        for (;;) {
          // (relaxed looks: an acquire load is a load AND a cache invalidate, per look and waiting workgroup; the one
          // acquire that matters is the fence behind the barrier below)
          if (__hip_atomic_load(&ctrl[16], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { seen = -1; break; }
          const int p = static_cast<int>(__hip_atomic_load(&progress[tt * nstrips + s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
          if (p >= want) { seen = p < seen ? p : seen; break; }
          __builtin_amdgcn_s_sleep(8);
        }
      }
      go = seen;
    }
    __syncthreads();
    const int g = go;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");     // every wave's loads behind this see the producers' rows
    __syncthreads();                                // (`go` is rewritten by the next call)
    return g;
  };
  constexpr int kAhead = 16;
  int known = t == 0 ? uv_h : 0;                    // row pairs of the sweep before known to be done in all three strips
  auto wait_for = [&](int need) -> bool {
    if (need > uv_h) need = uv_h;
    if (known >= need) return true;
    const int g = wait_strips(t - 1, need + kAhead < uv_h ? need + kAhead : uv_h, true);
    if (g < 0) return false;
    known = g;
    return true;
  };
  SHARP_RACE_POINT(40);
  __syncthreads();
  if (tid == 0 && strip == 0) ctrl[18 + 2 * t] = static_cast<uint32_t>(__builtin_amdgcn_s_memrealtime());
  unsigned long long diff = 0;
  bool wanted = wait_for(3);
  if (wanted) {
    // (a step is shorter than a trip to memory now: what a row pair needs is asked for TWO steps ahead)
    RowData now, ahead, ahead2;
    int nxt[3][3];
    if (live) {
      load_uv(0, now.uv);
      load_rest(0, now);
      load_uv(uv_h > 1 ? 1 : 0, nxt);
      if (uv_h > 1) { load_rest(1, ahead); load_uv(uv_h > 2 ? 2 : 1, ahead.uv); }
#pragma unroll
      for (int k = 0; k < 3; ++k) above[0][k][tid] = static_cast<int16_t>(now.uv[k][1]);   // row pair 0: "above" is the row itself
    }
    SHARP_RACE_POINT(42);
    __syncthreads();
    for (int ry = 0; ry < uv_h; ++ry) {
      const int pp = ry & 1;
      SHARP_RACE_POINT(43);
      if (ry > 0 && (ry % kStripHalo) == 0 && nstrips > 1) {
        // the strips of this sweep meet: the halo's row above comes from the neighbours' output (row ry - 1)
        SHARP_RACE_POINT(47);
        if (wait_strips(t, ry, false) < 0) { wanted = false; break; }
        if (live && !owned) {
          const int16_t* const r = out_uv + static_cast<size_t>(ry - 1) * 3 * uv_w;
#pragma unroll
          for (int k = 0; k < 3; ++k) above[pp][k][tid] = r[k * uv_w + c];       // (behind wait_strips' acquire)
        }
        __syncthreads();
      }
      if (ry + 2 < uv_h) {
        wanted = wait_for(ry + 4);
        if (!wanted) break;
        if (live) {
          load_rest(ry + 2, ahead2);
          load_uv(ry + 3 < uv_h ? ry + 3 : ry + 2, ahead2.uv);     // becomes `nxt` two steps on
        }
      }
      if (live) {
        const int wy[2][2] = {{static_cast<int>(now.wy[0] & 0xffffu), static_cast<int>(now.wy[0] >> 16)},
                              {static_cast<int>(now.wy[1] & 0xffffu), static_cast<int>(now.wy[1] >> 16)}};
        const int ty[2][2] = {{static_cast<int>(now.ty[0] & 0xffffu), static_cast<int>(now.ty[0] >> 16)},
                              {static_cast<int>(now.ty[1] & 0xffffu), static_cast<int>(now.ty[1] >> 16)}};
        int px[2][2][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int A = now.uv[k][1], Al = now.uv[k][0], Ar = now.uv[k][2];
          const int P = above[pp][k][tid], Pl = above[pp][k][tl], Pr = above[pp][k][tr];
          const bool has_next = ry + 1 < uv_h;
          const int N = has_next ? nxt[k][1] : A, Nl = has_next ? nxt[k][0] : Al, Nr = has_next ? nxt[k][2] : Ar;
          int up0, up1, dn0, dn1;
          if (c == 0) { up0 = (A * 3 + P + 2) >> 2; dn0 = (A * 3 + N + 2) >> 2; }
          else { up0 = (A * 9 + Al * 3 + P * 3 + Pl + 8) >> 4; dn0 = (A * 9 + Al * 3 + N * 3 + Nl + 8) >> 4; }
          if (c == uv_w - 1) { up1 = (A * 3 + P + 2) >> 2; dn1 = (A * 3 + N + 2) >> 2; }
          else { up1 = (A * 9 + Ar * 3 + P * 3 + Pr + 8) >> 4; dn1 = (A * 9 + Ar * 3 + N * 3 + Nr + 8) >> 4; }
          px[0][0][k] = clip_y(wy[0][0] + up0); px[0][1][k] = clip_y(wy[0][1] + up1);
          px[1][0][k] = clip_y(wy[1][0] + dn0); px[1][1][k] = clip_y(wy[1][1] + dn1);
        }
        int wt[2][2], uv[3];
        eval_group(g2l, l2g, px, wt, uv);
        uint32_t newy[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          int ny[2];
#pragma unroll
          for (int cc = 0; cc < 2; ++cc) {
            const int d = ty[r][cc] - wt[r][cc];
            ny[cc] = clip_y(wy[r][cc] + d);
            if (owned) diff += static_cast<unsigned long long>(d < 0 ? -d : d);
          }
          newy[r] = static_cast<uint32_t>(ny[0]) | (static_cast<uint32_t>(ny[1]) << 16);
        }
        // (the rows go out as agent-scope stores -- write-through, `sc1` -- so that publishing them needs no release
        // fence: that is an L2 write-back of whatever is dirty, per workgroup and hand-over, and with twenty times the
        // workgroups of the one-per-sweep kernel it halved the throughput of a batch)
        if (owned) {
          __hip_atomic_store(&reinterpret_cast<uint32_t*>(out_y + static_cast<size_t>(2 * ry) * w)[c], newy[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(&reinterpret_cast<uint32_t*>(out_y + static_cast<size_t>(2 * ry + 1) * w)[c], newy[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int16_t nv = static_cast<int16_t>(now.uv[k][1] + (now.tuv[k] - uv[k]));
          if (owned) __hip_atomic_store(&out_uv[static_cast<size_t>(ry) * 3 * uv_w + k * uv_w + c], nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          above[pp ^ 1][k][tid] = nv;
        }
      }
      SHARP_RACE_POINT(44);
      // hand-over (to the next sweep, and to the neighbour strips of this one): every wave's stores are acknowledged in
      // front of the barrier (written through, see above), the counter behind it is a store of the same kind
      const bool hand_over = (ry & 7) == 7 || ry + 1 == uv_h;
      if (hand_over) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      }
      SHARP_RACE_POINT(45);
      if (hand_over && tid == 0) {
        __hip_atomic_store(&progress[t * nstrips + strip], static_cast<uint32_t>(ry + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int q = 0; q < 3; ++q) { now.uv[k][q] = nxt[k][q]; nxt[k][q] = ahead.uv[k][q]; ahead.uv[k][q] = ahead2.uv[k][q]; }
        now.tuv[k] = ahead.tuv[k]; ahead.tuv[k] = ahead2.tuv[k];
      }
      now.wy[0] = ahead.wy[0]; now.wy[1] = ahead.wy[1];
      now.ty[0] = ahead.ty[0]; now.ty[1] = ahead.ty[1];
      ahead.wy[0] = ahead2.wy[0]; ahead.wy[1] = ahead2.wy[1];
      ahead.ty[0] = ahead2.ty[0]; ahead.ty[1] = ahead2.ty[1];
    }
  }
  if (tid == 0 && strip == 0) ctrl[19 + 2 * t] = static_cast<uint32_t>(__builtin_amdgcn_s_memrealtime());
  if (!wanted) return;                              // (uniform: an earlier sweep is the final one)
  // exit test (:660-666): the sweep's sum of |dW| over the picture = the strips' sums; the last strip to arrive takes it
  for (int d = 32; d > 0; d >>= 1) diff += __shfl_down(diff, d, 64);
  if ((tid & 63) == 0) red[tid >> 6] = diff;
  SHARP_RACE_POINT(46);
  __syncthreads();
  if (tid == 0) {
    unsigned long long mine = 0;
    for (int i = 0; i < kStripThreads / 64; ++i) mine += red[i];
    unsigned long long* const sum_t = reinterpret_cast<unsigned long long*>(ctrl + 8 + 2 * t);
    __hip_atomic_fetch_add(sum_t, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t arrived = __hip_atomic_fetch_add(&ctrl[t], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived + 1u == static_cast<uint32_t>(nstrips)) {
      const unsigned long long sum = __hip_atomic_load(sum_t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      bool cancelled = false;
      unsigned long long prev = ~0ull;
      if (t > 0) {
        while (__hip_atomic_load(&ctrl[4 + t - 1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
          if (__hip_atomic_load(&ctrl[16], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
          __builtin_amdgcn_s_sleep(4);
        }
        cancelled = __hip_atomic_load(&ctrl[16], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != 0u;
        prev = __hip_atomic_load(reinterpret_cast<unsigned long long*>(ctrl + 8 + 2 * (t - 1)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (!cancelled) {
        const bool stop = t > 0 && (sum < threshold || sum > prev);
        if (stop || t == 3) {
          ctrl[17] = static_cast<uint32_t>(t);
          __hip_atomic_store(&ctrl[16], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
        __hip_atomic_store(&ctrl[4 + t], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
