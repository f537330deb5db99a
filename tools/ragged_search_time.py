#!/usr/bin/env python3
"""The batch search (sjpeg_hip_encode_ragged_search_src) against the per-picture loop it replaces: 256 device-resident
pictures of seeded random sizes 320x240 .. 1920x1080, method 4, 4:2:0, each with a target size of half its q75 size,
10 passes.  (a) one batched call; (b) the same call once per picture; (c) one plain encode_ragged_batch at q75 for
scale.  Each: warm-up, then the median of several regions timed by the host clock around calls that end in a device
synchronise.  The bytes of (a) must equal those of (b).  The C-ABI does not report how many passes a frame took or
how often the call waited: the tool prints the q each frame ended at, and the UPPER BOUND on host waits that follows from
the header's contract (two per pass for method 4, at most 10 passes) -- a bound, not an observation.
    python tools/ragged_search_time.py [--n 256] [--regions 3]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sjpeg_amd as sj  # noqa: E402
from oracle import synth  # noqa: E402

MODE, METHOD, PASSES = sj.YUV_420, 4, 10
SIZES = [(320, 240), (640, 480), (800, 600), (1024, 768), (1280, 720), (1920, 1080)]


def timed(fn, regions):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(regions):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def frames(out, sizes, offs):
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    return [host[o:o + int(s)].tobytes() for o, s in zip(offs, sz)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--regions", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.RandomState(7)
    dims = [SIZES[i] for i in rng.randint(0, len(SIZES), args.n)]
    planes = []
    for k, (w, h) in enumerate(dims):
        im = synth.g_struct(w, h, 100 + k)
        planes.append([torch.from_numpy(im.reshape(h, 3 * w)).cuda()])
    quant = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(75.0, quant.ctypes.data)
    eng = sj.Engine(0)
    plain = lambda: eng.encode_ragged_batch(sj.SRC_RGB, planes, dims, MODE, quant, METHOD)  # noqa: E731
    q75 = [len(b) for b in frames(*plain())]
    search = [sj.SearchParams(sj.TARGET_SIZE, 0.5 * s, PASSES, 1.0, 0.0, 100.0) for s in q75]
    batched = lambda: eng.encode_ragged_search(sj.SRC_RGB, planes, dims, MODE, quant, search, METHOD)  # noqa: E731

    def loop():
        return [eng.encode_ragged_search(sj.SRC_RGB, [planes[k]], [dims[k]], MODE, quant, search[k], METHOD)
                for k in range(args.n)]

    res = batched()
    one = loop()
    same = frames(*res[:3]) == [frames(*r[:3])[0] for r in one]
    got = [len(b) for b in frames(*res[:3])]
    t_b, t_l, t_p = timed(batched, args.regions), timed(loop, args.regions), timed(plain, args.regions)
    px = sum(w * h for w, h in dims)
    print(f"# {args.n} pictures, {px / 1e6:.1f} Mpixels, method {METHOD}, target = q75 size / 2, {PASSES} passes")
    print(f"batched search     median {t_b[0]:9.2f} ms  (min {t_b[1]:.2f}, max {t_b[2]:.2f})")
    print(f"per-picture search median {t_l[0]:9.2f} ms  (min {t_l[1]:.2f}, max {t_l[2]:.2f})")
    print(f"plain ragged batch median {t_p[0]:9.2f} ms  (min {t_p[1]:.2f}, max {t_p[2]:.2f})")
    print(f"speed-up over the loop: {t_l[0] / t_b[0]:.2f}x; bytes equal: {same}")
    print(f"final q: min {min(res[3]):.2f} median {float(np.median(res[3])):.2f} max {max(res[3]):.2f}; "
          f"size / target: median {float(np.median([g / s.target_value for g, s in zip(got, search)])):.3f}")
    print(f"host waits (bound from the contract, not counted): at most {2 * PASSES} per batched call (2 per pass), "
          f"at most {2 * PASSES * args.n} for the loop")
    eng.close()


if __name__ == "__main__":
    main()
