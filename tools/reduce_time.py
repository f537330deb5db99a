#!/usr/bin/env python3
"""What the ragged reduction costs: 32 frames of 3840 x 2160 packed RGB, device-resident, at factor 2, factor 4 and as a
1/2/4/8 pyramid (8 pictures listed at the four factors), on one build:
  (a) the reduce kernel alone (sjpeg_hip_reduce_ragged_src into one buffer): its time and the bytes it moves -- the
      source read once plus the reduced pictures written -- per second, beside the rate a plain device copy of 1 GiB
      reaches on the same box (what tools/hbm_rw.py measures: read + write bytes of y.copy_(x)) and the time that rate
      gives for the kernel's bytes;
  (b) the reduced call (sjpeg_hip_encode_ragged_reduced_src, method 4, 4:2:0, q75) minus the existing _full_ call on
      uint8 pictures reduced beforehand: the same encode with the reduction free.
Median of --regions timed regions of --steps steps each (warm engine, a synchronise at both ends of a region).  The
bytes of (b)'s two routes are compared.
    python tools/reduce_time.py [--frames 32] [--steps 5] [--regions 9]
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 600 python tools/reduce_time.py > profiles/r13/reduce_time.txt"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sjpeg_amd as sj  # noqa: E402
from oracle import synth  # noqa: E402

W, H, Q = 3840, 2160, 75.0


def timed(fn, steps, regions):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / steps * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def copy_rate():
    """read + write bytes per second of a device copy of 1 GiB (tools/hbm_rw.py's `copy` line)"""
    n = 1 << 28
    x = torch.ones(n, dtype=torch.int32, device="cuda")
    y = torch.empty_like(x)
    r = timed(lambda: y.copy_(x), 10, 5)
    return 2 * n * 4 / (r[0] * 1e-3)


def streams(out, sizes, offs):
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    return [host[int(offs[k]):int(offs[k]) + int(sz[k])].tobytes() for k in range(len(sz))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--regions", type=int, default=9)
    args = ap.parse_args()
    F = args.frames
    distinct = min(F, 8)                          # 8 distinct pictures, tiled to F frames (bench.py)
    host = [synth.g_struct(W, H, 7654321 + k) for k in range(distinct)]
    devs = [torch.from_numpy(host[k % distinct]).cuda() for k in range(F)]
    planes = [[d.view(H, W * 3)] for d in devs]
    dims = [(W, H)] * F
    quant = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(Q, quant.ctypes.data)
    eng = sj.Engine(0)
    rate = copy_rate()
    print(f"device: {torch.cuda.get_device_name(0)}; {F} frames of {W}x{H} packed RGB; {args.regions} regions of {args.steps} "
          f"steps; device copy of 1 GiB: {rate / 1e9:.0f} GB/s (read + write bytes)", flush=True)
    bad = 0
    for name, factors in (("factor 2", [2] * F), ("factor 4", [4] * F), ("pyramid 1/2/4/8", [(1, 2, 4, 8)[k % 4] for k in range(F)])):
        rfmt, pics, buf = eng.reduce_ragged(sj.SRC_RGB, planes, dims, factors)
        moved = F * W * H * 3 + int(buf.numel())
        a = timed(lambda: eng.reduce_ragged(sj.SRC_RGB, planes, dims, factors, out=buf), args.steps, args.regions)
        floor = moved / rate * 1e3
        print(f"{name}:", flush=True)
        print(f"  (a) reduce kernel                      median {a[0]:8.4f} ms  (min {a[1]:.4f}, max {a[2]:.4f}); {moved / 1e6:.1f} MB moved, "
              f"{moved / (a[0] * 1e-3) / 1e9:.0f} GB/s; the copy rate gives {floor:.4f} ms: x{a[0] / floor:.2f}", flush=True)
        rplanes = [[p] for p in pics]
        rdims = [(int(p.shape[1]), int(p.shape[0])) for p in pics]
        caps = [sj.frame_bound(w, h, sj.YUV_420, 2048) for (w, h) in rdims]
        offs, at = [], 0
        for c in caps:
            offs.append(at)
            at += (c + 15) & ~15
        out = torch.empty(at, dtype=torch.uint8, device="cuda")
        sizes = torch.zeros(F, dtype=torch.int64, device="cuda")
        plain = timed(lambda: eng.encode_ragged_full(sj.SRC_RGB, rplanes, rdims, sj.YUV_420, quant, 4, capacities=caps, out=out,
                                                     offsets=offs, sizes=sizes), args.steps, args.regions)
        want = streams(out, sizes, offs)
        sizes.zero_()
        red = timed(lambda: eng.encode_ragged_reduced(sj.SRC_RGB, planes, dims, factors, sj.YUV_420, quant, 4, capacities=caps, out=out,
                                                      offsets=offs, sizes=sizes), args.steps, args.regions)
        wrong = sum(1 for p, q in zip(streams(out, sizes, offs), want) if p != q)
        bad += wrong
        print(f"  (b) _full_ call on pre-reduced pictures median {plain[0]:8.4f} ms  (min {plain[1]:.4f}, max {plain[2]:.4f})", flush=True)
        print(f"      reduced call                       median {red[0]:8.4f} ms  (min {red[1]:.4f}, max {red[2]:.4f}); "
              f"difference {red[0] - plain[0]:+.4f} ms; streams that differ: {wrong}", flush=True)
    print(f"streams of the reduced call that differ from the pre-reduced route's: {bad}")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
