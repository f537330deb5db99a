#!/usr/bin/env python3
"""What the ragged resize costs: 64 packed RGB pictures, device-resident, with sizes drawn around 4000 x 3000, fitted
into a 256 x 256 box and into a 1024 x 1024 box (sjpeg_hip_fit_size), on one build:
  (a) resize_images: the resize kernel, one launch for the batch;
  (b) what users run today, per picture: interpolate(mode="area") on a float copy, then round().clamp().to(uint8);
  (c) reduce_images at the nearest integer factor: the existing kernel reads the same source bytes, so it is the
      yardstick for the traffic (its pictures have other sizes: it is timed, not compared);
  (d) the source bytes over the HBM read bandwidth bench.py prices its roofline with (8.0e12 B/s): the floor.
Median of --regions timed regions of --steps steps each (warm, a synchronise at both ends of a region), the two
routes alternating region by region.  (a)'s pictures are compared with numpy on the first pictures of the batch, and
with (b)'s: the two round differently (float against exact), so the count of bytes that differ is printed, not
asserted.
    python tools/resize_time.py [--frames 64] [--steps 3] [--regions 11]
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 600 python tools/resize_time.py > profiles/r15/resize_time.txt"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sjpeg_amd as sj  # noqa: E402

HBM_PEAK = 8.0e12          # B/s: bench.py's


def region(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def timed(fns, steps, regions):
    """median, min and max of `regions` regions for each of fns, the routes alternating"""
    for fn in fns:
        for _ in range(2):
            fn()
    ts = [[] for _ in fns]
    for _ in range(regions):
        for k, fn in enumerate(fns):
            ts[k].append(region(fn, steps))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


def area(b, w2, h2):
    """the contract of sjpeg_hip.h in numpy: the sums in float64 (integers below 2^53 all the way: exact), the rounding
    in int64"""
    def weights(n_src, n_dst):
        x, xo = np.arange(n_src, dtype=np.int64)[None, :], np.arange(n_dst, dtype=np.int64)[:, None]
        return np.maximum(0, np.minimum((x + 1) * n_dst, (xo + 1) * n_src) - np.maximum(x * n_dst, xo * n_src))
    H, W = b.shape[:2]
    wy, wx = weights(H, h2), weights(W, w2)
    wy, wx = wy.astype(np.float64), wx.astype(np.float64)
    S = np.stack([(wy @ b[..., c].astype(np.float64)) @ wx.T for c in range(3)], axis=-1).astype(np.int64)
    return ((2 * S + W * H) // (2 * W * H)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=11)
    args = ap.parse_args()
    n = args.frames
    rs = np.random.RandomState(20240)
    dims = [(int(rs.randint(3600, 4400)), int(rs.randint(2700, 3300))) for _ in range(n)]
    # (random bytes made on the device: the content does not change what the kernels do)
    g = torch.Generator(device="cuda").manual_seed(7)
    devs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda", generator=g) for (w, h) in dims]
    src_bytes = sum(3 * w * h for (w, h) in dims)
    eng = sj.Engine(0)
    print(f"device: {torch.cuda.get_device_name(0)}; {n} packed RGB pictures, {min(d[0] for d in dims)}..{max(d[0] for d in dims)} x "
          f"{min(d[1] for d in dims)}..{max(d[1] for d in dims)}, {src_bytes / 1e6:.0f} MB; {args.regions} regions of {args.steps} steps",
          flush=True)
    bad = 0
    for box in (256, 1024):
        sizes = [sj.fit_size(w, h, (box, box)) for (w, h) in dims]
        factors = [max(1, min(8, int(round(w / s[0])))) for (w, h), s in zip(dims, sizes)]

        def ours():
            return sj.resize_images(devs, sizes, engine=eng)

        def torch_area():
            out = []
            for d, (w2, h2) in zip(devs, sizes):
                x = d.permute(2, 0, 1).unsqueeze(0).float()
                out.append(F.interpolate(x, size=(h2, w2), mode="area").round().clamp(0, 255).to(torch.uint8))
            return out

        def reduce():
            return sj.reduce_images(devs, factors, engine=eng)

        a, b, c = timed([ours, torch_area, reduce], args.steps, args.regions)
        floor = src_bytes / HBM_PEAK * 1e3
        got, theirs = ours(), torch_area()
        torch.cuda.synchronize()
        wrong = sum(0 if np.array_equal(got[k].cpu().numpy(), area(devs[k].cpu().numpy(), *sizes[k])) else 1 for k in range(min(n, 2)))
        bad += wrong
        differ = sum(int((got[k].permute(2, 0, 1) != theirs[k][0]).sum()) for k in range(n))
        total = sum(3 * w2 * h2 for (w2, h2) in sizes)
        print(f"box {box}: sizes {sizes[0][0]}x{sizes[0][1]}, {sizes[1][0]}x{sizes[1][1]}, ...; factors of (c): {sorted(set(factors))}", flush=True)
        print(f"  (a) resize_images                 median {a[0]:9.4f} ms  (min {a[1]:.4f}, max {a[2]:.4f}); {src_bytes / (a[0] * 1e-3) / 1e9:.0f} GB/s of source", flush=True)
        print(f"  (b) torch area + round, a picture  median {b[0]:9.4f} ms  (min {b[1]:.4f}, max {b[2]:.4f}); (b) / (a) = {b[0] / a[0]:.2f}", flush=True)
        print(f"  (c) reduce_images                 median {c[0]:9.4f} ms  (min {c[1]:.4f}, max {c[2]:.4f}); (a) / (c) = {a[0] / c[0]:.2f}", flush=True)
        print(f"  (d) source bytes at 8.0 TB/s              {floor:9.4f} ms; (a) / (d) = {a[0] / floor:.2f}", flush=True)
        print(f"  pictures of (a) that differ from numpy (first {min(n, 2)}): {wrong}; bytes of (a) that differ from (b)'s: {differ} of {total}", flush=True)
    print(f"pictures of the resize kernel that differ from numpy: {bad}")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
