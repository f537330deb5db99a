#!/usr/bin/env python3
"""What thumbnails of decoded video cost, host to host: 32 NV12 frames of 1920 x 1080 in pinned host memory to 32 JPEGs
of 320 x 180 in host memory, method 4, quality 75, two routes on one build:
  (a) encode_yuv_frames: the frames copied to the device as they are, then ONE call -- the resize kernel over the tiles
      of every plane (the UV plane read once, stored as two) and one inner encode of the planar 4:2:0 thumbnails;
  (b) what there was before: the same copies, then per plane torch.nn.functional.interpolate(mode="area") on a float
      copy + round + uint8 (U and V de-interleaved first), then encode_ragged_full of the planes as SRC_YUV420.
Median of --regions timed regions of --steps calls each (warm, a synchronise at both ends of a region), the two routes
alternating region by region.  The two round differently (exact integers against floats), so the JPEGs are not
compared; the planes of (a) are, against numpy on the first frame.
    python tools/yuv_resize_time.py [--frames 32] [--steps 3] [--regions 11]
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 300 python tools/yuv_resize_time.py > profiles/yuv_resize_time.txt"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sjpeg_amd as sj  # noqa: E402

W, H, W2, H2 = 1920, 1080, 320, 180


def region(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def timed(fns, steps, regions):
    for fn in fns:
        for _ in range(2):
            fn()
    ts = [[] for _ in fns]
    for _ in range(regions):
        for k, fn in enumerate(fns):
            ts[k].append(region(fn, steps))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


def area(b, w2, h2):
    """the contract of sjpeg_hip.h on a plane, in numpy: sums in int64, round half up"""
    def weights(n_src, n_dst):
        x, xo = np.arange(n_src, dtype=np.int64)[None, :], np.arange(n_dst, dtype=np.int64)[:, None]
        return np.maximum(0, np.minimum((x + 1) * n_dst, (xo + 1) * n_src) - np.maximum(x * n_dst, xo * n_src))
    h, w = b.shape
    S = (weights(h, h2) @ b.astype(np.int64)) @ weights(w, w2).T
    return ((2 * S + w * h) // (2 * w * h)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=11)
    args = ap.parse_args()
    n = args.frames
    rs = np.random.RandomState(1080)
    # smooth luma with some noise on it, as decoded frames are; the content does not change what the resize does
    ramp = (np.add.outer(np.arange(H), np.arange(W)) // 12 % 256).astype(np.int64)
    host = []
    for k in range(n):
        y = np.clip(ramp + rs.randint(-12, 13, (H, W)) + 3 * k, 0, 255).astype(np.uint8)
        uv = rs.randint(96, 160, (H // 2, W)).astype(np.uint8)
        host.append((torch.from_numpy(y).pin_memory(), torch.from_numpy(uv).pin_memory()))
    eng = sj.Engine(0)
    dims, sizes = [(W, H)] * n, [(W2, H2)] * n
    quant = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(75.0, quant.ctypes.data)
    print(f"device: {torch.cuda.get_device_name(0)}; {n} NV12 frames {W}x{H} -> {W2}x{H2}, host to host; {args.regions} regions of "
          f"{args.steps} calls", flush=True)

    def upload():
        return [(y.cuda(non_blocking=True), uv.cuda(non_blocking=True)) for (y, uv) in host]

    def ours():
        return sj.encode_yuv_frames(upload(), sj.SRC_NV12, sizes=sizes, engine=eng)

    def torch_route():
        planes = []
        for (y, uv) in upload():
            pair = uv.view(H // 2, W // 2, 2)
            made = []
            for p, (w2, h2) in ((y, (W2, H2)), (pair[..., 0], (W2 // 2, H2 // 2)), (pair[..., 1], (W2 // 2, H2 // 2))):
                x = F.interpolate(p.float()[None, None], size=(h2, w2), mode="area")
                made.append(x.round().clamp(0, 255).to(torch.uint8)[0, 0])
            planes.append(made)
        out, sz, offs, _, _, _ = eng.encode_ragged_full(sj.SRC_YUV420, planes, sizes, sj.YUV_420, quant, 4)
        eng.wait()
        return sj._fetch_ragged(out, sz, offs)

    a, b = timed([ours, torch_route], args.steps, args.regions)
    jpegs, theirs = ours(), torch_route()
    _, pics, _ = eng.resize_ragged_yuv(sj.SRC_NV12, [list(f) for f in upload()[:1]], dims[:1], sizes[:1])
    torch.cuda.synchronize()
    y, uv = host[0][0].numpy(), host[0][1].numpy().reshape(H // 2, W // 2, 2)
    want = [area(y, W2, H2), area(uv[..., 0], W2 // 2, H2 // 2), area(uv[..., 1], W2 // 2, H2 // 2)]
    wrong = sum(0 if np.array_equal(p.cpu().numpy(), w) else 1 for p, w in zip(pics[0], want))
    print(f"  (a) encode_yuv_frames                              median {a[0]:9.3f} ms/call  (min {a[1]:.3f}, max {a[2]:.3f}); "
          f"{n / a[0] * 1e3:.0f} frames/s", flush=True)
    print(f"  (b) torch area + round per plane, encode_ragged_full median {b[0]:9.3f} ms/call  (min {b[1]:.3f}, max {b[2]:.3f}); "
          f"(b) / (a) = {b[0] / a[0]:.2f}", flush=True)
    print(f"  JPEG bytes a call: (a) {sum(len(j) for j in jpegs)}, (b) {sum(len(j) for j in theirs)}; planes of (a) that differ from "
          f"numpy (frame 0): {wrong}", flush=True)
    return 0 if wrong == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
