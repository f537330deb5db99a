#!/usr/bin/env python3
"""What reading 10-bit video as the decoder wrote it costs, and what it saves: 100 P010 frames of 1920 x 1080, resident
on the device, to 100 JPEGs of 320 x 180 in host memory, BT.709 / limited, method 4, quality 75, three routes on one build:
  (a) sjpeg_amd.video.encode_deep_video_frames: the _yuv16 entry, the 16-bit words read by the resize kernel;
  (b) encode_video_frames on the same frames narrowed to NV12 BEFORE the clock starts: the floor, the 8-bit call;
  (c) the narrowing pass in torch over the full-size planes -- ((x + 128) >> 8).clamp(max=255).to(uint8), ONE pass over
      all frames' Y planes and one over their UV planes, which is the cheapest way to write it -- and then (b): what a
      caller with P010 frames does today.
Median of --regions timed regions of --steps calls each (warm, a synchronise at both ends of a region), the routes
alternating region by region.  The planes (a) makes of frame 0 are compared with the contract in numpy (the ratio is
whole: a box sum).
    python tools/yuv16_time.py [--frames 100] [--steps 3] [--regions 11]
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 300 python tools/yuv16_time.py > profiles/yuv16_time.txt"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sjpeg_amd as sj  # noqa: E402
import sjpeg_amd.video as sv  # noqa: E402
import yuv_colour_model as cm  # noqa: E402

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


def narrow(x):
    """the pass a caller writes today: 16-bit words (int16 bits) to bytes, each sample rounded on its own"""
    return (((x.to(torch.int32) & 0xffff) + 128) >> 8).clamp(max=255).to(torch.uint8)


def box(plane, w2, h2, shift):
    """the contract where the ratio is whole, vectorised"""
    h, w = plane.shape
    fy, fx = h // h2, w // w2
    s = plane.astype(np.int64).reshape(h2, fy, w2, fx).sum((1, 3))
    a = fy * fx
    return np.minimum(255, (2 * s + (a << shift)) // (a << (shift + 1))).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=11)
    args = ap.parse_args()
    n = args.frames
    rs = np.random.RandomState(2010)
    # studio-range 10-bit luma with some noise on it, in the high bits of the word as P010 has it
    ramp = (64 + np.add.outer(np.arange(H), np.arange(W)) // 4 % 876).astype(np.int64)
    y16 = np.empty((n, H, W), np.uint16)
    uv16 = np.empty((n, H // 2, W), np.uint16)
    for k in range(n):
        y16[k] = np.clip(ramp + rs.randint(-24, 25, (H, W)) + 4 * (k % 8), 0, 1023).astype(np.uint16) << 6
        uv16[k] = rs.randint(384, 640, (H // 2, W)).astype(np.uint16) << 6
    # all frames' planes in one tensor each, so that route (c) can narrow them in one pass; a frame is a view
    dy, duv = torch.from_numpy(y16.view(np.int16)).cuda(), torch.from_numpy(uv16.view(np.int16)).cuda()
    deep = [(dy[k], duv[k]) for k in range(n)]
    ny, nuv = narrow(dy), narrow(duv)
    narrowed = [(ny[k], nuv[k]) for k in range(n)]
    eng = sj.Engine(0)
    sizes = [(W2, H2)] * n
    hd = sv.VideoColour("bt709", "limited")
    print(f"device: {torch.cuda.get_device_name(0)}; {n} P010 frames {W}x{H} on the device -> {W2}x{H2} JPEGs on the host; "
          f"{args.regions} regions of {args.steps} calls", flush=True)

    def today():
        py, puv = narrow(dy), narrow(duv)
        return sv.encode_video_frames([(py[k], puv[k]) for k in range(n)], sj.SRC_NV12, hd, sizes=sizes, engine=eng)

    routes = [lambda: sv.encode_deep_video_frames(deep, sj.SRC_NV12, hd, sizes=sizes, engine=eng, depth=sv.VideoDepth.P010),
              lambda: sv.encode_video_frames(narrowed, sj.SRC_NV12, hd, sizes=sizes, engine=eng),
              today]
    a, b, c = timed(routes, args.steps, args.regions)
    ja, jb, jc = (fn() for fn in routes)
    _, got, _ = sv.convert_deep_frames(deep[:1], sj.SRC_NV12, hd, sizes=sizes[:1], engine=eng)
    torch.cuda.synchronize()
    uv = uv16[0].reshape(H // 2, W // 2, 2)
    made = [box(y16[0], W2, H2, 8), box(uv[:, :, 0], W2 // 2, H2 // 2, 8), box(uv[:, :, 1], W2 // 2, H2 // 2, 8)]
    want = cm.convert_planes(*made, cm.BT709, cm.LIMITED)
    wrong = sum(0 if np.array_equal(g.cpu().numpy(), w) else 1 for g, w in zip(got[0], want))
    print(f"  (a) encode_deep_video_frames, P010 as it is     median {a[0]:8.3f} ms/call  (min {a[1]:.3f}, max {a[2]:.3f})", flush=True)
    print(f"  (b) encode_video_frames, narrowed beforehand    median {b[0]:8.3f} ms/call  (min {b[1]:.3f}, max {b[2]:.3f}); (a) / (b) = {a[0] / b[0]:.3f}",
          flush=True)
    print(f"  (c) the torch narrowing pass, then (b)          median {c[0]:8.3f} ms/call  (min {c[1]:.3f}, max {c[2]:.3f}); (a) / (c) = {a[0] / c[0]:.3f}",
          flush=True)
    print(f"  JPEG bytes a call: (a) {sum(len(j) for j in ja)}, (b) {sum(len(j) for j in jb)}; (c) equals (b): {jc == jb}; "
          f"planes of (a) that differ from the contract (frame 0): {wrong}", flush=True)
    return 0 if wrong == 0 and jc == jb else 1


if __name__ == "__main__":
    sys.exit(main())
