#!/usr/bin/env python3
"""What the video colour conversion adds to a thumbnail call: 100 NV12 frames of 1920 x 1080, resident on the device, to
100 JPEGs of 320 x 180 in host memory, method 4, quality 75, three routes on one build:
  (r) encode_yuv_frames: the _yuv_resized_ entry, the samples coded as they are -- the parent's call, unchanged;
  (c) sjpeg_amd.video.encode_video_frames with VideoColour("bt709", "limited"): the same plus the colour launch;
  (i) encode_video_frames with VideoColour("bt601", "full"): the identity, which is route (r) by another name.
Median of --regions timed regions of --steps calls each (warm, a synchronise at both ends of a region), the routes
alternating region by region.  The planes of (c) are compared with the numpy model on frame 0.
    python tools/yuv_colour_time.py [--frames 100] [--steps 3] [--regions 11]
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 300 python tools/yuv_colour_time.py > profiles/yuv_colour_time.txt"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=11)
    args = ap.parse_args()
    n = args.frames
    rs = np.random.RandomState(709)
    # studio-range luma with some noise on it, as decoded frames are; the content does not change what the launches do
    ramp = (16 + np.add.outer(np.arange(H), np.arange(W)) // 14 % 220).astype(np.int64)
    frames = []
    for k in range(n):
        y = np.clip(ramp + rs.randint(-6, 7, (H, W)) + k % 8, 0, 255).astype(np.uint8)
        uv = rs.randint(96, 160, (H // 2, W)).astype(np.uint8)
        frames.append((torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()))
    eng = sj.Engine(0)
    sizes = [(W2, H2)] * n
    hd, ident = sv.VideoColour("bt709", "limited"), sv.VideoColour("bt601", "full")
    print(f"device: {torch.cuda.get_device_name(0)}; {n} NV12 frames {W}x{H} on the device -> {W2}x{H2} JPEGs on the host; "
          f"{args.regions} regions of {args.steps} calls", flush=True)
    routes = [lambda: sj.encode_yuv_frames(frames, sj.SRC_NV12, sizes=sizes, engine=eng),
              lambda: sv.encode_video_frames(frames, sj.SRC_NV12, hd, sizes=sizes, engine=eng),
              lambda: sv.encode_video_frames(frames, sj.SRC_NV12, ident, sizes=sizes, engine=eng)]
    r, c, i = timed(routes, args.steps, args.regions)
    plain, conv, same = (fn() for fn in routes)
    _, pics, _ = eng.resize_ragged_yuv(sj.SRC_NV12, [list(frames[0])], [(W, H)], sizes[:1])
    _, got, _ = sv.convert_yuv_frames(frames[:1], sj.SRC_NV12, hd, sizes=sizes[:1], engine=eng)
    torch.cuda.synchronize()
    want = cm.convert_planes(*[p.cpu().numpy() for p in pics[0]], cm.BT709, cm.LIMITED)
    wrong = sum(0 if np.array_equal(g.cpu().numpy(), w) else 1 for g, w in zip(got[0], want))
    print(f"  (r) encode_yuv_frames, no conversion          median {r[0]:8.3f} ms/call  (min {r[1]:.3f}, max {r[2]:.3f})", flush=True)
    print(f"  (c) encode_video_frames, BT.709 limited       median {c[0]:8.3f} ms/call  (min {c[1]:.3f}, max {c[2]:.3f}); (c) / (r) = {c[0] / r[0]:.3f}",
          flush=True)
    print(f"  (i) encode_video_frames, the identity         median {i[0]:8.3f} ms/call  (min {i[1]:.3f}, max {i[2]:.3f}); (i) / (r) = {i[0] / r[0]:.3f}",
          flush=True)
    print(f"  JPEG bytes a call: (r) {sum(len(j) for j in plain)}, (c) {sum(len(j) for j in conv)}; (i) equals (r): {same == plain}; "
          f"planes of (c) that differ from the model (frame 0): {wrong}", flush=True)
    return 0 if wrong == 0 and same == plain else 1


if __name__ == "__main__":
    sys.exit(main())
