#!/usr/bin/env python3
"""What averaging in linear light costs inside the ragged call, and what it saves: 100 RGB frames of 1920 x 1080,
resident on the device, to 100 JPEGs of 320 x 180 in host memory, method 4, quality 75, 4:2:0, three routes:
  (a) sjpeg_amd.light.encode_linear_images: the _linear entry, the bytes taken to light where the resize kernel stages them;
  (b) Engine.encode_ragged_flattened without a flatten on the same frames: the coded-light call, the average of the bytes;
  (c) the detour a caller takes today, per picture in torch -- float, the sRGB curve by pow, interpolate(mode="area"), the
      curve back by pow, round().clamp().to(uint8) -- and then encode_images on the made pictures.
Median of --regions timed regions of --steps calls each (warm, a synchronise at both ends of a region), the routes
alternating region by region.  The picture (a) makes of frame 0 is compared with the contract in numpy (the ratio is
whole: a box sum).
    python tools/linear_time.py [--frames 100] [--steps 3] [--regions 11] [--tree DIR]
--tree DIR: import sjpeg_amd from another checkout of this repository, built there -- the parent commit's, as the
baseline of (b); a tree without sjpeg_amd.light measures (b) alone.
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 300 python tools/linear_time.py > profiles/linear_time.txt"""
import argparse
import os
import sys
import time

import numpy as np
import torch

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


def box_linear(im, w2, h2):
    """the contract where the ratio is whole, vectorised: the table, the box sums, the count of midpoints reached"""
    c = np.arange(256) / 255.0
    T = np.floor(65535.0 * np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4) + 0.5).astype(np.int64)
    h, w = im.shape[:2]
    fy, fx = h // h2, w // w2
    S = T[im].reshape(h2, fy, w2, fx, -1).sum((1, 3))
    return (2 * S[..., None] >= (T[:-1] + T[1:]) * (fy * fx)).sum(-1).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=11)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import sjpeg_amd as sj
    try:
        import sjpeg_amd.light as li
    except ImportError:
        li = None
    n = args.frames
    gen = torch.Generator(device="cuda").manual_seed(2011)
    # a ramp with noise on it and some full-scale speckle: fine detail, which is where the two averages differ
    ramp = (torch.arange(H, device="cuda")[:, None, None] + torch.arange(W, device="cuda")[None, :, None] // 2 +
            40 * torch.arange(3, device="cuda")[None, None, :]) % 256
    frames = []
    for k in range(n):
        noise = torch.randint(-24, 25, (H, W, 3), device="cuda", generator=gen)
        speck = torch.randint(0, 16, (H, W, 1), device="cuda", generator=gen) == 0
        frames.append(torch.where(speck, 255, (ramp + noise + 4 * (k % 8)).clamp(0, 255)).to(torch.uint8).contiguous())
    planes = [[f.view(H, W * 3)] for f in frames]
    dims, sizes = [(W, H)] * n, [(W2, H2)] * n
    eng = sj.Engine(0)
    quant = sj._quality_quant([75.0] * n)
    print(f"device: {torch.cuda.get_device_name(0)}; tree {os.path.abspath(args.tree)}; {n} RGB frames {W}x{H} on the device -> "
          f"{W2}x{H2} JPEGs on the host; {args.regions} regions of {args.steps} calls", flush=True)

    def linear():
        return li.encode_linear_images(frames, sizes, engine=eng)

    def coded():
        out, szs, offs, _, _, _ = eng.encode_ragged_flattened(sj.SRC_RGB, planes, dims, None, sizes, None, sj.YUV_420, quant, 4)
        eng.wait()
        return sj._fetch_ragged(out, szs, offs)

    def curve(x):
        return torch.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)

    def back(y):
        return torch.where(y <= 0.0031308, y * 12.92, 1.055 * y ** (1 / 2.4) - 0.055)

    def detour():
        made = []
        for f in frames:
            lin = curve(f.permute(2, 0, 1).unsqueeze(0).float() / 255.0)
            small = torch.nn.functional.interpolate(lin, size=(H2, W2), mode="area")
            made.append((back(small) * 255.0).round().clamp(0, 255).to(torch.uint8).squeeze(0).permute(1, 2, 0).contiguous())
        return sj.encode_images(made, 75.0, sj.YUV_420, engine=eng, method=4)

    if li is None:
        (b,) = timed([coded], args.steps, args.regions)
        print(f"  (b) the coded-light call                        median {b[0]:8.3f} ms/call  (min {b[1]:.3f}, max {b[2]:.3f})", flush=True)
        return 0
    routes = [linear, coded, detour]
    a, b, c = timed(routes, args.steps, args.regions)
    ja, jb, jc = (fn() for fn in routes)
    got = li.linear_resize_images(frames[:1], sizes[:1], engine=eng)[0].cpu().numpy()
    wrong = int((got != box_linear(frames[0].cpu().numpy(), W2, H2)).sum())
    print(f"  (a) encode_linear_images, linear light          median {a[0]:8.3f} ms/call  (min {a[1]:.3f}, max {a[2]:.3f})", flush=True)
    print(f"  (b) the coded-light call                        median {b[0]:8.3f} ms/call  (min {b[1]:.3f}, max {b[2]:.3f}); (a) / (b) = {a[0] / b[0]:.3f}",
          flush=True)
    print(f"  (c) the torch detour, then encode_images        median {c[0]:8.3f} ms/call  (min {c[1]:.3f}, max {c[2]:.3f}); (a) / (c) = {a[0] / c[0]:.3f}",
          flush=True)
    print(f"  JPEG bytes a call: (a) {sum(len(j) for j in ja)}, (b) {sum(len(j) for j in jb)}, (c) {sum(len(j) for j in jc)}; "
          f"samples of (a) that differ from the contract (frame 0): {wrong}", flush=True)
    return 0 if wrong == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
