#!/usr/bin/env python3
"""What sharpening costs inside the ragged call, and what it saves: 100 RGB frames of 1920 x 1080, resident on the
device, to 100 JPEGs of 320 x 180 in host memory, method 4, quality 75, 4:2:0, three routes:
  (a) sjpeg_amd.unsharp.encode_unsharp_images: the _unsharp entry, one more small launch over the made thumbnails;
  (b) Engine.encode_ragged_flattened without a flatten on the same frames: the thumbnails unsharpened;
  (c) the detour a caller takes today: resize_images, then per picture in torch a float conv2d with the 3 x 3 kernel
      (edge replicated), p + amount / 32 (p - blur), round().clamp().to(uint8), and then encode_images on the made pictures.
and, to separate the filter's cost from the entropy coder's (sharpened pictures code to more bytes), the pictures alone:
  (d) sjpeg_amd.unsharp.unsharp_ragged against (e) Engine.orient_ragged.
Median of --regions timed regions of --steps calls each (warm, a synchronise at both ends of a region), the routes
alternating region by region.  The picture (d) makes of frame 0 is compared with the contract in numpy.
    python tools/unsharp_time.py [--frames 100] [--steps 3] [--regions 11] [--tree DIR]
--tree DIR: import sjpeg_amd from another checkout of this repository, built there -- the parent commit's, as the
baseline of (b); a tree without sjpeg_amd.unsharp measures (b) and (e) alone.
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 300 python tools/unsharp_time.py > profiles/unsharp_time.txt"""
import argparse
import os
import sys
import time

import numpy as np
import torch

W, H, W2, H2 = 1920, 1080, 320, 180
AMOUNT, THRESHOLD = 32, 0


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


def area(im, w2, h2):
    """the exact area average where the ratio is whole: box sums rounded half up"""
    h, w = im.shape[:2]
    fy, fx = h // h2, w // w2
    S = im.astype(np.int64).reshape(h2, fy, w2, fx, -1).sum((1, 3))
    return ((2 * S + fy * fx) // (2 * fy * fx)).astype(np.uint8)


def unsharp(b, amount, threshold):
    """the contract, vectorised"""
    p = b.astype(np.int64)
    h, w = p.shape[:2]
    e = np.pad(p, ((1, 1), (1, 1), (0, 0)), mode="edge")
    S = sum(wi * wj * e[i:i + h, j:j + w] for i, wi in enumerate((1, 2, 1)) for j, wj in enumerate((1, 2, 1)))
    D = 16 * p - S
    v = np.clip((512 * p + amount * D + 256) >> 9, 0, 255)
    return np.where(np.abs(D) < 16 * threshold, p, v).astype(np.uint8)


def line(tag, what, t, extra=""):
    print(f"  ({tag}) {what:<46} median {t[0]:8.3f} ms/call  (min {t[1]:.3f}, max {t[2]:.3f}){extra}", flush=True)


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
        import sjpeg_amd.unsharp as un
    except ImportError:
        un = None
    n = args.frames
    gen = torch.Generator(device="cuda").manual_seed(2012)
    # a ramp with noise on it and some full-scale speckle: detail that survives the average, so the filter has work
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

    def coded():
        out, szs, offs, _, _, _ = eng.encode_ragged_flattened(sj.SRC_RGB, planes, dims, None, sizes, None, sj.YUV_420, quant, 4)
        eng.wait()
        return sj._fetch_ragged(out, szs, offs)

    def made():
        return eng.orient_ragged(sj.SRC_RGB, planes, dims, sizes, None)[1]

    if un is None:
        b, e = timed([coded, made], args.steps, args.regions)
        line("b", "the unsharpened call", b)
        line("e", "orient_ragged: the pictures alone", e)
        return 0
    u = un.Unsharp(AMOUNT, THRESHOLD)
    kernel = (torch.tensor([[1., 2., 1.], [2., 4., 2.], [1., 2., 1.]], device="cuda") / 16.0).reshape(1, 1, 3, 3).repeat(3, 1, 1, 1)

    def sharpened():
        return un.encode_unsharp_images(frames, sizes, unsharp=u, engine=eng)

    def detour():
        out = []
        for p in sj.resize_images(frames, sizes, engine=eng):
            x = p.permute(2, 0, 1).unsqueeze(0).float()
            blur = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), kernel, groups=3)
            out.append((x + (AMOUNT / 32.0) * (x - blur)).round().clamp(0, 255).to(torch.uint8).squeeze(0).permute(1, 2, 0).contiguous())
        return sj.encode_images(out, 75.0, sj.YUV_420, engine=eng, method=4)

    def made_sharp():
        return un.unsharp_ragged(eng, sj.SRC_RGB, planes, dims, sizes, unsharp=u)[1]

    routes = [sharpened, coded, detour, made_sharp, made]
    a, b, c, d, e = timed(routes, args.steps, args.regions)
    ja, jb, jc = (fn() for fn in routes[:3])
    torch.cuda.synchronize()
    got = made_sharp()[0].cpu().numpy()
    wrong = int((got != unsharp(area(frames[0].cpu().numpy(), W2, H2), AMOUNT, THRESHOLD)).sum())
    line("a", "encode_unsharp_images", a)
    line("b", "the unsharpened call", b, f"; (a) / (b) = {a[0] / b[0]:.3f}")
    line("c", "resize_images, torch unsharp, encode_images", c, f"; (a) / (c) = {a[0] / c[0]:.3f}")
    line("d", "unsharp_ragged: the sharpened pictures alone", d)
    line("e", "orient_ragged: the pictures alone", e, f"; (d) - (e) = {d[0] - e[0]:.3f} ms")
    print(f"  JPEG bytes a call: (a) {sum(len(j) for j in ja)}, (b) {sum(len(j) for j in jb)}, (c) {sum(len(j) for j in jc)}; "
          f"samples of (d) that differ from the contract (frame 0): {wrong}", flush=True)
    return 0 if wrong == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
