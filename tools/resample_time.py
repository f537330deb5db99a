#!/usr/bin/env python3
"""What Pillow's filters cost inside the ragged call, and what they save: 100 RGB frames of 1920 x 1080, resident on the
device, to 100 JPEGs of 320 x 180 in host memory, method 4, quality 75, 4:2:0:
  (a) sjpeg_amd.resample.encode_resampled_images with LANCZOS and (b) with BICUBIC: the _resampled entry;
  (c) Engine.encode_ragged_flattened without a flatten on the same frames: the area average;
  (d) the detour a caller takes today: per picture a float interpolate(mode="bicubic", antialias=True),
      round().clamp().to(uint8), and then encode_images on the made pictures -- close to Pillow, not equal;
and the pictures alone:
  (e) sjpeg_amd.resample.resample_images with LANCZOS, (f) with BICUBIC, (g) resize_images, (h) the detour's resize step.
Median of --regions timed regions of --steps calls each (warm, a synchronise at both ends of a region), the routes
alternating region by region.  The picture (e) makes of frame 0 is compared with the definition in numpy
(tests/resample_model.py).
    python tools/resample_time.py [--frames 100] [--steps 3] [--regions 11] [--tree DIR]
--tree DIR: import sjpeg_amd from another checkout of this repository, built there -- the parent commit's, as the
baseline of (c); a tree without sjpeg_amd.resample measures (c) and (g) alone.
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 300 python tools/resample_time.py > profiles/resample_time.txt"""
import argparse
import os
import sys
import time

import numpy as np
import torch

W, H, W2, H2 = 1920, 1080, 320, 180
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def line(tag, what, t, extra=""):
    print(f"  ({tag}) {what:<52} median {t[0]:8.3f} ms/call  (min {t[1]:.3f}, max {t[2]:.3f}){extra}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=11)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import sjpeg_amd as sj
    try:
        import sjpeg_amd.resample as rs
    except ImportError:
        rs = None
    n = args.frames
    gen = torch.Generator(device="cuda").manual_seed(2012)
    # a ramp with noise on it and some full-scale speckle: detail that survives the filter, so the windows have work
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

    def area_coded():
        out, szs, offs, _, _, _ = eng.encode_ragged_flattened(sj.SRC_RGB, planes, dims, None, sizes, None, sj.YUV_420, quant, 4)
        eng.wait()
        return sj._fetch_ragged(out, szs, offs)

    def area_made():
        return sj.resize_images(frames, sizes, engine=eng)

    if rs is None:
        c, g = timed([area_coded, area_made], args.steps, args.regions)
        line("c", "the area-average call", c)
        line("g", "resize_images: the pictures alone", g)
        return 0

    def lanczos():
        return rs.encode_resampled_images(frames, sizes, filter=rs.Filter.LANCZOS, engine=eng)

    def bicubic():
        return rs.encode_resampled_images(frames, sizes, filter=rs.Filter.BICUBIC, engine=eng)

    def torch_resize():
        out = []
        for f in frames:
            x = torch.nn.functional.interpolate(f.permute(2, 0, 1).unsqueeze(0).float(), size=(H2, W2), mode="bicubic", antialias=True)
            out.append(x.round().clamp(0, 255).to(torch.uint8).squeeze(0).permute(1, 2, 0).contiguous())
        return out

    def detour():
        return sj.encode_images(torch_resize(), 75.0, sj.YUV_420, engine=eng, method=4)

    def lanczos_made():
        return rs.resample_images(frames, sizes, rs.Filter.LANCZOS, engine=eng)

    def bicubic_made():
        return rs.resample_images(frames, sizes, rs.Filter.BICUBIC, engine=eng)

    routes = [lanczos, bicubic, area_coded, detour, lanczos_made, bicubic_made, area_made, torch_resize]
    a, b, c, d, e, f, g, h = timed(routes, args.steps, args.regions)
    ja, jb, jc, jd = (fn() for fn in routes[:4])
    torch.cuda.synchronize()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import resample_model as rm
    got = lanczos_made()[0].cpu().numpy()
    wrong = int((got != rm.resample(frames[0].cpu().numpy(), (W2, H2), rm.LANCZOS)).sum())
    line("a", "encode_resampled_images, LANCZOS", a)
    line("b", "encode_resampled_images, BICUBIC", b)
    line("c", "the area-average call", c, f"; (a) / (c) = {a[0] / c[0]:.3f}, (b) / (c) = {b[0] / c[0]:.3f}")
    line("d", "torch bicubic antialias, round, encode_images", d, f"; (b) / (d) = {b[0] / d[0]:.3f}")
    line("e", "resample_images, LANCZOS: the pictures alone", e)
    line("f", "resample_images, BICUBIC: the pictures alone", f)
    line("g", "resize_images: the pictures alone", g, f"; (e) / (g) = {e[0] / g[0]:.2f}, (f) / (g) = {f[0] / g[0]:.2f}")
    line("h", "the detour's resize step alone", h, f"; (f) / (h) = {f[0] / h[0]:.3f}")
    print(f"  JPEG bytes a call: (a) {sum(len(j) for j in ja)}, (b) {sum(len(j) for j in jb)}, (c) {sum(len(j) for j in jc)}, "
          f"(d) {sum(len(j) for j in jd)}; samples of (e) that differ from the definition (frame 0): {wrong}", flush=True)
    return 0 if wrong == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
