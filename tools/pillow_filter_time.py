#!/usr/bin/env python3
"""What Pillow's UnsharpMask and GaussianBlur cost inside the ragged call, and the detour they replace: 100 RGB frames
of 1920 x 1080, resident on the device, to the box 320 x 180 -- 100 JPEGs in host memory, method 4, quality 75, 4:2:0:
  (a) sjpeg_amd.resample.encode_thumbnails(post=PillowFilter.unsharp_mask()): thumbnail, UnsharpMask(2, 150, 3), encode;
  (b) encode_thumbnails(post=PillowFilter.gaussian_blur(8)): a blurred placeholder;
  (c) encode_thumbnails without post: the _resampled_box_ call;
  (d) Engine.encode_ragged_flattened without a flatten on the same frames: the area average (the _flattened_ call);
and the pictures alone:
  (e) thumbnail_images(post=unsharp_mask()), (f) thumbnail_images(post=gaussian_blur(8)), (g) thumbnail_images;
and, where Pillow is importable, the detour:
  (h) thumbnail_images, copy to the host, PIL.ImageFilter.UnsharpMask per picture on one core, copy back, encode_images.
Median of --regions timed regions of --steps calls each (warm, a synchronise at both ends of a region), the routes
alternating region by region.  The pictures (e) and (f) make of frame 0 are compared with the definition in numpy
(tests/pillow_filter_model.py), and (h)'s JPEGs with (a)'s.
    python tools/pillow_filter_time.py [--frames 100] [--steps 3] [--regions 11] [--tree DIR] [--baseline]
--tree DIR: import sjpeg_amd from another checkout of this repository, built there -- the parent commit's, as the
baseline of (c) and (d); a tree without post= measures those and (g) alone, and --baseline measures this tree the same
way: a process with the same routes in it, which is what the two builds are compared by.
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 300 python tools/pillow_filter_time.py > profiles/pillow_filter_time.txt"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resample_time import H, W, W2, H2, line, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=11)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--baseline", action="store_true", help="(c), (d) and (g) alone, as a tree without post= is measured")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import sjpeg_amd as sj
    import sjpeg_amd.resample as rs
    n = args.frames
    gen = torch.Generator(device="cuda").manual_seed(2012)
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
          f"box {W2}x{H2}, JPEGs on the host; {args.regions} regions of {args.steps} calls", flush=True)

    def thumbs():
        return rs.encode_thumbnails(frames, (W2, H2), engine=eng)

    def area_coded():
        out, szs, offs, _, _, _ = eng.encode_ragged_flattened(sj.SRC_RGB, planes, dims, None, sizes, None, sj.YUV_420, quant, 4)
        eng.wait()
        return sj._fetch_ragged(out, szs, offs)

    def thumbs_made():
        return rs.thumbnail_images(frames, (W2, H2), engine=eng)

    if args.baseline or not hasattr(rs, "PillowFilter"):
        c, d, g = timed([thumbs, area_coded, thumbs_made], args.steps, args.regions)
        line("c", "encode_thumbnails: the _resampled_box_ call", c)
        line("d", "the area-average call (_flattened_)", d)
        line("g", "thumbnail_images: the pictures alone", g)
        return 0

    sharp, blur = rs.PillowFilter.unsharp_mask(), rs.PillowFilter.gaussian_blur(8)

    def sharp_coded():
        return rs.encode_thumbnails(frames, (W2, H2), post=sharp, engine=eng)

    def blur_coded():
        return rs.encode_thumbnails(frames, (W2, H2), post=blur, engine=eng)

    def sharp_made():
        return rs.thumbnail_images(frames, (W2, H2), post=sharp, engine=eng)

    def blur_made():
        return rs.thumbnail_images(frames, (W2, H2), post=blur, engine=eng)

    routes = [sharp_coded, blur_coded, thumbs, area_coded, sharp_made, blur_made, thumbs_made]
    try:
        from PIL import Image, ImageFilter
    except ImportError:
        Image = None
    if Image is not None:
        mask = ImageFilter.UnsharpMask(2, 150, 3)

        def detour():
            made = rs.thumbnail_images(frames, (W2, H2), engine=eng)
            torch.cuda.synchronize()
            host = [np.asarray(Image.fromarray(p.cpu().numpy()).filter(mask)) for p in made]
            return sj.encode_images([torch.from_numpy(x).cuda() for x in host], quality=75.0, yuv_mode=sj.YUV_420, method=4, engine=eng)
        routes.append(detour)
    t = timed(routes, args.steps, args.regions)
    ja, jb, jc = (fn() for fn in routes[:3])
    torch.cuda.synchronize()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pillow_filter_model as pm
    import resample_box_model as bm
    thumb = bm.thumbnail(frames[0].cpu().numpy(), (W2, H2))
    wrong = int((sharp_made()[0].cpu().numpy() != pm.unsharp_mask(thumb, 2, 150, 3)).sum()) + \
        int((blur_made()[0].cpu().numpy() != pm.gaussian_blur(thumb, 8)).sum())
    line("a", "encode_thumbnails(post=unsharp_mask())", t[0], f"; (a) - (c) = {t[0][0] - t[2][0]:.3f} ms")
    line("b", "encode_thumbnails(post=gaussian_blur(8))", t[1], f"; (b) - (c) = {t[1][0] - t[2][0]:.3f} ms")
    line("c", "encode_thumbnails: the _resampled_box_ call", t[2])
    line("d", "the area-average call (_flattened_)", t[3])
    line("e", "thumbnail_images(post=unsharp_mask()): pictures alone", t[4], f"; (e) - (g) = {t[4][0] - t[6][0]:.3f} ms")
    line("f", "thumbnail_images(post=gaussian_blur(8)): pictures alone", t[5], f"; (f) - (g) = {t[5][0] - t[6][0]:.3f} ms")
    line("g", "thumbnail_images: the pictures alone", t[6])
    same = "not run: no Pillow"
    if Image is not None:
        line("h", "the detour: thumbnails, host, PIL filter, back, encode", t[7], f"; (h) / (a) = {t[7][0] / t[0][0]:.2f}")
        same = str(routes[7]() == ja)
    print(f"  JPEG bytes a call: (a) {sum(len(j) for j in ja)}, (b) {sum(len(j) for j in jb)}, (c) {sum(len(j) for j in jc)}; "
          f"samples of (e) and (f) that differ from the definition (frame 0): {wrong}; (h)'s JPEGs equal (a)'s: {same}", flush=True)
    return 0 if wrong == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
