#!/usr/bin/env python3
"""What Image.thumbnail's reduce costs and saves inside the ragged call: 100 RGB frames of 1920 x 1080, resident on the
device, to the box 320 x 180 -- 100 JPEGs in host memory, method 4, quality 75, 4:2:0:
  (a) sjpeg_amd.resample.encode_thumbnails, BICUBIC, reducing_gap 2.0: a reduce by 3 x 3 as the rows are staged, then
      640 x 360 to 320 x 180 with 9 taps an axis;
  (b) sjpeg_amd.resample.encode_resampled_images, BICUBIC, no gap: 25 taps an axis -- other bytes than (a);
  (c) Engine.encode_ragged_flattened without a flatten on the same frames: the area average;
and the pictures alone:
  (d) thumbnail_images, (e) resample_images with BICUBIC, (f) resize_images.
Median of --regions timed regions of --steps calls each (warm, a synchronise at both ends of a region), the routes
alternating region by region.  The picture (d) makes of frame 0 is compared with the definition in numpy
(tests/resample_box_model.py).
    python tools/thumbnail_time.py [--frames 100] [--steps 3] [--regions 11] [--tree DIR]
--tree DIR: import sjpeg_amd from another checkout of this repository, built there -- the parent commit's, as the
baseline of (b), (c), (e) and (f); a tree without thumbnail_images measures those alone.
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 300 python tools/thumbnail_time.py > profiles/thumbnail_time.txt"""
import argparse
import os
import sys

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

    def plain():
        return rs.encode_resampled_images(frames, sizes, filter=rs.Filter.BICUBIC, engine=eng)

    def area_coded():
        out, szs, offs, _, _, _ = eng.encode_ragged_flattened(sj.SRC_RGB, planes, dims, None, sizes, None, sj.YUV_420, quant, 4)
        eng.wait()
        return sj._fetch_ragged(out, szs, offs)

    def plain_made():
        return rs.resample_images(frames, sizes, rs.Filter.BICUBIC, engine=eng)

    def area_made():
        return sj.resize_images(frames, sizes, engine=eng)

    if not hasattr(rs, "thumbnail_images"):
        b, c, e, f = timed([plain, area_coded, plain_made, area_made], args.steps, args.regions)
        line("b", "encode_resampled_images, BICUBIC, no gap", b)
        line("c", "the area-average call", c)
        line("e", "resample_images, BICUBIC: the pictures alone", e)
        line("f", "resize_images: the pictures alone", f)
        return 0

    def thumbs():
        return rs.encode_thumbnails(frames, (W2, H2), engine=eng)

    def thumbs_made():
        return rs.thumbnail_images(frames, (W2, H2), engine=eng)

    assert rs.thumbnail_size(W, H, (W2, H2)) == (W2, H2) and rs.box_decision(rs.Filter.BICUBIC, W, H, (W2, H2), None, 2.0)["factor"] == (3, 3)
    routes = [thumbs, plain, area_coded, thumbs_made, plain_made, area_made]
    a, b, c, d, e, f = timed(routes, args.steps, args.regions)
    ja, jb, jc = (fn() for fn in routes[:3])
    torch.cuda.synchronize()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import resample_box_model as bm
    got = thumbs_made()[0].cpu().numpy()
    wrong = int((got != bm.thumbnail(frames[0].cpu().numpy(), (W2, H2))).sum())
    line("a", "encode_thumbnails, BICUBIC, reducing_gap 2.0", a)
    line("b", "encode_resampled_images, BICUBIC, no gap", b, f"; (a) / (b) = {a[0] / b[0]:.3f}")
    line("c", "the area-average call", c, f"; (a) / (c) = {a[0] / c[0]:.3f}")
    line("d", "thumbnail_images: the pictures alone", d)
    line("e", "resample_images, BICUBIC: the pictures alone", e, f"; (d) / (e) = {d[0] / e[0]:.3f}")
    line("f", "resize_images: the pictures alone", f, f"; (d) / (f) = {d[0] / f[0]:.3f}")
    print(f"  JPEG bytes a call: (a) {sum(len(j) for j in ja)}, (b) {sum(len(j) for j in jb)}, (c) {sum(len(j) for j in jc)}; "
          f"samples of (d) that differ from the definition (frame 0): {wrong}", flush=True)
    return 0 if wrong == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
