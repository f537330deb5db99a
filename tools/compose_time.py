#!/usr/bin/env python3
"""What the compose stage costs inside the ragged call, and the detour it replaces: 100 RGB frames of 1920 x 1080,
resident on the device, to the box 320 x 180, padded to 320 x 320 with a 64 x 64 logo 8 from the bottom-right corner --
100 JPEGs in host memory, method 4, quality 75, 4:2:0:
  (a) sjpeg_amd.resample.encode_thumbnails(compose=Compose.pad((320, 320), overlays=[logo])): the composed call;
  (b) encode_thumbnails without compose: the _resampled_box_ call, JPEGs of 320 x 180;
  (c) encode_thumbnails(post=PillowFilter.unsharp_mask()): the _filtered_ call;
  (d) Engine.encode_ragged_flattened without a flatten on the same frames: the area average (the _flattened_ call);
and the pictures alone:
  (e) thumbnail_images(compose=...), (f) thumbnail_images;
and the detour in torch:
  (g) thumbnail_images, then per picture a new canvas tensor, a slice assignment and a float blend of the logo with
      round().clamp().to(uint8), then encode_images -- whose JPEGs must equal (a)'s.
Median of --regions timed regions of --steps calls each (warm, a synchronise at both ends of a region), the routes
alternating region by region.  The picture (e) makes of frame 0 is compared with the definition in numpy
(tests/compose_model.py).
    python tools/compose_time.py [--frames 100] [--steps 3] [--regions 11] [--tree DIR] [--baseline]
--tree DIR: import sjpeg_amd from another checkout of this repository, built there -- the parent commit's, as the
baseline of (b), (c), (d) and (f); a tree without compose= measures those alone, and --baseline measures this tree the
same way: a process with the same routes in it, which is what the two builds are compared by.
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 300 python tools/compose_time.py > profiles/compose_time.txt"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resample_time import H, W, W2, H2, line, timed  # noqa: E402

CANVAS, LOGO, MARGIN, COLOUR = (320, 320), 64, 8, (24, 24, 24)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=11)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--baseline", action="store_true", help="(b), (c), (d) and (f) alone, as a tree without compose= is measured")
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
          f"box {W2}x{H2} on {CANVAS[0]}x{CANVAS[1]}, JPEGs on the host; {args.regions} regions of {args.steps} calls", flush=True)
    sharp = rs.PillowFilter.unsharp_mask()

    def thumbs():
        return rs.encode_thumbnails(frames, (W2, H2), engine=eng)

    def sharp_coded():
        return rs.encode_thumbnails(frames, (W2, H2), post=sharp, engine=eng)

    def area_coded():
        out, szs, offs, _, _, _ = eng.encode_ragged_flattened(sj.SRC_RGB, planes, dims, None, sizes, None, sj.YUV_420, quant, 4)
        eng.wait()
        return sj._fetch_ragged(out, szs, offs)

    def thumbs_made():
        return rs.thumbnail_images(frames, (W2, H2), engine=eng)

    if args.baseline or not hasattr(rs, "Compose"):
        b, c, d, f = timed([thumbs, sharp_coded, area_coded, thumbs_made], args.steps, args.regions)
        line("b", "encode_thumbnails: the _resampled_box_ call", b)
        line("c", "encode_thumbnails(post=unsharp_mask()): _filtered_", c)
        line("d", "the area-average call (_flattened_)", d)
        line("f", "thumbnail_images: the pictures alone", f)
        return 0

    # the logo: a disc with a soft edge over a gradient, alpha from 0 to 255
    yy, xx = torch.meshgrid(torch.arange(LOGO, device="cuda"), torch.arange(LOGO, device="cuda"), indexing="ij")
    dist = ((yy - 31.5) ** 2 + (xx - 31.5) ** 2).sqrt()
    alpha = ((30.0 - dist) * 40.0).clamp(0, 255)
    logo_t = torch.stack([(4 * xx) % 256, (4 * yy) % 256, 255 - (2 * xx + 2 * yy) % 256, alpha], dim=2).to(torch.uint8).contiguous()
    logo = rs.Overlay(logo_t)
    comp = rs.Compose.pad(CANVAS, COLOUR, overlays=[(logo, (MARGIN, MARGIN), "bottom-right")])

    def composed():
        return rs.encode_thumbnails(frames, (W2, H2), compose=comp, engine=eng)

    def composed_made():
        return rs.thumbnail_images(frames, (W2, H2), compose=comp, engine=eng)

    src, a255 = logo_t[..., :3].float(), logo_t[..., 3:].float()
    fill = torch.tensor(COLOUR, dtype=torch.uint8, device="cuda")

    def detour():
        made = rs.thumbnail_images(frames, (W2, H2), engine=eng)
        out = []
        for p in made:
            canvas = fill.expand(CANVAS[1], CANVAS[0], 3).contiguous()
            h, w = p.shape[0], p.shape[1]
            x, y = round((CANVAS[0] - w) * 0.5), round((CANVAS[1] - h) * 0.5)
            canvas[y:y + h, x:x + w] = p
            ox, oy = CANVAS[0] - LOGO - MARGIN, CANVAS[1] - LOGO - MARGIN
            under = canvas[oy:oy + LOGO, ox:ox + LOGO].float()
            # (the exact quotient: the numerator is an integer below 2^24, so float32 holds it, and the floor of the
            # sum with 127 is the definition's)
            canvas[oy:oy + LOGO, ox:ox + LOGO] = ((under * (255.0 - a255) + src * a255 + 127.0) / 255.0).floor().round().clamp(0, 255).to(torch.uint8)
            out.append(canvas)
        return sj.encode_images(out, quality=75.0, yuv_mode=sj.YUV_420, method=4, engine=eng)

    routes = [composed, thumbs, sharp_coded, area_coded, composed_made, thumbs_made, detour]
    t = timed(routes, args.steps, args.regions)
    ja, jb = composed(), thumbs()
    torch.cuda.synchronize()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import compose_model as cm
    import resample_box_model as bm
    thumb = bm.thumbnail(frames[0].cpu().numpy(), (W2, H2))
    want = cm.compose(thumb, CANVAS, colour=COLOUR, overlays=[(logo_t.cpu().numpy(), (MARGIN, MARGIN), "bottom-right")])
    wrong = int((composed_made()[0].cpu().numpy() != want).sum())
    line("a", "encode_thumbnails(compose=pad + logo): _composed_", t[0], f"; (a) - (b) = {t[0][0] - t[1][0]:.3f} ms")
    line("b", "encode_thumbnails: the _resampled_box_ call", t[1])
    line("c", "encode_thumbnails(post=unsharp_mask()): _filtered_", t[2])
    line("d", "the area-average call (_flattened_)", t[3])
    line("e", "thumbnail_images(compose=...): pictures alone", t[4], f"; (e) - (f) = {t[4][0] - t[5][0]:.3f} ms")
    line("f", "thumbnail_images: the pictures alone", t[5])
    line("g", "the detour: thumbnails, torch canvas and blend, encode", t[6], f"; (g) / (a) = {t[6][0] / t[0][0]:.2f}")
    same = detour() == ja
    print(f"  JPEG bytes a call: (a) {sum(len(j) for j in ja)}, (b) {sum(len(j) for j in jb)}; samples of (e) that differ from the "
          f"definition (frame 0): {wrong}; (g)'s JPEGs equal (a)'s: {same}", flush=True)
    return 0 if wrong == 0 and same else 1


if __name__ == "__main__":
    sys.exit(main())
