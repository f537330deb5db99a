#!/usr/bin/env python3
"""What flattening alpha inside the resize launch costs (sjpeg_hip_flatten_ragged_src): 32 device-resident RGBA 1080p
pictures fitted into 320 x 320 (320 x 180), timed these ways on the same buffers:
  (a)  sjpeg_hip_orient_ragged_src on the RGBA frames -- the same kernel without the flag, alpha dropped
  (f)  sjpeg_hip_flatten_ragged_src on them, straight alpha over white; (fp) premultiplied
  (p)  a separate flatten pass -- the flat launch at the pictures' own size, RGBA to full-size RGB -- and
  (r)  the unflattened resize of those RGB pictures: (p) + (r) is what a caller without (f) would run on this library
  (t)  the torch route per picture: (rgb * a + bg * (1 - a)).round().clamp(0, 255).to(uint8).contiguous(), then (r)
The pictures of (f) and of (p) + (r) are compared byte for byte.  Device events around regions of --steps calls each
(warm engine), (a) and (f) alternating region by region; median of --regions regions with the fastest and slowest
beside it: the spread a difference has to exceed.
    python tools/flatten_time.py [--frames 32] [--steps 10] [--regions 11]
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 300 python tools/flatten_time.py > profiles/flatten_time.txt"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sjpeg_amd as sj  # noqa: E402


def region(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def timed(fns, steps, regions):
    """the calls of fns timed in alternating regions: [(median, min, max)] in ms a call"""
    for fn in fns:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(regions):
        for k, fn in enumerate(fns):
            ts[k].append(region(fn, steps))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


def line(what, r, extra=""):
    print(f"  {what:<78s} median {r[0]:8.4f} ms/call  (min {r[1]:.4f}, max {r[2]:.4f}){extra}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=11)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    F, W, H = args.frames, args.width, args.height
    if not torch.cuda.is_available():
        print("no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    eng = sj.Engine(0)
    g = torch.Generator(device="cuda").manual_seed(W)
    pics = [torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(F)]
    planes = [[p.as_strided((H, W * 4), (p.stride(0), 1))] for p in pics]
    dims = [(W, H)] * F
    size = sj.fit_size(W, H, (320, 320))
    sizes = [size] * F
    white, pre = sj.Flatten((255, 255, 255)), sj.Flatten((255, 255, 255), True)
    print(f"device: {torch.cuda.get_device_name(0)}; {F} RGBA pictures {W}x{H} -> {size[0]}x{size[1]} a call; "
          f"{args.regions} regions of {args.steps} calls", flush=True)
    small = torch.empty(F * ((size[0] * 3 + 3) // 4 * 4 * size[1] + 16) + 64, dtype=torch.uint8, device="cuda")
    full = torch.empty(F * ((W * 3 + 3) // 4 * 4 * H + 16) + 64, dtype=torch.uint8, device="cuda")

    # the timed calls go to the C entries with ready arrays: the host's share is the entries' own
    L = sj.lib()
    frames = sj._ragged_frames(planes, dims, None, None, None, None)[0]
    sz = np.ascontiguousarray(np.asarray(sizes, np.int32))
    made, rfmt = (sj.RaggedFrame * F)(), C.c_int(0)
    fw, fpre = white._struct(), pre._struct()

    def chk(rc):
        if rc != 0:
            raise sj.SjpegError(sj.last_error())

    def plain(fmt=sj.SRC_RGBA, fr=frames):
        chk(L.sjpeg_hip_orient_ragged_src(eng._h, fmt, F, fr, sz.ctypes.data, None, small.data_ptr(), small.numel(), made, C.byref(rfmt),
                                          eng._stream()))

    def flat(f=fw):
        chk(L.sjpeg_hip_flatten_ragged_src(eng._h, sj.SRC_RGBA, F, frames, C.addressof(f), sz.ctypes.data, None, small.data_ptr(),
                                           small.numel(), made, C.byref(rfmt), eng._stream()))

    def flatten_pass():
        chk(L.sjpeg_hip_flatten_ragged_src(eng._h, sj.SRC_RGBA, F, frames, C.addressof(fw), None, None, full.data_ptr(), full.numel(), made,
                                           C.byref(rfmt), eng._stream()))

    _, rgb, _ = eng.flatten_ragged(sj.SRC_RGBA, planes, dims, white, None, None, out=full)
    rgb_frames = sj._ragged_frames([[p.as_strided((H, W * 3), (p.stride(0), 1))] for p in rgb], dims, None, None, None, None)[0]

    def resize_rgb(fr=rgb_frames):
        plain(sj.SRC_RGB, fr)

    bg = torch.full((3,), 255.0, device="cuda")

    def torch_route():
        keep = []
        for p in pics:
            al = p[..., 3:].to(torch.float32) / 255.0
            keep.append((p[..., :3].to(torch.float32) * al + bg * (1.0 - al)).round().clamp(0, 255).to(torch.uint8).contiguous())
        resize_rgb(sj._ragged_frames([[m.as_strided((H, W * 3), (m.stride(0), 1))] for m in keep], dims, None, None, None, None)[0])
        return keep

    want = [p.clone() for p in eng.flatten_ragged(sj.SRC_RGBA, planes, dims, white, sizes, None)[1]]
    got = [p.clone() for p in eng.orient_ragged(sj.SRC_RGB, [[p.as_strided((H, W * 3), (p.stride(0), 1))] for p in rgb], dims, sizes, None)[1]]
    torch.cuda.synchronize()
    wrong = sum(1 for p, q in zip(got, want) if not torch.equal(p, q))
    print(f"  pictures of (p) + (r) that differ from (f)'s: {wrong}", flush=True)

    a, f, fp = timed([plain, flat, lambda: flat(fpre)], args.steps, args.regions)
    line("(a)  oriented entry on the RGBA frames: the kernel without the flag", a, f"   spread {100 * (a[2] - a[1]) / a[0]:.1f} % of the median")
    line("(f)  flattened entry, straight alpha over white", f, f"   (f) / (a) = {f[0] / a[0]:.3f}")
    line("(fp) flattened entry, premultiplied", fp, f"   (fp) / (a) = {fp[0] / a[0]:.3f}")
    p, r = timed([flatten_pass, resize_rgb], args.steps, args.regions)
    line("(p)  a separate flatten pass at full size (the flat launch at ratio 1)", p)
    line("(r)  oriented entry on the full-size RGB pictures it makes", r, f"   ((p) + (r)) / (f) = {(p[0] + r[0]) / f[0]:.2f}")
    t, = timed([torch_route], max(1, args.steps // 5), args.regions)
    line("(t)  torch: rgb * a + bg * (1 - a), round, clamp, uint8, contiguous per picture; then (r)", t, f"   (t) / (f) = {t[0] / f[0]:.2f}")
    read = F * W * H * 4
    print(f"  source bytes a call: {read / 1e6:.1f} MB; (a) reads them at {read / a[0] / 1e6:.0f} GB/s, (f) at {read / f[0] / 1e6:.0f} GB/s", flush=True)
    return 0 if wrong == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
