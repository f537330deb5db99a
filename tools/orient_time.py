#!/usr/bin/env python3
"""What turning pictures upright inside the resize launch costs (sjpeg_hip_orient_ragged_src): 64 device-resident RGB
pictures, two cases,
  fit      1024 x 768 fitted into 256 x 256 (256 x 192 as stored): the thumbnail service's call, the source read dominates
  turn     512 x 384 at ratio 1: the pure turn, where the stores dominate
each timed these ways on the same buffers:
  (a)  sjpeg_hip_resize_ragged_src, the existing entry
  (b)  sjpeg_hip_orient_ragged_src with every orientation 1 -- the same kernel path as (a)
  (c6) ... with every orientation 6 (the portrait photo), (cm) with the orientations 1..8 mixed over the batch
  (t)  what (c6) replaces: torch.rot90(picture, -1).contiguous() for every full-size source, then (a) at the swapped sizes
The pictures of (c6) and (t) are compared byte for byte.  Median of --regions timed regions of --steps calls each (warm
engine, a synchronise at both ends of a region), with the fastest and slowest region beside it: the spread a difference
has to exceed.  --cases a times (a) alone and touches no oriented entry, so the same file runs on a build from before
them.
    python tools/orient_time.py [--frames 64] [--steps 20] [--regions 11] [--cases a,b,c,t]
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 300 python tools/orient_time.py > profiles/orient_time.txt"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sjpeg_amd as sj  # noqa: E402


def timed(fn, steps, regions):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / steps * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def line(what, r, extra=""):
    print(f"  {what:<74s} median {r[0]:8.4f} ms/call  (min {r[1]:.4f}, max {r[2]:.4f}){extra}", flush=True)


def frames_of(pics):
    planes = [[p.as_strided((p.shape[0], p.shape[1] * 3), (p.stride(0), 1))] for p in pics]
    dims = [(int(p.shape[1]), int(p.shape[0])) for p in pics]
    return sj._ragged_frames(planes, dims, None, None, None, None)[0], dims


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=11)
    ap.add_argument("--cases", default="a,b,c,t")
    args = ap.parse_args()
    F, cases = args.frames, args.cases.split(",")
    L = sj.lib()
    eng = sj.Engine(0)
    print(f"device: {torch.cuda.get_device_name(0)}; {F} RGB pictures a call; {args.regions} regions of {args.steps} calls", flush=True)
    bad = 0
    for name, (W, H), box in (("fit 1024x768 into 256x256", (1024, 768), (256, 256)), ("turn 512x384 at ratio 1", (512, 384), None)):
        g = torch.Generator(device="cuda").manual_seed(W)
        pics = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(F)]
        size = sj.fit_size(W, H, box) if box else (W, H)
        frames, dims = frames_of(pics)
        sizes = np.ascontiguousarray(np.asarray([size] * F, np.int32))
        swapped = np.ascontiguousarray(np.asarray([size[::-1]] * F, np.int32))
        need = L.sjpeg_hip_resize_ragged_bytes(sj.SRC_RGB, F, frames, sizes.ctypes.data)
        out = torch.empty(2 * need + 4096, dtype=torch.uint8, device="cuda")      # (room for the turned layout's padding too)
        made, rfmt = (sj.RaggedFrame * F)(), C.c_int(0)
        print(f"{name}: {W}x{H} -> {size[0]}x{size[1]}", flush=True)

        def chk(rc):
            if rc != 0:
                raise sj.SjpegError(sj.last_error())

        def resize(fr=frames, sz=sizes):
            chk(L.sjpeg_hip_resize_ragged_src(eng._h, sj.SRC_RGB, F, fr, sz.ctypes.data, out.data_ptr(), out.numel(), made,
                                              C.byref(rfmt), eng._stream()))

        def orient(o):
            chk(L.sjpeg_hip_orient_ragged_src(eng._h, sj.SRC_RGB, F, frames, sizes.ctypes.data, o.ctypes.data, out.data_ptr(),
                                              out.numel(), made, C.byref(rfmt), eng._stream()))

        def views():
            torch.cuda.synchronize()
            return [out.as_strided((m.height, m.width, 3), (int(m.row_stride[0]), 3, 1), int(m.plane[0]) - out.data_ptr()).clone()
                    for m in made]

        a = None
        if "a" in cases:
            a = timed(resize, args.steps, args.regions)
            line("(a)  resize entry", a, f"   spread {100 * (a[2] - a[1]) / a[0]:.1f} % of the median")
        if "b" in cases:
            ones = np.ones(F, np.uint8)
            b = timed(lambda: orient(ones), args.steps, args.regions)
            line("(b)  oriented entry, every orientation 1", b, f"   (b) / (a) = {b[0] / a[0]:.3f}" if a else "")
        want = None
        if "c" in cases:
            six = np.full(F, 6, np.uint8)
            c6 = timed(lambda: orient(six), args.steps, args.regions)
            line("(c6) oriented entry, every orientation 6", c6, f"   (c6) / (a) = {c6[0] / a[0]:.3f}" if a else "")
            want = views()
            mixed = np.asarray([1 + k % 8 for k in range(F)], np.uint8)
            cm = timed(lambda: orient(mixed), args.steps, args.regions)
            line("(cm) oriented entry, orientations 1..8 mixed", cm, f"   (cm) / (a) = {cm[0] / a[0]:.3f}" if a else "")
        if "t" in cases:
            def torch_route():
                turned = [torch.rot90(p, -1).contiguous() for p in pics]
                fr, _ = frames_of(turned)
                resize(fr, swapped)
                return turned
            t = timed(torch_route, args.steps, args.regions)
            line("(t)  rot90(source, -1).contiguous() per picture, then the resize entry", t,
                 f"   (t) / (c6) = {t[0] / c6[0]:.2f}" if want is not None else "")
            if want is not None:
                keep = torch_route()
                wrong = sum(1 for p, q in zip(views(), want) if not torch.equal(p, q))
                bad += wrong
                print(f"  pictures of (t) that differ from (c6)'s: {wrong}", flush=True)
                del keep
        del pics
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
