#!/usr/bin/env python3
"""What a channel-first batch costs: 32 frames of 3840 x 2160, q75, 4:2:0, standard tables, device-resident, coded
  (a) from [N, H, W, 3] with encode_frames (method 0) / encode_batch (method 4),
  (b) from [N, 3, H, W] through permute(0, 2, 3, 1).contiguous() followed by (a) -- what a torch user had to do,
  (c) from [N, 3, H, W] as SRC_RGB_PLANAR with encode_source / encode_batch, no repack.
Median of 11 timed regions of --steps steps each, as bench.py times its headline (warm engine, pipelined mode, a
synchronise at both ends of a region); every output of (b) and (c) is compared with the bytes of (a).  On a build without
SRC_RGB_PLANAR (the parent commit) (a) and (b) alone are measured, for the comparison across commits.
    python tools/planar_time.py [--frames 32] [--steps 10] [--regions 11] [--methods 0,4]
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 600 python tools/planar_time.py > profiles/r10/planar_time.txt"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sjpeg_amd as sj  # noqa: E402
from oracle import synth  # noqa: E402

W, H, Q = 3840, 2160, 75.0
HAS_PLANAR = hasattr(sj, "SRC_RGB_PLANAR")


def timed(fn, steps, regions):
    for _ in range(20):
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
    print(f"  {what:<52s} median {r[0]:8.4f} ms/step  (min {r[1]:.4f}, max {r[2]:.4f}){extra}", flush=True)


def streams(out, sizes):
    torch.cuda.synchronize()
    sz = sizes.cpu().numpy()
    return [bytes(out[k, :int(sz[k])].cpu().numpy()) for k in range(len(sz))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=11)
    ap.add_argument("--methods", default="0,4")
    args = ap.parse_args()
    F = args.frames
    distinct = min(F, 8)                          # 8 distinct pictures, tiled to F frames (bench.py)
    host = [synth.g_struct(W, H, 7654321 + k) for k in range(distinct)]
    hwc = torch.empty((F, H, W, 3), dtype=torch.uint8, device="cuda")
    for k in range(F):
        hwc[k] = torch.from_numpy(host[k % distinct]).cuda()
    chw = hwc.permute(0, 3, 1, 2).contiguous()    # [N, 3, H, W]: what a dataloader or a model hands over
    tables, quant = sj.make_tables(quality=Q)
    header = sj.make_header(W, H, sj.YUV_420, quant)
    stride = (int(W * H * 0.75) + 2048 + 4095) & ~4095
    out = torch.empty((F, stride), dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(F, dtype=torch.int64, device="cuda")
    eng = sj.Engine(0)
    eng.set_pipelined(True)
    print(f"device: {torch.cuda.get_device_name(0)}; {F} frames of {W}x{H}, q{Q:g}, 4:2:0; {args.regions} regions of "
          f"{args.steps} steps; SRC_RGB_PLANAR in this build: {HAS_PLANAR}", flush=True)
    px = F * W * H
    bad = 0
    for method in [int(m) for m in args.methods.split(",")]:
        if HAS_PLANAR:
            psrc, _ = sj.make_source(sj.SRC_RGB_PLANAR, (chw[:, 0], chw[:, 1], chw[:, 2]))

        def from_hwc(frames=hwc):
            if method == 0:
                eng.encode_frames(frames, tables, header, sj.YUV_420, out=out, sizes=sizes, out_stride=stride)
            else:
                src, _ = sj.make_source(sj.SRC_RGB, [frames.view(F, H, W * 3)])
                eng.encode_batch(src, F, W, H, sj.YUV_420, quant, method=method, out_stride=stride, out=out, sizes=sizes)

        def repack_then_hwc():
            from_hwc(chw.permute(0, 2, 3, 1).contiguous())

        def from_planar():
            if method != 0:
                eng.encode_batch(psrc, F, W, H, sj.YUV_420, quant, method=method, out_stride=stride, out=out, sizes=sizes)
                return
            # (Engine.encode_source allocates its output per call; the timed call writes into the buffers of (a))
            rc = sj.lib().sjpeg_hip_encode_scan_src(eng._h, C.byref(psrc), W, H, sj.YUV_420, F, C.byref(tables), header,
                                                    len(header), 1, out.data_ptr(), stride, sizes.data_ptr(), eng._stream())
            if rc != 0:
                raise sj.SjpegError(sj.last_error())

        print(f"method {method}:", flush=True)
        a = timed(from_hwc, args.steps, args.regions)
        eng.wait()
        want = streams(out, sizes)
        line("(a) [N, H, W, 3]", a, f"   {px / a[0] / 1e6:.1f} Gpx/s")
        b = timed(repack_then_hwc, args.steps, args.regions)
        eng.wait()
        bad += sum(1 for x, y in zip(streams(out, sizes), want) if x != y)
        line("(b) [N, 3, H, W]: permute().contiguous(), then (a)", b, f"   (b) / (a) = {b[0] / a[0]:.3f}")
        if HAS_PLANAR:
            sizes.zero_()
            c = timed(from_planar, args.steps, args.regions)
            eng.wait()
            bad += sum(1 for x, y in zip(streams(out, sizes), want) if x != y)
            line("(c) [N, 3, H, W]: SRC_RGB_PLANAR", c, f"   (c) / (a) = {c[0] / a[0]:.3f}, (c) / (b) = {c[0] / b[0]:.3f}")
    print(f"byte mismatches against (a): {bad}")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
