#!/usr/bin/env python3
"""What a storyboard sheet costs on the device: 100 NV12 frames of 1920 x 1080, resident in device memory, to ONE JPEG
of a 10 x 10 sheet of 160 x 90 cells (1600 x 900), method 4, quality 75, two routes on one build:
  (a) encode_yuv_sheets: ONE call -- the background fill, the resize kernel over the tiles of every plane storing each
      thumbnail straight into its cell, one inner encode of the sheet;
  (b) the same sheet composed from the calls of before: Engine.resize_ragged_yuv, a slice copy per plane per frame into
      a sheet tensor, then encode_ragged_full of the sheet's planes as SRC_YUV420.
The two make the same bytes, which is checked.  Then (c): Engine.resize_ragged_yuv alone on the same frames -- the
UNPLACED path, to be timed on this build and on a build of the parent commit (the same loop run from a checkout of the
parent, whose binding does not know the sheet entries): it shows whether that path kept its code.  Median of --regions timed regions of --steps calls each (warm, a synchronise at both ends of a region),
the routes alternating region by region.
    python tools/sheet_time.py [--frames 100] [--steps 5] [--regions 11] [--only-resize]
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 300 python tools/sheet_time.py > profiles/sheet_time.txt"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sjpeg_amd as sj  # noqa: E402

W, H, CW, CH, COLS, ROWS = 1920, 1080, 160, 90, 10, 10
BG = (16, 128, 128)


def region(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def timed(fns, steps, regions):
    for fn in fns:
        for _ in range(3):
            fn()
    ts = [[] for _ in fns]
    for _ in range(regions):
        for k, fn in enumerate(fns):
            ts[k].append(region(fn, steps))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--regions", type=int, default=11)
    ap.add_argument("--only-resize", action="store_true", help="time (c) alone")
    args = ap.parse_args()
    n = args.frames
    rs = np.random.RandomState(1080)
    ramp = (np.add.outer(np.arange(H), np.arange(W)) // 12 % 256).astype(np.int64)
    frames = []
    for k in range(n):
        y = np.clip(ramp + rs.randint(-12, 13, (H, W)) + 2 * k, 0, 255).astype(np.uint8)
        uv = rs.randint(96, 160, (H // 2, W)).astype(np.uint8)
        frames.append((torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()))
    eng = sj.Engine(0)
    dims, sizes = [(W, H)] * n, [(CW, CH)] * n
    planes = [list(f) for f in frames]
    quant = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(75.0, quant.ctypes.data)
    print(f"device: {torch.cuda.get_device_name(0)}; library {os.path.basename(sj.LIB_PATH)}; {n} NV12 frames {W}x{H} on the device; {args.regions} regions "
          f"of {args.steps} calls", flush=True)

    def resize_alone():
        return eng.resize_ragged_yuv(sj.SRC_NV12, planes, dims, sizes)

    if args.only_resize:
        (c,) = timed([resize_alone], args.steps, args.regions)
        print(f"  (c) resize_ragged_yuv alone (unplaced path)          median {c[0]:9.3f} ms/call  (min {c[1]:.3f}, max {c[2]:.3f})", flush=True)
        return 0
    sheet = sj.Sheet(COLS, ROWS, (CW, CH), 0, 0, BG)
    SW, SH = sj.sheet_size(sheet, sj.SRC_NV12)
    per = COLS * ROWS
    nsheets = (n + per - 1) // per

    def ours():
        return sj.encode_yuv_sheets(frames, sj.SRC_NV12, sheet, sizes=sizes, engine=eng)[0]

    def composed():
        _, pics, _ = eng.resize_ragged_yuv(sj.SRC_NV12, planes, dims, sizes)
        made = []
        for s in range(nsheets):
            ys = torch.full((SH, SW), BG[0], dtype=torch.uint8, device="cuda")
            us = torch.full((SH // 2, SW // 2), BG[1], dtype=torch.uint8, device="cuda")
            vs = torch.full((SH // 2, SW // 2), BG[2], dtype=torch.uint8, device="cuda")
            for k in range(s * per, min(n, (s + 1) * per)):
                j, i = divmod(k - s * per, COLS)
                y, u, v = pics[k]
                ys[j * CH:(j + 1) * CH, i * CW:(i + 1) * CW] = y
                us[j * CH // 2:(j + 1) * CH // 2, i * CW // 2:(i + 1) * CW // 2] = u
                vs[j * CH // 2:(j + 1) * CH // 2, i * CW // 2:(i + 1) * CW // 2] = v
            made.append([ys, us, vs])
        out, sz, offs, _, _, _ = eng.encode_ragged_full(sj.SRC_YUV420, made, [(SW, SH)] * nsheets, sj.YUV_420, quant, 4)
        eng.wait()
        return sj._fetch_ragged(out, sz, offs)

    a, b, c = timed([ours, composed, resize_alone], args.steps, args.regions)
    same = ours() == composed()
    print(f"  (a) encode_yuv_sheets                                median {a[0]:9.3f} ms/call  (min {a[1]:.3f}, max {a[2]:.3f})", flush=True)
    print(f"  (b) resize_ragged_yuv + slice copies + encode_ragged_full median {b[0]:9.3f} ms/call  (min {b[1]:.3f}, max {b[2]:.3f}); "
          f"(b) / (a) = {b[0] / a[0]:.2f}", flush=True)
    print(f"  (c) resize_ragged_yuv alone (unplaced path)          median {c[0]:9.3f} ms/call  (min {c[1]:.3f}, max {c[2]:.3f})", flush=True)
    print(f"  the two sheets' JPEGs are {'the same bytes' if same else 'DIFFERENT'}: {sum(len(j) for j in ours())} bytes", flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
