#!/usr/bin/env python3
"""One ragged call (sjpeg_hip_encode_ragged_src) against the calls it replaces, device-resident pictures, method 0, q75,
4:2:0.  (a) 512 pictures of seeded random sizes 32x32 .. 640x480: one ragged call vs a loop of per-picture encode calls.
(b) 32 frames, 1080p and 4K mixed: one ragged call vs the loop and vs two uniform batches (all 1080p, all 4K).
Every configuration: warm-up, synchronise, median of several timed regions (each a few calls, synchronised at its
ends); the bytes of the ragged call must equal the per-picture calls'.
    python tools/ragged_time.py [--regions 7] [--calls 5]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sjpeg_amd as sj  # noqa: E402
from oracle import synth  # noqa: E402

Q, MODE = 75.0, sj.YUV_420


def timed(fn, regions, calls):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(regions):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / calls * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def case(name, imgs, eng, tables, quant, regions, calls, uniform_groups=None):
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    headers = [sj.make_header(im.shape[1], im.shape[0], MODE, quant) for im in imgs]
    planes = [[d.view(d.shape[0], d.shape[1] * 3)] for d in dev]
    dims = [(im.shape[1], im.shape[0]) for im in imgs]
    caps = [sj.frame_bound(w, h, MODE, len(hd)) for (w, h), hd in zip(dims, headers)]
    offs, at = [], 0
    for c in caps:
        offs.append(at)
        at += (c + 15) & ~15
    out = torch.empty(at, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(len(imgs), dtype=torch.int64, device="cuda")
    one_out = [torch.empty((1, c), dtype=torch.uint8, device="cuda") for c in caps]
    one_sz = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in caps]
    stacked = [d.unsqueeze(0) for d in dev]

    def ragged():
        eng.encode_ragged(sj.SRC_RGB, planes, dims, MODE, tables, headers, capacities=caps, out=out, offsets=offs,
                          sizes=sizes)

    def loop():
        for k in range(len(dev)):
            eng.encode_frames(stacked[k], tables, headers[k], MODE, out=one_out[k], sizes=one_sz[k],
                              out_stride=caps[k])

    # bytes: the ragged call against the per-picture calls
    ragged()
    loop()
    torch.cuda.synchronize()
    sz = sizes.cpu().numpy()
    host = out.cpu().numpy()
    bad = 0
    for k in range(len(dev)):
        n1 = int(one_sz[k].item())
        if sz[k] == 0 or host[offs[k]:offs[k] + sz[k]].tobytes() != one_out[k][0, :n1].cpu().numpy().tobytes():
            bad += 1
    px = sum(w * h for w, h in dims)
    r = timed(ragged, regions, calls)
    lp = timed(loop, regions, max(1, calls // 2))
    print(f"{name}: {len(imgs)} pictures, {px / 1e6:.1f} Mpixel, {int(sz.sum())} bytes, byte mismatches vs per-picture "
          f"calls: {bad}")
    print(f"  ragged call        median {r[0]:9.3f} ms  (min {r[1]:.3f}, max {r[2]:.3f})")
    print(f"  per-picture loop   median {lp[0]:9.3f} ms  (min {lp[1]:.3f}, max {lp[2]:.3f})   loop / ragged = "
          f"{lp[0] / r[0]:.2f}x")
    if uniform_groups:
        groups = []
        for idx in uniform_groups:
            h, w = imgs[idx[0]].shape[:2]
            g = torch.stack([dev[k] for k in idx])
            hd = headers[idx[0]]
            c = sj.frame_bound(w, h, MODE, len(hd))
            groups.append((g, hd, torch.empty((len(idx), c), dtype=torch.uint8, device="cuda"),
                           torch.zeros(len(idx), dtype=torch.int64, device="cuda"), c))

        def uniform():
            for g, hd, o, s, c in groups:
                eng.encode_frames(g, tables, hd, MODE, out=o, sizes=s, out_stride=c)
        u = timed(uniform, regions, calls)
        print(f"  uniform batches    median {u[0]:9.3f} ms  (min {u[1]:.3f}, max {u[2]:.3f})   ragged / uniform = "
              f"{r[0] / u[0]:.3f}  ({len(groups)} calls, one per size)")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    eng = sj.Engine(0)
    tables, quant = sj.make_tables(quality=Q)
    rng = np.random.RandomState(2024)
    small = []
    for k in range(512):
        w, h = int(rng.randint(32, 641)), int(rng.randint(32, 481))
        small.append(synth.g_struct(w, h, k) if k % 2 else synth.g_noise(w, h, k) // 2 + 60)
    bad = case("(a) thumbnails 32x32 .. 640x480", small, eng, tables, quant, args.regions, args.calls)
    big = [synth.g_struct(*((1920, 1080) if k % 2 else (3840, 2160)), 100 + k) for k in range(32)]
    order = list(rng.permutation(32))
    big = [big[i] for i in order]
    hd = [k for k in range(32) if big[k].shape[0] == 1080]
    uhd = [k for k in range(32) if big[k].shape[0] == 2160]
    bad += case("(b) 1080p and 4K mixed", big, eng, tables, quant, args.regions, args.calls, [hd, uhd])
    print(f"mismatches {bad}")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
