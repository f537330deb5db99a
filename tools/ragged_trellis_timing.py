#!/usr/bin/env python3
"""One ragged call with the trellis (sjpeg_hip_encode_ragged_trellis_src, method 7, 4:2:0, q75) against what it
replaces and against what the trellis costs, device-resident pictures.  Two batches: (a) 1 000 thumbnails of 32..256
pixels a side from a fixed seed, (b) 16 x 1080p + 4 x 4K.  For each, the median of 11 timed regions on a warm engine of
  1. the ragged trellis call;
  2. a loop of SjpegEncode(picture, 75, 7, YUV_420) FROM HOST MEMORY, one picture per call -- what there was before
     this call.  That figure includes an upload, three host waits and a download per picture, transfers the batch does
     not make; the loop's pure device share is in DESIGN.md section 6;
  3. the same batch through encode_ragged_batch method 4 (the same flow without the trellis).
The bytes of (1) must equal (2)'s.
    python tools/ragged_trellis_timing.py [--regions 11] [--calls 3] [--only a|b]
--kernels-only: the (b) batch a few times and nothing else -- run under `rocprofv3 --kernel-trace --stats -- python
tools/ragged_trellis_timing.py --kernels-only` it puts the ragged trellis statistics kind beside the uniform kind's
per-picture kernel (the SjpegEncode loop runs too)."""
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


def thumbnails():
    rng = np.random.RandomState(20261)
    imgs = []
    for k in range(1000):
        w, h = int(rng.randint(32, 257)), int(rng.randint(32, 257))
        imgs.append(synth.g_struct(w, h, k) if k % 2 else synth.g_noise(w, h, k) // 2 + 60)
    return imgs


def large():
    return [synth.g_struct(*((3840, 2160) if k % 5 == 4 else (1920, 1080)), 100 + k) for k in range(20)]


def setup(imgs):
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    planes = [[d.view(d.shape[0], d.shape[1] * 3)] for d in dev]
    dims = [(im.shape[1], im.shape[0]) for im in imgs]
    caps = [sj.frame_bound(w, h, MODE, 2048) for (w, h) in dims]
    offs, at = [], 0
    for c in caps:
        offs.append(at)
        at += (c + 15) & ~15
    out = torch.empty(at, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(len(imgs), dtype=torch.int64, device="cuda")
    return dev, planes, dims, caps, offs, out, sizes


def case(name, imgs, eng, quant, regions, calls):
    dev, planes, dims, caps, offs, out, sizes = setup(imgs)

    def trellis():
        eng.encode_ragged_trellis(sj.SRC_RGB, planes, dims, MODE, quant, 7, capacities=caps, out=out, offsets=offs,
                                  sizes=sizes)

    def method4():
        eng.encode_ragged_batch(sj.SRC_RGB, planes, dims, MODE, quant, 4, capacities=caps, out=out, offsets=offs,
                                sizes=sizes)

    host_bytes = []

    def loop():
        host_bytes[:] = [sj.SjpegEncode(im, Q, 7, MODE) for im in imgs]

    trellis()
    torch.cuda.synchronize()
    sz = sizes.cpu().numpy()
    host = out.cpu().numpy()
    loop()
    bad = sum(1 for k in range(len(imgs)) if sz[k] == 0 or host[offs[k]:offs[k] + sz[k]].tobytes() != host_bytes[k])
    px = sum(w * h for w, h in dims)
    print(f"{name}: {len(imgs)} pictures, {px / 1e6:.1f} Mpixel, {int(sz.sum())} bytes, byte mismatches vs SjpegEncode: {bad}",
          flush=True)
    t = timed(trellis, regions, calls)
    print(f"  1. ragged trellis call (method 7)      median {t[0]:9.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f})", flush=True)
    lp = timed(loop, regions, 1)
    print(f"  2. SjpegEncode(.., 7) loop, host memory median {lp[0]:9.3f} ms  (min {lp[1]:.3f}, max {lp[2]:.3f})   "
          f"loop / ragged = {lp[0] / t[0]:.2f}x  (includes the per-picture PCIe transfers and host waits)", flush=True)
    m4 = timed(method4, regions, calls)
    print(f"  3. ragged method 4 (no trellis)        median {m4[0]:9.3f} ms  (min {m4[1]:.3f}, max {m4[2]:.3f})   "
          f"trellis / method 4 = {t[0] / m4[0]:.2f}x", flush=True)
    return bad


def kernels_only(eng, quant):
    imgs = large()
    _, planes, dims, caps, offs, out, sizes = setup(imgs)
    for _ in range(4):
        eng.encode_ragged_trellis(sj.SRC_RGB, planes, dims, MODE, quant, 7, capacities=caps, out=out, offsets=offs,
                                  sizes=sizes)
        torch.cuda.synchronize()
    for _ in range(4):
        for im in imgs:
            sj.SjpegEncode(im, Q, 7, MODE)
    print(f"kernels-only: 4 ragged trellis calls and 4 SjpegEncode loops over {len(imgs)} pictures, "
          f"{sum(sj.segment_count(w, h, MODE) for (w, h) in dims)} segments a batch")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=11)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--only", choices=["a", "b"], default=None)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    eng = sj.Engine(0)
    quant = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(Q, quant.ctypes.data)
    if args.kernels_only:
        return kernels_only(eng, quant)
    bad = 0
    if args.only in (None, "a"):
        bad += case("(a) 1000 thumbnails 32..256 a side", thumbnails(), eng, quant, args.regions, args.calls)
    if args.only in (None, "b"):
        bad += case("(b) 16 x 1080p + 4 x 4K", large(), eng, quant, args.regions, args.calls)
    eng.close()
    print(f"mismatches {bad}")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
