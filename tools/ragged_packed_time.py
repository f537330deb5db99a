#!/usr/bin/env python3
"""Ragged batches into one packed buffer (sjpeg_hip_encode_ragged_packed_src) against the unpacked call, method 4,
SJPEG_YUV_AUTO, q75, device-resident pictures.  Two batches, those of tools/ragged_trellis_timing.py: (a) 1 000
thumbnails of 32..256 pixels a side, (b) 16 x 1080p + 4 x 4K.  For each:
  (a) the device call: encode_ragged_auto into per-frame slots, encode_ragged_packed into one pool;
  (b) call plus fetch to host bytes: compress_images(packed=False) and compress_images(packed=True);
  (c) bytes allocated for the output and the engine's scratch (Engine.scratch_bytes(), a fresh engine each way).
Median of several timed regions on a warm engine, each a few calls, synchronised at its ends.  Each form is timed on an
engine of its own, the unpacked one first: the packed form's engine is the second one the process makes, which
profiles/HISTORY.md names as a possible confound of the thumbnail device-call figure.  On a build without the
packed call (the parent commit) the unpacked figures alone are measured, for the comparison across commits.
    python tools/ragged_packed_time.py [--regions 9] [--calls 3]
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 600 python tools/ragged_packed_time.py > profiles/r09/ragged_packed_time.txt"""
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

Q, METHOD = 75.0, 4
HAS_PACKED = hasattr(sj.Engine, "encode_ragged_packed")


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


def line(what, r, extra=""):
    print(f"  {what:<44s} median {r[0]:9.3f} ms  (min {r[1]:.3f}, max {r[2]:.3f}){extra}")


def case(name, imgs, quant, regions, calls):
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    planes = [[d.view(d.shape[0], d.shape[1] * 3)] for d in dev]
    dims = [(im.shape[1], im.shape[0]) for im in imgs]
    caps = [sj.frame_bound(w, h, sj.YUV_444, 2048) for (w, h) in dims]
    offs, at = [], 0
    for c in caps:
        offs.append(at)
        at += (c + 15) & ~15
    slots_bytes = at
    print(f"{name}: {len(imgs)} pictures, {sum(w * h for w, h in dims) / 1e6:.1f} Mpixel")
    bad = 0

    # unpacked: per-frame slots of frame_bound() bytes
    eng = sj.Engine(0)
    out = torch.empty(slots_bytes, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(len(imgs), dtype=torch.int64, device="cuda")

    def unpacked():
        eng.encode_ragged_auto(sj.SRC_RGB, planes, dims, sj.YUV_AUTO, quant, METHOD, capacities=caps, out=out,
                               offsets=offs, sizes=sizes)

    u = timed(unpacked, regions, calls)
    coded = int(sizes.cpu().numpy().sum())
    u_scratch = eng.scratch_bytes()
    uf = timed(lambda: sj.compress_images(dev, Q, engine=eng), regions, calls)
    want = sj.compress_images(dev, Q, engine=eng)
    eng.close()
    line("(a) device call, unpacked", u)
    line("(b) compress_images(packed=False)", uf, f"   fetch = {uf[0] - u[0]:.3f} ms over the device call")
    print(f"  (c) unpacked: output {slots_bytes} bytes allocated for {coded} coded, engine scratch {u_scratch} bytes")
    if not HAS_PACKED:
        print("  (this build has no packed call)")
        return 0

    eng = sj.Engine(0)
    pool_bytes = sj._first_pool(dims, sj.YUV_AUTO)
    pool = torch.empty(pool_bytes, dtype=torch.uint8, device="cuda")

    def packed():
        return eng.encode_ragged_packed(sj.SRC_RGB, planes, dims, sj.YUV_AUTO, quant, METHOD, capacities=caps, out=pool)

    p = timed(packed, regions, calls)
    res = packed()
    torch.cuda.synchronize()
    end = int(res[2][-1].item())
    p_scratch = eng.scratch_bytes()
    before = sj.packed_stats()
    pf = timed(lambda: sj.compress_images(dev, Q, engine=eng, packed=True), regions, calls)
    got = sj.compress_images(dev, Q, engine=eng, packed=True)
    retries = sj.packed_stats()["retries"] - before["retries"]
    eng.close()
    bad += sum(1 for a, b in zip(got, want) if a != b) + (end < 0)
    line("(a) device call, packed", p, f"   packed / unpacked = {p[0] / u[0]:.3f}")
    line("(b) compress_images(packed=True)", pf, f"   packed / unpacked = {pf[0] / uf[0]:.3f}, second calls {retries}")
    print(f"  (c) packed:   output {pool_bytes} bytes allocated (first pool) for {end & ((1 << 63) - 1)} used, "
          f"engine scratch {p_scratch} bytes")
    print(f"  byte mismatches packed vs unpacked: {bad}")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--calls", type=int, default=3)
    args = ap.parse_args()
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        sj.set_riskiness_table(f.read())
    mhz = C.c_float(0)
    torch.zeros(1, device="cuda")
    if sj.lib().sjpeg_hip_debug_shader_clock(C.byref(mhz), C.c_void_p(torch.cuda.current_stream().cuda_stream)) != 0:
        mhz.value = 0
    print(f"device: {torch.cuda.get_device_name(0)}, shader clock measured by a probe wave {mhz.value:.0f} MHz, "
          f"packed call in this build: {HAS_PACKED}; regions {args.regions} x {args.calls} calls")
    quant = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(Q, quant.ctypes.data)
    bad = case("(1) 1000 thumbnails 32..256 a side", thumbnails(), quant, args.regions, args.calls)
    bad += case("(2) 16 x 1080p + 4 x 4K", large(), quant, args.regions, args.calls)
    print(f"mismatches {bad}")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
