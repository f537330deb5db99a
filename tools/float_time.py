#!/usr/bin/env python3
"""What a float channel-first batch costs: 32 frames of 3840 x 2160, q75, 4:2:0, device-resident [N, 3, H, W] tensors
of float32, float16 and bfloat16 with values in 0..1, coded with method 0 and method 4 by two routes on the same build:
  (a) x.mul(255).round().clamp(0, 255).to(torch.uint8), then the planar encode (SRC_RGB_PLANAR) -- what a torch user
      had to do: the conversion passes, a second copy of the batch, a handful of launches;
  (b) the fused call: SRC_RGB_PLANAR_F32 / _F16 / _BF16 with the engine's pixel transform (255, 0), no uint8 copy.
Median of 11 timed regions of --steps steps each, as bench.py times its headline (warm engine, pipelined mode, a
synchronise at both ends of a region).  The bytes of (b) are compared with the planar encode of the uint8 batch the
contract defines -- (x.float() * 255) rounded to even and clamped: with a bias of 0 the product has the one rounding of
the fused multiply-add.  (Route (a) multiplies in the tensor's own dtype, so for float16 and bfloat16 its bytes may
differ from the contract's in the last unit; its time is what is measured, not its bytes.)
    python tools/float_time.py [--frames 32] [--steps 10] [--regions 11] [--methods 0,4] [--dtypes f32,f16,bf16]
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 600 python tools/float_time.py > profiles/r11/float_time.txt"""
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
DTYPES = {"f32": (torch.float32, sj.SRC_RGB_PLANAR_F32), "f16": (torch.float16, sj.SRC_RGB_PLANAR_F16),
          "bf16": (torch.bfloat16, sj.SRC_RGB_PLANAR_BF16)}


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
    print(f"  {what:<58s} median {r[0]:8.4f} ms/step  (min {r[1]:.4f}, max {r[2]:.4f}){extra}", flush=True)


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
    ap.add_argument("--dtypes", default="f32,f16,bf16")
    args = ap.parse_args()
    F = args.frames
    distinct = min(F, 8)                          # 8 distinct pictures, tiled to F frames (bench.py)
    host = [synth.g_struct(W, H, 7654321 + k) for k in range(distinct)]
    chw8 = torch.empty((F, 3, H, W), dtype=torch.uint8, device="cuda")
    for k in range(F):
        chw8[k] = torch.from_numpy(np.ascontiguousarray(host[k % distinct].transpose(2, 0, 1))).cuda()
    tables, quant = sj.make_tables(quality=Q)
    header = sj.make_header(W, H, sj.YUV_420, quant)
    stride = (int(W * H * 0.75) + 2048 + 4095) & ~4095
    out = torch.empty((F, stride), dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(F, dtype=torch.int64, device="cuda")
    eng = sj.Engine(0)
    eng.set_pipelined(True)
    eng.set_pixel_transform(255.0, 0.0)
    print(f"device: {torch.cuda.get_device_name(0)}; {F} frames of {W}x{H}, q{Q:g}, 4:2:0; {args.regions} regions of "
          f"{args.steps} steps", flush=True)
    bad = 0

    def encode(src, method):
        if method != 0:
            eng.encode_batch(src, F, W, H, sj.YUV_420, quant, method=method, out_stride=stride, out=out, sizes=sizes)
            return
        # (Engine.encode_source allocates its output per call; the timed call writes into one pair of buffers)
        rc = sj.lib().sjpeg_hip_encode_scan_src(eng._h, C.byref(src), W, H, sj.YUV_420, F, C.byref(tables), header,
                                                len(header), 1, out.data_ptr(), stride, sizes.data_ptr(), eng._stream())
        if rc != 0:
            raise sj.SjpegError(sj.last_error())

    for name in args.dtypes.split(","):
        dtype, fmt = DTYPES[name]
        x = (chw8.to(torch.float32) / 255.0).to(dtype)        # what a network puts out: values in 0..1
        contract = (x.float() * 255.0).round().clamp(0, 255).to(torch.uint8)
        csrc, _ = sj.make_source(sj.SRC_RGB_PLANAR, (contract[:, 0], contract[:, 1], contract[:, 2]))
        fsrc, _ = sj.make_source(fmt, (x[:, 0], x[:, 1], x[:, 2]))
        for method in [int(m) for m in args.methods.split(",")]:
            sizes.zero_()
            encode(csrc, method)
            eng.wait()
            want = streams(out, sizes)

            def unfused():
                u8 = x.mul(255).round().clamp(0, 255).to(torch.uint8)
                src, _ = sj.make_source(sj.SRC_RGB_PLANAR, (u8[:, 0], u8[:, 1], u8[:, 2]))
                encode(src, method)

            def fused():
                encode(fsrc, method)

            print(f"{name}, method {method}:", flush=True)
            a = timed(unfused, args.steps, args.regions)
            eng.wait()
            line("(a) mul/round/clamp/to(uint8), then SRC_RGB_PLANAR", a)
            sizes.zero_()
            b = timed(fused, args.steps, args.regions)
            eng.wait()
            wrong = sum(1 for p, q in zip(streams(out, sizes), want) if p != q)
            bad += wrong
            line(f"(b) fused, SRC_RGB_PLANAR_{name.upper()}", b, f"   (b) / (a) = {b[0] / a[0]:.3f}; byte mismatches: {wrong}")
        del x, contract
    print(f"byte mismatches of (b) against the contract's uint8 batch: {bad}")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
