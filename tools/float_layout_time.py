#!/usr/bin/env python3
"""What the one-plane float formats and the per-channel pixel transform save: 32 frames of 3840 x 2160, q75, 4:2:0,
method 0, device-resident, each case coded by two routes on the same build:
  channels-last fp16   a [N, 3, H, W] half tensor in torch.channels_last
      (a) x.contiguous(), then the fused planar encode (SRC_RGB_PLANAR_F16) -- a full read and write of the batch first
      (b) SRC_RGB_F16 on the tensor as it lies
  [H, W, 4] fp16       a renderer's RGBA16F batch [N, H, W, 4]
      (a) x[..., :3].permute(0, 3, 1, 2).contiguous(), then SRC_RGB_PLANAR_F16
      (b) SRC_RGBA_F16 on the tensor as it lies
  un-normalise fp32    a planar [N, 3, H, W] float tensor normalised with a per-channel mean and std
      (a) x.mul(std).add(mean).mul(255).round().clamp(0, 255).to(torch.uint8), then SRC_RGB_PLANAR
      (b) SRC_RGB_PLANAR_F32 with scale[c] = 255 std[c], bias[c] = 255 mean[c]
Median of 11 timed regions of --steps steps each, as bench.py times its headline (warm engine, pipelined mode, a
synchronise at both ends of a region).  In the first two cases both routes code the same uint8 picture by contract, and
the bytes are compared; in the third route (a) rounds twice more than the fused multiply-add does, so its bytes may
differ in the last unit near ties and only its time is measured.
    python tools/float_layout_time.py [--frames 32] [--steps 10] [--regions 11] [--cases cl,rgba,norm]
A job script runs every GPU step under its own timeout, the steps chained with &&:
    timeout -k 10 600 python tools/float_layout_time.py > profiles/r12/float_layout_time.txt"""
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
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


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
    print(f"  {what:<66s} median {r[0]:8.4f} ms/step  (min {r[1]:.4f}, max {r[2]:.4f}){extra}", flush=True)


def streams(out, sizes):
    torch.cuda.synchronize()
    sz = sizes.cpu().numpy()
    return [bytes(out[k, :int(sz[k])].cpu().numpy()) for k in range(len(sz))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=11)
    ap.add_argument("--cases", default="cl,rgba,norm")
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
    print(f"device: {torch.cuda.get_device_name(0)}; {F} frames of {W}x{H}, q{Q:g}, 4:2:0, method 0; {args.regions} "
          f"regions of {args.steps} steps", flush=True)
    bad = 0

    def encode(src):
        # (Engine.encode_source allocates its output per call; the timed call writes into one pair of buffers)
        rc = sj.lib().sjpeg_hip_encode_scan_src(eng._h, C.byref(src), W, H, sj.YUV_420, F, C.byref(tables), header,
                                                len(header), 1, out.data_ptr(), stride, sizes.data_ptr(), eng._stream())
        if rc != 0:
            raise sj.SjpegError(sj.last_error())

    def planar(x, fmt):
        return sj.make_source(fmt, (x[:, 0], x[:, 1], x[:, 2]))[0]

    def run(name, label_a, label_b, route_a, route_b, compare):
        nonlocal bad
        print(f"{name}:", flush=True)
        sizes.zero_()
        a = timed(route_a, args.steps, args.regions)
        eng.wait()
        want = streams(out, sizes)
        line("(a) " + label_a, a)
        sizes.zero_()
        b = timed(route_b, args.steps, args.regions)
        eng.wait()
        wrong = sum(1 for p, q in zip(streams(out, sizes), want) if p != q)
        if compare:
            bad += wrong
        line("(b) " + label_b, b, f"   (b) / (a) = {b[0] / a[0]:.3f}; streams that differ from (a)'s: {wrong}" +
             ("" if compare else " (not held to it: (a) rounds twice more)"))

    cases = args.cases.split(",")
    if "cl" in cases:
        eng.set_pixel_transform(255.0, 0.0)
        x = (chw8.to(torch.float32) / 255.0).to(torch.float16).to(memory_format=torch.channels_last)
        assert x.stride() == (3 * H * W, 1, 3 * W, 3)
        fsrc, _ = sj.make_source(sj.SRC_RGB_F16, [x.permute(0, 2, 3, 1).reshape(F, H, W * 3)])
        run("channels-last fp16", "x.contiguous(), then SRC_RGB_PLANAR_F16", "fused, SRC_RGB_F16",
            lambda: encode(planar(x.contiguous(), sj.SRC_RGB_PLANAR_F16)), lambda: encode(fsrc), True)
        del x, fsrc
    if "rgba" in cases:
        eng.set_pixel_transform(255.0, 0.0)
        x = torch.ones((F, H, W, 4), dtype=torch.float16, device="cuda")
        x[..., :3] = (chw8.to(torch.float32) / 255.0).to(torch.float16).permute(0, 2, 3, 1)
        fsrc, _ = sj.make_source(sj.SRC_RGBA_F16, [x.reshape(F, H, W * 4)])
        run("[H, W, 4] fp16", "x[..., :3].permute(0, 3, 1, 2).contiguous(), then SRC_RGB_PLANAR_F16", "fused, SRC_RGBA_F16",
            lambda: encode(planar(x[..., :3].permute(0, 3, 1, 2).contiguous(), sj.SRC_RGB_PLANAR_F16)),
            lambda: encode(fsrc), True)
        del x, fsrc
    if "norm" in cases:
        mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
        std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
        x = (chw8.to(torch.float32) / 255.0 - mean) / std
        fp = sj.FloatPixels.normalized([], MEAN, STD)
        eng.set_pixel_transform(fp.scale3, fp.bias3)
        fsrc = planar(x, sj.SRC_RGB_PLANAR_F32)

        def unfused():
            u8 = x.mul(std).add(mean).mul(255).round().clamp(0, 255).to(torch.uint8)
            encode(planar(u8, sj.SRC_RGB_PLANAR))

        run("un-normalise fp32 (per-channel mean and std)", "mul(std).add(mean).mul(255).round().clamp().to(uint8), then SRC_RGB_PLANAR",
            "fused, SRC_RGB_PLANAR_F32 with the per-channel transform", unfused, lambda: encode(fsrc), False)
    print(f"streams of (b) that differ where both routes code the same picture by contract: {bad}")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
