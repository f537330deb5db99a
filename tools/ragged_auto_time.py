#!/usr/bin/env python3
"""One ragged call with the reference's SJPEG_YUV_AUTO decision (sjpeg_hip_encode_ragged_auto_src, method 4 = the
defaults of SjpegCompress) against the calls it replaces, device-resident pictures, q75.  (a) the 512 picture sizes of
tools/ragged_method_time.py (seeded 32x32 .. 640x480), content chosen so that every verdict occurs; (b) 32 frames, 1080p
and 4K mixed.  For each: the AUTO call; a per-picture loop of one-frame AUTO calls (riskiness, its read-back, the sharp
conversion where the verdict says so, the method 4 encode: what SjpegEncode(..., SJPEG_YUV_AUTO) does on the device);
the fixed-4:2:0 ragged call (sjpeg_hip_encode_ragged_batch_src); the verdict counts; byte mismatches against the loop
and against SjpegEncode(picture, 75, 4, SJPEG_YUV_AUTO) from host memory.  Then the host timeline of one AUTO call
(SJPEG_HIP_BATCH_DEBUG, in a child process).
    python tools/ragged_auto_time.py [--regions 7] [--calls 5]"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sjpeg_amd as sj  # noqa: E402
from oracle import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, METHOD = 75.0, 4
NAMES = {sj.YUV_420: "420", sj.YUV_SHARP: "sharp", sj.YUV_444: "444", sj.YUV_400: "400"}


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


def content(k, w, h):
    """Five kinds: structured, a gentle gradient, gray, black and white, the tiled test picture."""
    rng = np.random.RandomState(9000 + k)
    kind = k % 5
    if kind == 0:
        return synth.g_struct(w, h, k)
    if kind == 1:
        x = np.arange(w)[None, :] * 8 // w
        y = np.arange(h)[:, None] * 8 // h
        return np.stack([np.broadcast_to(x + 20, (h, w)), np.broadcast_to(y + 30, (h, w)), np.full((h, w), 90)],
                        2).astype(np.uint8)
    if kind == 2:
        return np.repeat(synth.g_struct(w, h, k)[:, :, 1:2], 3, 2)
    if kind == 3:
        return (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    t128 = np.fromfile(os.path.join(ROOT, "tests", "golden", "test128.rgb"), np.uint8).reshape(128, 128, 3)
    return np.ascontiguousarray(np.tile(t128, ((h + 127) // 128, (w + 127) // 128, 1))[:h, :w])


def thumbnails():
    rng = np.random.RandomState(2024)
    out = []
    for k in range(512):
        w, h = int(rng.randint(32, 641)), int(rng.randint(32, 481))
        out.append(content(k, w, h))
    return out, rng


def big_frames(rng):
    imgs = [content(k % 5, *((1920, 1080) if k % 2 else (3840, 2160))) for k in range(32)]
    return [imgs[i] for i in rng.permutation(32)]


def setup(imgs):
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    planes = [[d.view(d.shape[0], d.shape[1] * 3)] for d in dev]
    dims = [(im.shape[1], im.shape[0]) for im in imgs]
    caps = [sj.frame_bound(w, h, sj.YUV_444, 2048) for (w, h) in dims]
    offs, at = [], 0
    for c in caps:
        offs.append(at)
        at += (c + 15) & ~15
    out = torch.empty(at, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(len(imgs), dtype=torch.int64, device="cuda")
    return dev, planes, dims, caps, offs, out, sizes


def case(name, imgs, eng, quant, regions, calls):
    dev, planes, dims, caps, offs, out, sizes = setup(imgs)
    out420 = torch.empty_like(out)
    sizes420 = torch.zeros_like(sizes)
    one_out = [torch.empty(c, dtype=torch.uint8, device="cuda") for c in caps]
    one_sz = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in caps]
    modes = []

    def auto():
        modes[:] = eng.encode_ragged_auto(sj.SRC_RGB, planes, dims, sj.YUV_AUTO, quant, METHOD, capacities=caps, out=out,
                                          offsets=offs, sizes=sizes)[3]

    def fixed420():
        eng.encode_ragged_batch(sj.SRC_RGB, planes, dims, sj.YUV_420, quant, METHOD, capacities=caps, out=out420,
                                offsets=offs, sizes=sizes420)

    def loop():
        for k in range(len(dev)):
            eng.encode_ragged_auto(sj.SRC_RGB, [planes[k]], [dims[k]], sj.YUV_AUTO, quant, METHOD, capacities=[caps[k]],
                                   out=one_out[k], offsets=[0], sizes=one_sz[k])

    auto()
    loop()
    torch.cuda.synchronize()
    sz = sizes.cpu().numpy()
    host = out.cpu().numpy()
    bad_loop = bad_host = 0
    for k in range(len(dev)):
        got = host[offs[k]:offs[k] + sz[k]].tobytes() if sz[k] > 0 else b""
        n1 = int(one_sz[k].item())
        if not got or got != one_out[k][:n1].cpu().numpy().tobytes():
            bad_loop += 1
        if got != sj.SjpegEncode(imgs[k], Q, METHOD, sj.YUV_AUTO):
            bad_host += 1
    counts = {NAMES[m]: modes.count(m) for m in NAMES}
    px = sum(w * h for w, h in dims)
    r = timed(auto, regions, calls)
    f = timed(fixed420, regions, calls)
    lp = timed(loop, max(1, regions // 2), 1)
    print(f"{name}: {len(imgs)} pictures, {px / 1e6:.1f} Mpixel, {int(sz.sum())} bytes; verdicts "
          + ", ".join(f"{k} {v}" for k, v in counts.items())
          + f"; byte mismatches vs the per-picture calls {bad_loop}, vs SjpegEncode(AUTO) from host memory {bad_host}")
    print(f"  AUTO ragged call       median {r[0]:9.3f} ms  (min {r[1]:.3f}, max {r[2]:.3f})")
    print(f"  per-picture AUTO loop  median {lp[0]:9.3f} ms  (min {lp[1]:.3f}, max {lp[2]:.3f})   loop / ragged = "
          f"{lp[0] / r[0]:.2f}x")
    print(f"  fixed-4:2:0 ragged     median {f[0]:9.3f} ms  (min {f[1]:.3f}, max {f[2]:.3f})   AUTO / 4:2:0 = "
          f"{r[0] / f[0]:.2f}x")
    return bad_loop + bad_host


def timeline_child(which, calls):
    """(child process, SJPEG_HIP_BATCH_DEBUG set) one case's AUTO call a few times; the library prints its timeline"""
    eng = sj.Engine(0)
    quant = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(Q, quant.ctypes.data)
    imgs, rng = thumbnails()
    if which == "b":
        imgs = big_frames(rng)
    _, planes, dims, caps, offs, out, sizes = setup(imgs)
    for _ in range(calls):
        eng.encode_ragged_auto(sj.SRC_RGB, planes, dims, sj.YUV_AUTO, quant, METHOD, capacities=caps, out=out,
                               offsets=offs, sizes=sizes)
        torch.cuda.synchronize()
        sys.stderr.write("call done\n")
    return 0


def timeline(which, calls):
    env = dict(os.environ, SJPEG_HIP_BATCH_DEBUG="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--timeline-child", which, "--calls", str(calls)],
                       env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        print(f"({which}) timeline: child failed ({p.returncode}): {p.stderr[-500:]}")
        return
    runs, marks = [], []
    for line in p.stderr.splitlines():
        m = re.match(r"(auto|ragged) +(.+?)\s+([0-9.]+) us$", line.strip())
        if m:
            marks.append((m.group(1), m.group(2), float(m.group(3))))
        elif line.strip() == "call done" and marks:
            runs.append(marks)
            marks = []
    last = runs[-1]
    print(f"({which}) host timeline of the AUTO call (last of {len(runs)}; ms since the call's / the mode groups' "
          "start): " + ", ".join(f"{w} {n} {v / 1e3:.3f}" for w, n, v in last))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--timeline-child", default=None)
    args = ap.parse_args()
    if args.timeline_child:
        return timeline_child(args.timeline_child, args.calls)
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        sj.set_riskiness_table(f.read())
    eng = sj.Engine(0)
    quant = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(Q, quant.ctypes.data)
    small, rng = thumbnails()
    bad = case("(a) thumbnails 32x32 .. 640x480, method 4, AUTO", small, eng, quant, args.regions, args.calls)
    bad += case("(b) 1080p and 4K mixed, method 4, AUTO", big_frames(rng), eng, quant, args.regions, args.calls)
    eng.close()
    timeline("a", 3)
    timeline("b", 3)
    print(f"mismatches {bad}")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
