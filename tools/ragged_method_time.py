#!/usr/bin/env python3
"""One ragged call at the reference's default method 4 (sjpeg_hip_encode_ragged_batch_src) against the calls it
replaces, device-resident pictures, q75, 4:2:0.  (a) the 512 pictures of tools/ragged_time.py (seeded random sizes
32x32 .. 640x480): one ragged call vs a loop of encode_device_method per picture.  (b) 32 frames, 1080p and 4K mixed:
one ragged call vs two uniform encode_batch calls (one per size).  Every configuration: warm-up, synchronise, median of
several timed regions; the bytes of the ragged call must equal the per-picture calls'.  Then the host's share of (a):
the library's own timeline (SJPEG_HIP_BATCH_DEBUG, in a child process) from the symbol counts' arrival to the end of
the Huffman codes and headers (step 4), against the whole call.
    python tools/ragged_method_time.py [--regions 7] [--calls 5]"""
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

Q, MODE, METHOD = 75.0, sj.YUV_420, 4


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
    rng = np.random.RandomState(2024)
    small = []
    for k in range(512):
        w, h = int(rng.randint(32, 641)), int(rng.randint(32, 481))
        small.append(synth.g_struct(w, h, k) if k % 2 else synth.g_noise(w, h, k) // 2 + 60)
    return small, rng


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


def case(name, imgs, eng, quant, regions, calls, uniform_groups=None):
    dev, planes, dims, caps, offs, out, sizes = setup(imgs)
    stacked = [d.unsqueeze(0) for d in dev]
    srcs = [sj.make_source(sj.SRC_RGB, [s.view(1, s.shape[1], s.shape[2] * 3)])[0] for s in stacked]
    one_out = [torch.empty((1, c), dtype=torch.uint8, device="cuda") for c in caps]
    one_sz = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in caps]

    def ragged():
        eng.encode_ragged_batch(sj.SRC_RGB, planes, dims, MODE, quant, METHOD, capacities=caps, out=out, offsets=offs,
                                sizes=sizes)

    def loop():                                  # (encode_device_method's call, without its read-back)
        for k in range(len(dev)):
            eng.encode_batch(srcs[k], 1, dims[k][0], dims[k][1], MODE, quant, METHOD, out_stride=caps[k],
                             out=one_out[k], sizes=one_sz[k])

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
    print(f"{name}: {len(imgs)} pictures, {px / 1e6:.1f} Mpixel, {int(sz.sum())} bytes, byte mismatches vs per-picture "
          f"calls: {bad}")
    print(f"  ragged call        median {r[0]:9.3f} ms  (min {r[1]:.3f}, max {r[2]:.3f})")
    if uniform_groups is None:
        lp = timed(loop, regions, max(1, calls // 2))
        print(f"  per-picture loop   median {lp[0]:9.3f} ms  (min {lp[1]:.3f}, max {lp[2]:.3f})   loop / ragged = "
              f"{lp[0] / r[0]:.2f}x")
    else:
        groups = []
        for idx in uniform_groups:
            h, w = imgs[idx[0]].shape[:2]
            g = torch.stack([dev[k] for k in idx])
            src, _ = sj.make_source(sj.SRC_RGB, [g.view(len(idx), h, w * 3)])
            c = sj.frame_bound(w, h, MODE, 2048)
            o = torch.empty((len(idx), c), dtype=torch.uint8, device="cuda")
            s = torch.zeros(len(idx), dtype=torch.int64, device="cuda")
            groups.append((src, len(idx), w, h, c, o, s, g))

        def uniform():
            for src, n, w, h, c, o, s, _ in groups:
                eng.encode_batch(src, n, w, h, MODE, quant, METHOD, out_stride=c, out=o, sizes=s)
        uniform()
        torch.cuda.synchronize()
        for (src, n, w, h, c, o, s, _), idx in zip(groups, uniform_groups):
            ss = s.cpu().numpy()
            for j, k in enumerate(idx):
                if host[offs[k]:offs[k] + sz[k]].tobytes() != o[j, :int(ss[j])].cpu().numpy().tobytes():
                    bad += 1
        u = timed(uniform, regions, calls)
        print(f"  uniform batches    median {u[0]:9.3f} ms  (min {u[1]:.3f}, max {u[2]:.3f})   ragged / uniform = "
              f"{r[0] / u[0]:.3f}  ({len(groups)} calls, one per size; byte mismatches incl. these: {bad})")
    return bad


def host_share_child(calls):
    """(child process, SJPEG_HIP_BATCH_DEBUG set) (a)'s ragged call a few times; the library prints its timeline"""
    eng = sj.Engine(0)
    quant = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(Q, quant.ctypes.data)
    imgs, _ = thumbnails()
    _, planes, dims, caps, offs, out, sizes = setup(imgs)
    for _ in range(calls):
        eng.encode_ragged_batch(sj.SRC_RGB, planes, dims, MODE, quant, METHOD, capacities=caps, out=out, offsets=offs,
                                sizes=sizes)
        torch.cuda.synchronize()
        sys.stderr.write("call done\n")
    return 0


def host_share(calls):
    env = dict(os.environ, SJPEG_HIP_BATCH_DEBUG="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-share-child", "--calls", str(calls)],
                       env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        print(f"host share: child failed ({p.returncode}): {p.stderr[-500:]}")
        return
    marks, runs = {}, []
    for line in p.stderr.splitlines():
        m = re.match(r"ragged (.+?)\s+([0-9.]+) us$", line.strip())
        if m:
            marks[m.group(1)] = float(m.group(2))
        elif line.strip() == "call done" and marks:
            runs.append(marks)
            marks = {}
    runs = runs[1:] or runs                      # (the first call allocates)
    step4 = [r["tables built"] - r["counts here"] for r in runs]
    total = [r["encode launched"] for r in runs]
    print(f"(a) host share, step 4 (Huffman codes + headers of 512 pictures): median {np.median(step4) / 1e3:.3f} ms of "
          f"{np.median(total) / 1e3:.3f} ms host time to the encode launch ({len(runs)} calls; the timeline: "
          + ", ".join(f"{k} {v / 1e3:.3f}" for k, v in runs[-1].items()) + " ms)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-share-child", action="store_true")
    args = ap.parse_args()
    if args.host_share_child:
        return host_share_child(args.calls)
    eng = sj.Engine(0)
    quant = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(Q, quant.ctypes.data)
    small, rng = thumbnails()
    bad = case("(a) thumbnails 32x32 .. 640x480, method 4", small, eng, quant, args.regions, args.calls)
    big = [synth.g_struct(*((1920, 1080) if k % 2 else (3840, 2160)), 100 + k) for k in range(32)]
    order = list(rng.permutation(32))
    big = [big[i] for i in order]
    hd = [k for k in range(32) if big[k].shape[0] == 1080]
    uhd = [k for k in range(32) if big[k].shape[0] == 2160]
    bad += case("(b) 1080p and 4K mixed, method 4", big, eng, quant, args.regions, args.calls, [hd, uhd])
    eng.close()
    host_share(args.calls)
    print(f"mismatches {bad}")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
