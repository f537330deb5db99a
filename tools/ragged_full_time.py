#!/usr/bin/env python3
"""sjpeg_hip_encode_ragged_full_src against the per-picture loop it replaces: 32 device-resident pictures of mixed sizes
around 1 Mpixel, method 7 (= 4 + trellis), SJPEG_YUV_AUTO, each with a target size of 60 % of its q75 size, 10 passes.
(a) one batched call (pictures on the device); (b) the same pictures one at a time through the host API,
sjpeg::Encode(EncoderParam) from host memory (tools/full_search_host_loop.cc) -- the only way to these bytes before the
batched call.  The bytes of (a) must equal those of (b).  Prints both times and the batch's search_stats.
    python tools/ragged_full_time.py [--n 32] [--regions 3] [--host-loop BINARY]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sjpeg_amd as sj  # noqa: E402
from oracle import synth  # noqa: E402

METHOD, PASSES, Q = 7, 10, 75.0
SIZES = [(1280, 720), (1024, 1024), (1152, 864), (1000, 1000), (1366, 768), (960, 1080), (1200, 900), (800, 1280)]


def content(k, w, h):
    rng = np.random.RandomState(900 + k)
    kind = k % 4
    if kind == 0:
        return synth.g_struct(w, h, 100 + k)
    if kind == 1:
        return synth.g_noise(w, h, 100 + k)
    if kind == 2:
        return np.repeat(rng.randint(0, 256, (h, w, 1)), 3, 2).astype(np.uint8)
    x = np.arange(w)[None, :] * 200 // w
    y = np.arange(h)[:, None] * 200 // h
    return np.stack([np.broadcast_to(x + 20, (h, w)), np.broadcast_to(y + 30, (h, w)), np.full((h, w), 90)], 2).astype(np.uint8)


def frames(out, sizes, offs):
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    return [host[o:o + int(s)].tobytes() for o, s in zip(offs, sz)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--host-loop", default=None, help="a built tools/full_search_host_loop.cc (default: built here)")
    args = ap.parse_args()
    rng = np.random.RandomState(11)
    dims = [SIZES[i] for i in rng.randint(0, len(SIZES), args.n)]
    imgs = [content(k, w, h) for k, (w, h) in enumerate(dims)]
    planes = [[torch.from_numpy(im.reshape(im.shape[0], -1)).cuda()] for im in imgs]
    quant = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(Q, quant.ctypes.data)
    eng = sj.Engine(0)
    out, sizes, offs, modes = eng.encode_ragged_trellis(sj.SRC_RGB, planes, dims, sj.YUV_AUTO, quant, METHOD)
    q75 = [len(b) for b in frames(out, sizes, offs)]
    search = [sj.SearchParams(sj.TARGET_SIZE, float(int(0.6 * s)), PASSES, 1.0, 0.0, 100.0) for s in q75]
    batched = lambda: eng.encode_ragged_full(sj.SRC_RGB, planes, dims, sj.YUV_AUTO, quant, METHOD, search=search)  # noqa: E731
    res = batched()
    got = frames(*res[:3])
    stats = eng.search_stats()
    ts = []
    for _ in range(args.regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batched()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    with tempfile.TemporaryDirectory() as tmp:
        exe = args.host_loop
        if exe is None:
            exe = os.path.join(tmp, "full_search_host_loop")
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                                   os.path.join(ROOT, "tools", "full_search_host_loop.cc"), "-L", sj.CSRC, "-lsjpeg_amd",
                                   "-Wl,-rpath," + sj.CSRC, "-o", exe])
        with open(os.path.join(tmp, "cases"), "w") as f:
            for k, im in enumerate(imgs):
                path = os.path.join(tmp, f"{k}.rgb")
                im.tofile(path)
                f.write(f"{path} {dims[k][0]} {dims[k][1]} {Q} {METHOD} {sj.YUV_AUTO} 1 {search[k].target_value} {PASSES} 1.0\n")
        loops = []
        for _ in range(args.regions):
            text = subprocess.check_output([exe, os.path.join(tmp, "cases"), tmp], text=True)
            loops.append(float(text.split()[1]))
        host = [open(os.path.join(tmp, f"{k}.jpg"), "rb").read() for k in range(args.n)]
    px = sum(w * h for w, h in dims)
    print(f"# {args.n} pictures, {px / 1e6:.1f} Mpixels, method {METHOD}, SJPEG_YUV_AUTO, target = 0.6 x q75 size, {PASSES} passes")
    print(f"modes: {sorted((m, modes.count(m)) for m in set(modes))}")
    print(f"batched call   median {float(np.median(ts)):9.2f} ms  (min {min(ts):.2f}, max {max(ts):.2f})")
    print(f"host-API loop  median {float(np.median(loops)):9.2f} ms  (min {min(loops):.2f}, max {max(loops):.2f})")
    print(f"speed-up over the loop: {float(np.median(loops)) / float(np.median(ts)):.2f}x; bytes equal: {got == host}")
    print(f"search_stats [passes, measurement launches, waits, replayed, requantized, trellis launches]: {stats}")
    eng.close()


if __name__ == "__main__":
    main()
