"""What per-picture metadata costs a ragged batch: 32 pictures of 1920x1080, method 4, 4:2:0, timed four ways in ONE
process, the variants alternating round by round, medians reported:
  (a) sjpeg_hip_encode_ragged_full_src                      (the call without metadata)
  (b) sjpeg_hip_encode_ragged_full_meta_src, meta = NULL    (must stay within the run-to-run spread of (a))
  (c) ... with a 3 KB ICC profile per picture
  (d) ... with 64 KiB of EXIF and a 1 MiB ICC profile per picture (headers placed by the 16-byte copy)
and, for (d)'s header copy alone, method 0 through sjpeg_hip_encode_ragged_src with ready headers: this build (the
16-byte copy) and, with --byte-loop-lib PATH, a build of the library whose kernels still copy a byte per thread (the
commit before the wide copy) -- loaded beside this one, timed in the same rounds.

    python tools/ragged_meta_time.py [--rounds 15] [--byte-loop-lib /path/to/libsjpeg_amd.so]
Prints one JSON line; the exit status is 1 when (b) is slower than (a) by more than (a)'s own spread in this run."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sjpeg_amd as sj  # noqa: E402
from oracle import synth  # noqa: E402

N, W, H, Q = 32, 1920, 1080, 75.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--byte-loop-lib", default=None)
    args = ap.parse_args()
    eng = sj.Engine(0)
    base = synth.g_struct(W, H, 7654321)
    imgs = [torch.from_numpy(np.roll(base, 16 * k, axis=1).copy()).cuda() for k in range(N)]
    planes = [[im.view(H, 3 * W)] for im in imgs]
    dims = [(W, H)] * N
    quant = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(Q, quant.ctypes.data)
    rng = np.random.RandomState(5)
    small = [sj.PictureMetadata(iccp=rng.randint(0, 256, 3000).astype(np.uint8).tobytes()) for _ in range(N)]
    large = [sj.PictureMetadata(exif=rng.randint(0, 256, 65527).astype(np.uint8).tobytes(),
                                iccp=rng.randint(0, 256, 1 << 20).astype(np.uint8).tobytes()) for _ in range(N)]
    marr_s = sj._metadata_args("time", N, small)
    marr_l = sj._metadata_args("time", N, large)
    caps = [sj.frame_bound(W, H, sj.YUV_420, 2048 + marr_l[2][k]) for k in range(N)]     # one output layout for all
    frames, out, sizes, _ = sj._ragged_frames(planes, dims, caps, None, None, None)
    params = sj.RaggedParams(sj.YUV_420, 4, quant.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    st = sj.Engine._stream()
    L = sj.lib()

    def full():
        return L.sjpeg_hip_encode_ragged_full_src(eng._h, sj.SRC_RGB, N, frames, C.byref(params), out.data_ptr(), sizes.data_ptr(),
                                                  None, None, None, st)

    def meta(marr):
        return lambda: L.sjpeg_hip_encode_ragged_full_meta_src(eng._h, sj.SRC_RGB, N, frames, C.byref(params),
                                                               None if marr is None else C.cast(marr[0], C.c_void_p), 1,
                                                               out.data_ptr(), sizes.data_ptr(), None, None, None, st)

    # (d)'s headers ready-made, method 0: the header copy with as little else as a ragged call has
    tables, qm = sj.make_tables(quality=Q)
    headers = [sj.make_header_meta(W, H, sj.YUV_420, qm, None, b"", m.exif, m.iccp, b"") for m in large]
    hoffs = (C.c_size_t * (N + 1))()
    for i, hd in enumerate(headers):
        hoffs[i + 1] = hoffs[i] + len(hd)
    blob = b"".join(headers)
    tarr = (sj.ScanTables * 1)(tables)

    def ready(lib, h):
        return lambda: lib.sjpeg_hip_encode_ragged_src(h, sj.SRC_RGB, sj.YUV_420, N, frames, C.cast(tarr, C.c_void_p), 0, blob,
                                                       C.cast(hoffs, C.c_void_p), 1, out.data_ptr(), sizes.data_ptr(), st)

    variants = {"a_full": full, "b_meta_null": meta(None), "c_icc_3k": meta(marr_s), "d_exif64k_icc1m": meta(marr_l),
                "d_headers_ready_wide_copy": ready(L, eng._h)}
    if args.byte_loop_lib:
        old = C.CDLL(args.byte_loop_lib, mode=os.RTLD_LOCAL | os.RTLD_NOW)
        old.sjpeg_hip_engine_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        old.sjpeg_hip_encode_ragged_src.argtypes = L.sjpeg_hip_encode_ragged_src.argtypes
        h_old = C.c_void_p()
        assert old.sjpeg_hip_engine_create(0, C.byref(h_old)) == 0
        variants["d_headers_ready_byte_loop"] = ready(old, h_old)
    times = {k: [] for k in variants}
    for r in range(args.warmup + args.rounds):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (name, L.sjpeg_hip_last_error())
            assert int(sizes.min()) > 0, name
            if r >= args.warmup:
                times[name].append(dt)
    res = {"pictures": N, "size": [W, H], "method": 4, "rounds": args.rounds, "unit": "ms per call (host wall clock, synchronised)"}
    for name, ts in times.items():
        res[name] = {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}
    a, b = res["a_full"], res["b_meta_null"]
    res["b_over_a"] = round(b["median"] / a["median"], 4)
    res["a_spread"] = round((a["max"] - a["min"]) / a["median"], 4)
    # the one condition: meta = NULL costs what the call without metadata costs, within that call's own spread here
    res["b_within_spread_of_a"] = bool(b["median"] <= a["median"] * (1.0 + res["a_spread"]))
    print(json.dumps(res))
    return 0 if res["b_within_spread_of_a"] else 1


if __name__ == "__main__":
    sys.exit(main())
