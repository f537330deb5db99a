"""Resampling with Pillow's filters (sjpeg_hip_resample_ragged_src and the _resampled_ entries, sjpeg_amd.resample) without
a GPU: every refusal before any device work with its message, the size function, the module's own refusals, the
constants the kernel and the plan share, and the exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sjpeg_amd as sj
import sjpeg_amd.resample as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = C.c_void_p(1 << 20)          # (the checks come before the engine is touched: any non-NULL value stands in for one)
SHAPE = "sjpeg_hip_resample_ragged_src"
ENCODE = "sjpeg_hip_encode_ragged_resampled_src"
PACKED = "sjpeg_hip_encode_ragged_resampled_packed_src"
ENTRIES = (SHAPE, ENCODE, PACKED)
YUV_FORMATS = [(sj.SRC_YUV444, "SJPEG_HIP_SRC_YUV444", 3), (sj.SRC_YUV420, "SJPEG_HIP_SRC_YUV420", 3),
               (sj.SRC_NV12, "SJPEG_HIP_SRC_NV12", 2), (sj.SRC_NV21, "SJPEG_HIP_SRC_NV21", 2)]
WHITE = ((255, 255, 255), 0, 255.0, 0.0)
LANCZOS = ((4, 0, 0, 0),)
L = rs._lib()


def _err():
    return L.sjpeg_hip_last_error().decode()


def _refused(rc, who, *words):
    assert rc == EINVAL
    msg = _err()
    assert msg.startswith(who + ": "), msg
    for w in words:
        assert w in msg, (w, msg)


def _frames(dims, planes=1, stride=1 << 19):
    f = (sj.RaggedFrame * len(dims))()
    for k, (w, h) in enumerate(dims):
        f[k].width, f[k].height = w, h
        for i in range(planes):
            f[k].plane[i] = (1 << 30) + (i << 24)
            f[k].row_stride[i] = stride
        f[k].out_offset = (1 << 20) * k
        f[k].out_capacity = 1 << 20
    return f


def _ptr(values, dtype, shape):
    if values is None:
        return None, None
    arr = np.ascontiguousarray(np.asarray(values, dtype).reshape(shape))
    return arr, arr.ctypes.data


def _call(who, frames, fmt=sj.SRC_RGB, resample=LANCZOS, per_frame=0, unsharp=None, sizes=None, orientations=None, flatten=None, mode=None,
          engine=FAKE, out_bytes=1 << 30, d_out=1 << 28, nframes=None, params=True, made=True):
    """one of the three entries on a stand-in engine.  resample: rows (filter, reserved 0, 1, 2) or None; unsharp: rows
    (amount, threshold, reserved 0, 1) or None; flatten: (background, premultiplied, alpha_scale, alpha_bias)"""
    if mode is None:
        mode = sj.YUV_400 if fmt == sj.SRC_GRAY else sj.YUV_420
    n = len(frames) if nframes is None else nframes
    k1, sp = _ptr(sizes, np.int32, (-1, 2))
    k2, op = _ptr(orientations, np.uint8, (-1,))
    k3, rp = _ptr(resample, np.uint8, (-1, 4))
    k4, up = _ptr(unsharp, np.uint8, (-1, 4))
    fst = None if flatten is None else sj._FlattenStruct((C.c_uint8 * 3)(*flatten[0]), flatten[1], flatten[2], flatten[3])
    fp = None if fst is None else C.addressof(fst)
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, 4, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    pp = C.byref(p) if params else None
    out = (sj.RaggedFrame * 8)() if made else None
    rfmt = C.c_int(-7)
    if who == SHAPE:
        rc = L.sjpeg_hip_resample_ragged_src(engine, fmt, n, frames, fp, sp, op, rp, per_frame, up, 0, d_out, out_bytes, out, C.byref(rfmt), None)
    elif who == ENCODE:
        rc = L.sjpeg_hip_encode_ragged_resampled_src(engine, fmt, n, frames, pp, fp, sp, op, rp, per_frame, up, 0, None, 0, 1 << 16, 1 << 12,
                                                     None, None, None, None)
    else:
        assert who == PACKED
        rc = L.sjpeg_hip_encode_ragged_resampled_packed_src(engine, fmt, n, frames, pp, fp, sp, op, rp, per_frame, up, 0, None, 0, 1 << 16,
                                                            1 << 20, 1 << 12, 1 << 13, None, None, None, None)
    assert rfmt.value == -7             # refused: nothing was reported
    return rc


# ---- the entries' refusals, each before the engine is touched; the messages are pinned here

@pytest.mark.parametrize("who", ENTRIES)
def test_null_resample_a_bad_filter_and_a_reserved_byte(who):
    fr = _frames([(32, 16), (20, 10), (8, 8)])
    _refused(_call(who, fr, resample=None), who, "resample == NULL")
    assert _err() == who + ": resample == NULL"
    _refused(_call(who, fr, resample=[(4, 0, 0, 0), (0, 0, 0, 0), (5, 0, 0, 0)], per_frame=1), who,
             "frame 2: resample: filter 5 is not one of SJPEG_HIP_RESAMPLE_BOX (0) .. SJPEG_HIP_RESAMPLE_LANCZOS (4)")
    _refused(_call(who, fr, resample=[(255, 0, 0, 0)]), who, "resample: filter 255 is not one of")
    assert "frame" not in _err()
    _refused(_call(who, fr, resample=[(4, 0, 0, 0), (3, 0, 9, 0), (0, 0, 0, 0)], per_frame=1), who, "frame 1: resample: reserved must be 0")
    assert _err() == who + ": frame 1: resample: reserved must be 0"
    for k in range(3):
        row = [4, 0, 0, 0]
        row[1 + k] = 1
        _refused(_call(who, fr, resample=[tuple(row)]), who, "resample: reserved must be 0")
    # (resample_per_frame == 0: resample[0] alone is read)
    _refused(_call(who, fr, resample=[(4, 0, 0, 0), (9, 0, 0, 0)], orientations=[1, 9, 1]), who, "frame 1: orientation 9")


@pytest.mark.parametrize("who", ENTRIES)
@pytest.mark.parametrize("fmt,name,planes", YUV_FORMATS)
def test_yuv_plane_formats_are_refused_by_name(who, fmt, name, planes):
    mode = sj.YUV_444 if fmt == sj.SRC_YUV444 else sj.YUV_420
    _refused(_call(who, _frames([(32, 16)], planes), fmt, mode=mode, sizes=[(8, 4)]), who, name + " pictures are not resampled",
             "an RGB-like or a gray format")


@pytest.mark.parametrize("who", ENTRIES)
def test_sizes_and_the_cap(who):
    fr = _frames([(400, 200), (20, 10)])
    _refused(_call(who, fr, sizes=[(0, 4), (20, 10)]), who, "frame 0: size 0x4 is below 1x1")
    _refused(_call(who, fr, sizes=[(8, 4), (20, -1)]), who, "frame 1: size 20x-1 is below 1x1")
    _refused(_call(who, fr, sizes=[(8, 4), (65536, 10)]), who, "frame 1: size 65536x10 is above 65535x65535")
    _refused(_call(who, fr, sizes=[(400, 65536), (20, 10)]), who, "frame 0: size 400x65536 is above 65535x65535")
    # Lanczos 400 -> 6 takes 2 * ceil(3 * 400 / 6) + 1 = 401 samples; bicubic takes 269, and the y axis is named as the x
    assert rs.resample_ksize(rs.Filter.LANCZOS, 400, 6) == 401 and rs.resample_ksize(rs.Filter.LANCZOS, 400, 7) == 345
    _refused(_call(who, fr, sizes=[(6, 200), (20, 10)]), who,
             "frame 0: the x axis, 400 to 6 samples with SJPEG_HIP_RESAMPLE_LANCZOS, takes a window of 401 samples, above the cap of 385")
    _refused(_call(who, fr, sizes=[(400, 3), (20, 10)]), who, "frame 0: the y axis, 200 to 3 samples with SJPEG_HIP_RESAMPLE_LANCZOS",
             "above the cap of 385")
    _refused(_call(who, fr, resample=[(3, 0, 0, 0), (0, 0, 0, 0)], per_frame=1, sizes=[(400, 200), (20, 1)], orientations=[1, 1],
                   flatten=WHITE), who, "flatten: SJPEG_HIP_SRC_RGB has no alpha channel")
    _refused(_call(who, _frames([(20, 1000)]), resample=[(0, 0, 0, 0)], sizes=[(20, 2)]), who, "frame 0: the y axis, 1000 to 2 samples with "
             "SJPEG_HIP_RESAMPLE_BOX, takes a window of 501 samples")


@pytest.mark.parametrize("who", ENTRIES)
def test_null_arguments_and_the_short_buffer(who):
    fr = _frames([(32, 16)])
    _refused(_call(who, fr, engine=None), who, "engine == NULL")
    _refused(_call(who, None, nframes=1), who, "frames", "== NULL")
    if who == SHAPE:
        _refused(_call(who, fr, d_out=None), who, "d_out", "== NULL")
        _refused(_call(who, fr, made=False), who, "== NULL")
        _refused(_call(who, fr, d_out=(1 << 28) + 4), who, "d_out must be a multiple of 16")
        # enlarged to 64 x 32: 64 * 3 * 32 bytes
        _refused(_call(who, fr, sizes=[(64, 32)], out_bytes=6143), who, "bytes 6143 is below the 6144 bytes the resampled pictures take",
                 "sjpeg_hip_resample_ragged_bytes")
    else:
        _refused(_call(who, fr, params=False), who, "params == NULL")
    _refused(_call(who, fr, nframes=0), who, "nframes must be 1..65535")
    _refused(_call(who, fr, 99), who, "unknown source format")


@pytest.mark.parametrize("who", ENTRIES)
def test_the_older_entries_checks_are_reached(who):
    fr = _frames([(32, 16), (20, 10)])
    _refused(_call(who, fr, orientations=[1, 9]), who, "frame 1: orientation 9 is not one of 1..8")
    _refused(_call(who, fr, flatten=WHITE), who, "flatten: SJPEG_HIP_SRC_RGB has no alpha channel")
    _refused(_call(who, fr, sj.SRC_RGBA, flatten=((1, 2, 3), 2, 255.0, 0.0)), who, "flatten: premultiplied 2 is not 0")
    _refused(_call(who, fr, unsharp=[(32, 0, 0, 1)]), who, "unsharp: reserved must be 0")
    if who != SHAPE:
        _refused(_call(who, fr, sj.SRC_GRAY, mode=sj.YUV_420), who, "yuv_mode does not match the source format", "gray pictures are coded 4:0:0 only")


def test_the_size_function():
    fr = _frames([(32, 16), (20, 10)])
    k, sp = _ptr([(64, 32), (5, 30)], np.int32, (-1, 2))
    k2, op = _ptr([1, 6], np.uint8, (-1,))
    assert L.sjpeg_hip_resample_ragged_bytes(sj.SRC_RGB, 2, fr, sp, None) == 64 * 3 * 32 + ((16 * 30 + 15) & ~15)
    assert L.sjpeg_hip_resample_ragged_bytes(sj.SRC_RGB, 2, fr, sp, op) == 64 * 3 * 32 + ((92 * 5 + 15) & ~15)     # (30 x 5 upright)
    assert L.sjpeg_hip_resample_ragged_bytes(sj.SRC_GRAY, 2, fr, sp, None) == 64 * 32 + ((8 * 30 + 15) & ~15)
    assert L.sjpeg_hip_resample_ragged_bytes(sj.SRC_RGB, 2, fr, None, None) == 96 * 16 + 60 * 10 + 8
    assert L.sjpeg_hip_resample_ragged_bytes(sj.SRC_NV12, 2, fr, sp, None) == 0
    assert L.sjpeg_hip_resample_ragged_bytes(sj.SRC_RGB, 2, None, sp, None) == 0
    k3, zp = _ptr([(64, 32), (0, 30)], np.int32, (-1, 2))
    assert L.sjpeg_hip_resample_ragged_bytes(sj.SRC_RGB, 2, fr, zp, None) == 0


def test_the_host_entries_refuse():
    who = "sjpeg_hip_resample_ksize"
    for args, words in (((5, 4, 4), "filter 5 is not one of"), ((-1, 4, 4), "filter -1"), ((0, 0, 4), "in 0 or out 4 is not one of 1..65535"),
                        ((0, 4, 65536), "in 4 or out 65536")):
        assert L.sjpeg_hip_resample_ksize(*args) == 0
        assert _err().startswith(who + ": ") and words in _err()
    who = "sjpeg_hip_resample_table"
    b, K = np.zeros((4, 2), np.int32), np.zeros((4, 7), np.int32)
    _refused(L.sjpeg_hip_resample_table(4, 2, 4, None, K.ctypes.data, 28), who, "bounds or K == NULL")
    _refused(L.sjpeg_hip_resample_table(4, 2, 4, b.ctypes.data, K.ctypes.data, 27), who, "K_capacity 27 is below the 28 coefficients")
    assert L.sjpeg_hip_resample_table(9, 2, 4, b.ctypes.data, K.ctypes.data, 28) == EINVAL and "filter 9" in _err()
    assert not K.any()


# ---- sjpeg_amd.resample

def test_module_names_and_signatures():
    import inspect
    assert [int(f) for f in rs.Filter] == [0, 1, 2, 3, 4] and rs.Filter.LANCZOS == 4 and rs.Filter.BOX == 0 and rs.KSIZE_MAX == 385
    assert C.sizeof(rs._ResampleStruct) == 4
    for fn, kws in ((rs.resample_images, ("images", "sizes", "filter", "orientations", "flatten", "engine", "layout")),
                    (rs.encode_resampled_images, ("images", "sizes", "box", "filter", "unsharp", "metadata", "packed", "orientations", "flatten",
                                                  "quality", "yuv_mode", "method", "use_trellis", "target_size", "target_psnr", "engine")),
                    (rs.resample_ragged, ("engine", "fmt", "planes_per_frame", "dims", "sizes", "filter", "orientations", "flatten", "unsharp", "out")),
                    (rs.encode_ragged_resampled, ("filter", "flatten", "unsharp", "search", "metadata", "packed")), (rs.resample_table, ("filter", "n_in", "n_out"))):
        names = list(inspect.signature(fn).parameters)
        for kw in kws:
            assert kw in names, (fn.__name__, kw)
        assert "light" not in names and "sheet" not in names
    assert inspect.signature(rs.resample_images).parameters["filter"].default == rs.Filter.LANCZOS
    # nothing public was added to the package itself
    assert not hasattr(sj, "Filter") and not hasattr(sj, "resample_images") and not hasattr(sj.Engine, "resample_ragged")


def test_module_refusals():
    for bad in (-1, 5, True, 1.5, "LANCZOS", None):
        with pytest.raises(sj.SjpegError, match="x: filter .* is not a Filter"):
            rs._filter("x", bad)
    with pytest.raises(sj.SjpegError, match=r"x: filter is one Filter or a sequence of one per frame \(2\)"):
        rs._filter_args("x", 2, [rs.Filter.BOX])
    with pytest.raises(sj.SjpegError, match="x: filter 'a' is not a Filter"):
        rs._filter_args("x", 2, ["a", "b"])
    with pytest.raises(sj.SjpegError, match="x: filter 1.5 is not a Filter or a sequence"):
        rs._filter_args("x", 2, 1.5)
    arr, addr, per = rs._filter_args("x", 2, [rs.Filter.BICUBIC, 4])
    assert per == 1 and bytes(arr) == bytes([3, 0, 0, 0, 4, 0, 0, 0]) and addr == C.addressof(arr)
    assert rs._filter_args("x", 2, rs.Filter.HAMMING)[2] == 0 and bytes(rs._filter_args("x", 2, 2)[0]) == bytes([2, 0, 0, 0])
    with pytest.raises(sj.SjpegError, match="resample_images: no images"):
        rs.resample_images([], (4, 4))
    with pytest.raises(sj.SjpegError, match="resample_images: flatten is not a Flatten"):
        rs.resample_images([], (4, 4), flatten=(255, 255, 255))
    with pytest.raises(sj.SjpegError, match="encode_resampled_images: layout 'xyz' is not"):
        rs.encode_resampled_images([], layout="xyz")
    with pytest.raises(sj.SjpegError, match="sjpeg_hip_resample_ksize failed: sjpeg_hip_resample_ksize: in 0 or out 4"):
        rs.resample_ksize(rs.Filter.BOX, 0, 4)
    b, K = rs.resample_table(rs.Filter.BILINEAR, 7, 3)
    assert b.tolist() == [[0, 4], [1, 5], [4, 3]] and K[1].tolist() == [246724, 986895, 1727066, 986895, 246724, 0, 0]


def test_abi_version_symbols_and_shared_constants():
    assert L.sjpeg_hip_abi_version() == 18           # (entries were added, none changed)
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    assert re.search(r"#define\s+SJPEG_HIP_ABI_VERSION\s+18\b", text)
    for name in ENTRIES + ("sjpeg_hip_resample_ksize", "sjpeg_hip_resample_table"):
        assert hasattr(L, name) and name in sj.EXPORTED_C_SYMBOLS, name
        assert re.search(r"\bint\s+%s\(" % name, text), name
    assert hasattr(L, "sjpeg_hip_resample_ragged_bytes") and "sjpeg_hip_resample_ragged_bytes" in sj.EXPORTED_C_SYMBOLS
    assert re.search(r"\bsize_t\s+sjpeg_hip_resample_ragged_bytes\(", text)
    assert re.search(r"typedef struct sjpeg_hip_resample \{\s*uint8_t filter;[^}]*uint8_t reserved\[3\];", text)
    for k, name in enumerate(("BOX", "BILINEAR", "HAMMING", "BICUBIC", "LANCZOS")):
        assert re.search(r"#define\s+SJPEG_HIP_RESAMPLE_%s\s+%d\b" % (name, k), text)
    assert "is refused\n * before any device work" in text and "An axis whose ksize is above 385" in text
    assert "NOT exif_transpose followed by resize" in text and "no `light` and no sheet argument" in text
    # the tile, the stage and the cap are stated once, for the plan and the kernel
    csrc = os.path.join(ROOT, "sjpeg_amd", "csrc")
    aux = open(os.path.join(csrc, "ragged_aux.h")).read()
    assert "constexpr unsigned kResampleTileCols = 32, kResampleTileRows = 16, kResampleStageBytes = 16384, kResampleSegmentMax = 4096;" in aux
    assert "constexpr int kResampleKsizeMax = 385;" in aux
    kernel = open(os.path.join(csrc, "resample.hip")).read()
    for word in ("sjpeg_internal::kResampleStageBytes", "sjpeg_internal::kResampleTileCols", "sjpeg_internal::kResampleTileRows",
                 "sjpeg_internal::kResampleSegmentMax"):
        assert word in kernel, word
    assert "kResampleKsizeMax" in open(os.path.join(csrc, "resample_plan.cc")).read()
    # the kernel, the host and the stand-alone tests share one statement of the arithmetic
    for f in ("resample.hip", "resample_plan.cc"):
        assert '#include "resample_math.h"' in open(os.path.join(csrc, f)).read()
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^HOST_SRCS := .*\bresample_plan\b", mk, re.M) and re.search(r"^HIP_SRCS := .*\bresample\b", mk, re.M)
