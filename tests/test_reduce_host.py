"""Pictures reduced inside the ragged call (sjpeg_hip_reduce_ragged_src, sjpeg_hip_encode_ragged_reduced_src, Reduced)
without a GPU: the sizes, the layout of the reduced buffer, every argument check before any device work (the frame
named), the exports, the Reduced wrapper and the pinned signatures."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import sjpeg_amd as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = C.c_void_p(1 << 20)          # (the checks come before the engine is touched: any non-NULL value stands in for one)
NEW = ("sjpeg_hip_reduced_size", "sjpeg_hip_reduce_ragged_bytes", "sjpeg_hip_reduce_ragged_src",
       "sjpeg_hip_encode_ragged_reduced_src", "sjpeg_hip_encode_ragged_reduced_packed_src")
REDUCE = "sjpeg_hip_reduce_ragged_src"
ENCODE = "sjpeg_hip_encode_ragged_reduced_src"
PACKED = "sjpeg_hip_encode_ragged_reduced_packed_src"


def _err():
    return sj.lib().sjpeg_hip_last_error().decode()


def _refused(rc, who, *words):
    assert rc == EINVAL
    msg = _err()
    assert who in msg, msg
    for w in words:
        assert w in msg, (w, msg)


# ---- sizes

def test_reduced_size_for_every_factor():
    for (w, h) in ((1, 1), (17, 9), (65535, 65535)):
        for s in range(1, 9):
            assert sj.reduced_size(w, h, s) == ((w + s - 1) // s, (h + s - 1) // s)
    assert sj.reduced_size(17, 9, 8) == (3, 2)
    assert sj.reduced_size(130, 70, 1) == (130, 70)


def test_reduced_size_refusals():
    L = sj.lib()
    rw, rh = C.c_int(7), C.c_int(7)
    for s in (0, 9, -1, 256):
        _refused(L.sjpeg_hip_reduced_size(16, 16, s, C.byref(rw), C.byref(rh)), "sjpeg_hip_reduced_size", "factor")
    for (w, h) in ((0, 4), (4, 0), (65536, 4), (4, 65536), (-1, 4)):
        _refused(L.sjpeg_hip_reduced_size(w, h, 2, C.byref(rw), C.byref(rh)), "sjpeg_hip_reduced_size", "dimensions")
    _refused(L.sjpeg_hip_reduced_size(16, 16, 2, None, C.byref(rh)), "sjpeg_hip_reduced_size", "NULL")
    _refused(L.sjpeg_hip_reduced_size(16, 16, 2, C.byref(rw), None), "sjpeg_hip_reduced_size", "NULL")
    assert (rw.value, rh.value) == (7, 7)          # nothing was written
    with pytest.raises(sj.SjpegError, match="factor 9"):
        sj.reduced_size(16, 16, 9)


# ---- the reduced buffer

def _frames(dims, fmt=sj.SRC_RGB, planes=1):
    """frames of `planes` planes each, wide strides: in order for every byte format"""
    f = (sj.RaggedFrame * len(dims))()
    for k, (w, h) in enumerate(dims):
        f[k].width, f[k].height = w, h
        for i in range(planes):
            f[k].plane[i] = (1 << 30) + (i << 24)
            f[k].row_stride[i] = 1 << 19
        f[k].out_offset = (1 << 20) * k
        f[k].out_capacity = 1 << 20
    return f


def _bytes(fmt, frames, factors):
    fac = None if factors is None else (C.c_uint8 * len(factors))(*factors)
    return sj.lib().sjpeg_hip_reduce_ragged_bytes(fmt, len(frames), frames, None if fac is None else C.cast(fac, C.c_void_p))


def _layout(dims, factors, channels):
    """The documented layout, restated: rows a multiple of 4 apart, pictures at multiples of 16.  Returns the bytes and,
    per picture, (base, row stride, w', h')."""
    at, out = 0, []
    for (w, h), s in zip(dims, factors):
        w2, h2 = (w + s - 1) // s, (h + s - 1) // s
        rs = (w2 * channels + 3) & ~3
        out.append((at, rs, w2, h2))
        at += (rs * h2 + 15) & ~15
    return at, out


@pytest.mark.parametrize("fmt,channels,planes", [(sj.SRC_RGB, 3, 1), (sj.SRC_BGRA, 3, 1), (sj.SRC_RGB_PLANAR, 3, 3),
                                                 (sj.SRC_GRAY, 1, 1), (sj.SRC_GRAY_F16, 1, 1), (sj.SRC_RGBA_BF16, 3, 1)])
def test_reduce_ragged_bytes_holds_every_row_and_padded_store(fmt, channels, planes):
    # w' of 1, of 5, and a multiple of 4 -- and a batch of all three
    cases = [([(8, 9)], [8]), ([(17, 9)], [8]), ([(1, 1)], [1]),            # w' = 1 .. 3
             ([(5, 3)], [1]), ([(10, 7)], [2]), ([(40, 2)], [8]),           # w' = 5
             ([(8, 8)], [2]), ([(64, 5)], [8]), ([(12, 1)], [1]),           # w' = 4, 8, 12
             ([(8, 9), (10, 7), (64, 5), (130, 70)], [8, 2, 8, 3])]
    for dims, factors in cases:
        got = _bytes(fmt, _frames(dims, fmt, planes), factors)
        want, pics = _layout(dims, factors, channels)
        assert got == want and got % 16 == 0, (dims, factors, got, want)
        for k, (base, rs, w2, h2) in enumerate(pics):
            assert base % 16 == 0 and rs % 4 == 0 and rs >= w2 * channels
            # the kernel stores whole dwords: a group of four reduced pixels is 12 bytes of RGB or 4 of gray, and only
            # the dwords that START inside the row are written -- so the furthest store ends at the row's end at most
            group = 12 if channels == 3 else 4
            stores = [g * group + 4 * d for g in range((w2 + 3) // 4) for d in range(group // 4) if g * group + 4 * d < rs]
            assert max(stores) + 4 <= rs
            end = base + (h2 - 1) * rs + max(stores) + 4
            assert end <= (pics[k + 1][0] if k + 1 < len(pics) else got)
    # factors NULL: all 1
    assert _bytes(fmt, _frames([(5, 3)], fmt, planes), None) == _layout([(5, 3)], [1], channels)[0]


def test_reduce_ragged_bytes_is_zero_on_bad_arguments():
    fr = _frames([(16, 16)])
    assert _bytes(sj.SRC_RGB, fr, [0]) == 0 and "factor 0" in _err()
    assert _bytes(sj.SRC_RGB, fr, [9]) == 0 and "factor 9" in _err()
    assert _bytes(99, fr, [1]) == 0
    assert _bytes(sj.SRC_NV12, _frames([(16, 16)], planes=2), [2]) == 0 and "SJPEG_HIP_SRC_NV12" in _err()
    assert sj.lib().sjpeg_hip_reduce_ragged_bytes(sj.SRC_RGB, 1, None, None) == 0
    assert sj.lib().sjpeg_hip_reduce_ragged_bytes(sj.SRC_RGB, 0, fr, None) == 0
    bad = _frames([(0, 16)])
    assert _bytes(sj.SRC_RGB, bad, [1]) == 0 and "frame 0" in _err()


# ---- argument checks with a stand-in engine: nothing touches it

def _params(mode, method=4):
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, method, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    p._keep = q
    return p


def _reduce(frames, fmt, factors, reduced_bytes=1 << 30, d_reduced=1 << 28):
    n = len(frames)
    fac = (C.c_uint8 * n)(*factors)
    out = (sj.RaggedFrame * n)()
    rfmt = C.c_int(-7)
    rc = sj.lib().sjpeg_hip_reduce_ragged_src(FAKE, fmt, n, frames, C.cast(fac, C.c_void_p), d_reduced, reduced_bytes, out,
                                              C.byref(rfmt), None)
    assert rfmt.value == -7                       # refused: nothing was reported
    return rc


def _encode(frames, fmt, factors, mode=sj.YUV_420):
    n = len(frames)
    fac = None if factors is None else C.cast((C.c_uint8 * n)(*factors), C.c_void_p)
    p = _params(mode)
    return sj.lib().sjpeg_hip_encode_ragged_reduced_src(FAKE, fmt, n, frames, C.byref(p), fac, None, 0, 1 << 16, 1 << 12,
                                                        None, None, None, None)


def _packed(frames, fmt, factors, mode=sj.YUV_420):
    n = len(frames)
    fac = None if factors is None else C.cast((C.c_uint8 * n)(*factors), C.c_void_p)
    p = _params(mode)
    return sj.lib().sjpeg_hip_encode_ragged_reduced_packed_src(FAKE, fmt, n, frames, C.byref(p), fac, None, 0, 1 << 16, 1 << 20,
                                                               1 << 12, 1 << 13, None, None, None, None)


@pytest.mark.parametrize("call,who", [(_reduce, REDUCE), (_encode, ENCODE), (_packed, PACKED)])
def test_factor_outside_1_to_8_names_the_frame(call, who):
    fr = _frames([(16, 16), (17, 9), (8, 8)])
    _refused(call(fr, sj.SRC_RGB, [2, 0, 4]), who, "frame 1", "factor 0")
    _refused(call(fr, sj.SRC_RGB, [1, 1, 9]), who, "frame 2", "factor 9")
    _refused(call(fr, sj.SRC_RGBA_F16, [9, 1, 1]), who, "frame 0", "factor 9")


@pytest.mark.parametrize("call,who", [(_reduce, REDUCE), (_encode, ENCODE), (_packed, PACKED)])
def test_yuv_plane_formats_are_not_reduced(call, who):
    for fmt, name, planes in ((sj.SRC_NV12, "SJPEG_HIP_SRC_NV12", 2), (sj.SRC_NV21, "SJPEG_HIP_SRC_NV21", 2),
                              (sj.SRC_YUV420, "SJPEG_HIP_SRC_YUV420", 3), (sj.SRC_YUV444, "SJPEG_HIP_SRC_YUV444", 3)):
        mode = sj.YUV_444 if fmt == sj.SRC_YUV444 else sj.YUV_420
        fr = _frames([(16, 16), (32, 8)], planes=planes)
        args = (fr, fmt, [1, 2]) if call is _reduce else (fr, fmt, [1, 2], mode)
        _refused(call(*args), who, name)


@pytest.mark.parametrize("call,inner", [(_encode, "sjpeg_hip_encode_ragged_full_src"), (_packed, "sjpeg_hip_encode_ragged_full_packed_src")])
def test_all_ones_is_the_plain_call_with_its_own_checks(call, inner):
    """NV12 with every factor 1 (or no factors) is not refused for its format: the call is the _full_ call, whose own
    checks answer -- here, in its own name, for a sampling NV12 does not have and for a frame out of order."""
    fr = _frames([(16, 16), (32, 8)], planes=2)
    for factors in ([1, 1], None):
        _refused(call(fr, sj.SRC_NV12, factors, sj.YUV_444), inner, "yuv_mode does not match the source format")
        bad = _frames([(16, 16), (32, 8)], planes=2)
        bad[1].row_stride[1] = 8
        _refused(call(bad, sj.SRC_NV12, factors, sj.YUV_420), inner, "frame 1", "row_stride")


@pytest.mark.parametrize("call,who", [(_encode, ENCODE), (_packed, PACKED)])
def test_gray_is_400_only(call, who):
    for fmt in (sj.SRC_GRAY, sj.SRC_GRAY_F32, sj.SRC_GRAY_F16, sj.SRC_GRAY_BF16):
        for mode in (sj.YUV_420, sj.YUV_444):
            _refused(call(_frames([(16, 16)]), fmt, [2], mode), who, "yuv_mode")
        for mode in (sj.YUV_AUTO, sj.YUV_SHARP):
            assert call(_frames([(16, 16)]), fmt, [2], mode) == EINVAL and who in _err()


def test_reduced_bytes_one_short():
    dims, factors = [(17, 9), (130, 70), (8, 8)], [8, 3, 1]
    fr = _frames(dims)
    need = _bytes(sj.SRC_RGB, fr, factors)
    assert need == _layout(dims, factors, 3)[0]
    _refused(_reduce(fr, sj.SRC_RGB, factors, reduced_bytes=need - 1), REDUCE, "reduced_bytes", str(need))
    _refused(_reduce(fr, sj.SRC_RGB, factors, reduced_bytes=0), REDUCE, "reduced_bytes")
    _refused(_reduce(fr, sj.SRC_RGB, factors, d_reduced=(1 << 28) + 4), REDUCE, "multiple of 16")


@pytest.mark.parametrize("call,who", [(_reduce, REDUCE), (_encode, ENCODE), (_packed, PACKED)])
def test_the_frame_checks_of_the_ragged_entries(call, who):
    def two():
        return _frames([(16, 16), (16, 16)])
    f = two(); f[1].plane[0] = None
    _refused(call(f, sj.SRC_RGB, [2, 2]), who, "frame 1", "null plane")
    f = two(); f[1].row_stride[0] = 47
    _refused(call(f, sj.SRC_RGB, [2, 2]), who, "frame 1", "row_stride")
    f = two(); f[1].row_stride[0] = -47
    _refused(call(f, sj.SRC_RGB, [2, 2]), who, "frame 1", "row_stride")
    f = two(); f[0].width = 0
    _refused(call(f, sj.SRC_RGB, [2, 2]), who, "frame 0", "dimensions")
    f = two(); f[1].row_stride[0] = 1025
    _refused(call(f, sj.SRC_RGB_F16, [2, 2]), who, "frame 1", "row_stride[0]", "element size")
    f = two(); f[1].out_offset, f[1].out_capacity = 2 ** 64 - 1, 2
    _refused(call(f, sj.SRC_RGB, [2, 2]), who, "frame 1", "out_offset + out_capacity")
    # planar RGB: one pitch
    f = _frames([(16, 16), (16, 16)], planes=3); f[1].row_stride[2] = 1 << 18
    _refused(call(f, sj.SRC_RGB_PLANAR, [2, 2]), who, "frame 1", "row_stride[2]")


def test_null_arguments():
    L = sj.lib()
    fr = _frames([(16, 16)])
    fac = C.cast((C.c_uint8 * 1)(2), C.c_void_p)
    out = (sj.RaggedFrame * 1)()
    rfmt = C.c_int(0)
    p = _params(sj.YUV_420)
    assert L.sjpeg_hip_reduce_ragged_src(None, 0, 1, fr, fac, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_reduce_ragged_src(FAKE, 0, 1, None, fac, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_reduce_ragged_src(FAKE, 0, 1, fr, None, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_reduce_ragged_src(FAKE, 0, 1, fr, fac, None, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_reduce_ragged_src(FAKE, 0, 1, fr, fac, 1 << 28, 1 << 20, None, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_reduce_ragged_src(FAKE, 0, 1, fr, fac, 1 << 28, 1 << 20, out, None, None) == EINVAL
    assert L.sjpeg_hip_reduce_ragged_src(FAKE, 0, 0, fr, fac, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_reduce_ragged_src(FAKE, 99, 1, fr, fac, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    for args in ((None, 0, 1, fr, C.byref(p), fac, None, 0, 1 << 16, 1 << 12), (FAKE, 0, 1, fr, None, fac, None, 0, 1 << 16, 1 << 12),
                 (FAKE, 0, 1, None, C.byref(p), fac, None, 0, 1 << 16, 1 << 12), (FAKE, 0, 1, fr, C.byref(p), fac, None, 0, None, 1 << 12),
                 (FAKE, 0, 1, fr, C.byref(p), fac, None, 0, 1 << 16, None), (FAKE, 0, 0, fr, C.byref(p), fac, None, 0, 1 << 16, 1 << 12)):
        assert L.sjpeg_hip_encode_ragged_reduced_src(*args, None, None, None, None) == EINVAL
        assert ENCODE in _err()
    # the inner call's parameter checks come before any device work too
    bad = _params(sj.YUV_420, method=9)
    assert L.sjpeg_hip_encode_ragged_reduced_src(FAKE, 0, 1, fr, C.byref(bad), fac, None, 0, 1 << 16, 1 << 12, None, None, None, None) == EINVAL
    assert "method" in _err()
    assert L.sjpeg_hip_encode_ragged_reduced_packed_src(FAKE, 0, 1, fr, C.byref(p), fac, None, 0, (1 << 16) + 8, 1 << 20, 1 << 12, 1 << 13,
                                                        None, None, None, None) == EINVAL
    assert "multiple of 16" in _err()


# ---- exports

def test_symbols_are_exported_and_declared():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    declared = set(re.findall(r"\b(sjpeg_hip_[a-z_0-9]+)\s*\(", text.split("namespace sjpeg")[0]))
    for name in NEW:
        assert name in sj.EXPORTED_C_SYMBOLS and name in declared, name
        getattr(sj.lib(), name)
    assert declared == set(n for n in sj.EXPORTED_C_SYMBOLS if n.startswith("sjpeg_hip_"))
    assert re.search(r"#define\s+SJPEG_HIP_REDUCE_MAX\s+8\b", text) and sj.REDUCE_MAX == 8
    assert re.search(r"#define\s+SJPEG_HIP_ABI_VERSION\s+18\b", text) and sj.lib().sjpeg_hip_abi_version() == 18
    # no new source format
    assert "SJPEG_HIP_SRC_GRAY_BF16 = 20\n};" in text


# ---- Reduced

def test_reduced_wrapper():
    ims = [np.zeros((8, 8, 3), np.uint8), np.zeros((4, 6, 3), np.uint8), np.zeros((3, 3, 3), np.uint8)]
    r = sj.Reduced(ims, 2)
    assert r.factors == [2, 2, 2] and r.images == ims
    r = sj.Reduced(ims, [1, 4, 8])
    assert r.factors == [1, 4, 8]
    assert sj.Reduced(ims, np.array([1, 2, 3])).factors == [1, 2, 3]
    assert sj.Reduced(tuple(ims), np.int64(3)).factors == [3, 3, 3]
    with pytest.raises(sj.SjpegError, match="2 factors for 3 pictures"):
        sj.Reduced(ims, [2, 2])
    with pytest.raises(sj.SjpegError, match="4 factors for 3 pictures"):
        sj.Reduced(ims, [2, 2, 2, 2])
    for bad in (0, 9, -1):
        with pytest.raises(sj.SjpegError, match="picture 1"):
            sj.Reduced(ims, [1, bad, 1])
        with pytest.raises(sj.SjpegError, match="1..8"):
            sj.Reduced(ims, bad)
    with pytest.raises(sj.SjpegError, match="picture 0"):
        sj.Reduced(ims, 2.0)
    # a wrapped FloatPixels keeps its transform
    fp = sj.FloatPixels(ims, 127.5, 127.5)
    r = sj.Reduced(fp, [1, 2, 4])
    assert r.images is fp and r.factors == [1, 2, 4]
    with pytest.raises(sj.SjpegError, match="1 factors for 3 pictures"):
        sj.Reduced(fp, [2])
    # all ones: nothing to reduce
    assert sj._reduced(sj.Reduced(ims, 1)) == (ims, None)
    assert sj._reduced(sj.Reduced(ims, [1, 2, 1])) == (ims, [1, 2, 1])
    assert sj._reduced(ims) == (ims, None)
    assert sj._reduced(sj.Reduced(fp, 3))[0] is fp


def test_reduced_goes_through_the_calls_own_checks():
    """A Reduced is unwrapped first: the calls answer for its pictures as they answer for plain ones."""
    hwc = [np.zeros((8, 8, 3), np.uint8)]
    for call in (lambda r: sj.encode_images(r), lambda r: sj.compress_images(r), lambda r: sj.encode_images_full(r),
                 lambda r: sj.encode_images_full_meta(r, None), lambda r: sj.reduce_images(hwc, 2)):
        with pytest.raises(sj.SjpegError, match="image 0"):
            call(sj.Reduced(hwc, 2))
    with pytest.raises(sj.SjpegError, match="image 0 is not a CUDA tensor"):
        sj.encode_images_full_chw(sj.Reduced([np.zeros((3, 8, 8), np.uint8)], 2))
    with pytest.raises(sj.SjpegError, match="layout='chw'"):
        sj.encode_images(sj.Reduced(sj.FloatPixels(hwc), 2))
    with pytest.raises(sj.SjpegError, match="layout"):
        sj.reduce_images(hwc, 2, layout="nhwc")
    with pytest.raises(sj.SjpegError, match="1..8"):
        sj.reduce_images(hwc, 0)


def test_riskiness_images_refuses_reduced():
    ims = [np.zeros((8, 8, 3), np.uint8)]
    for layout in ("hwc", "chw"):
        with pytest.raises(sj.SjpegError, match="reduce first"):
            sj.riskiness_images(sj.Reduced(ims, 2), layout=layout)
    with pytest.raises(sj.SjpegError, match="reduce_images"):
        sj.riskiness_images(sj.Reduced(ims, 1))


# ---- the pinned signatures of the existing functions, unchanged

def test_pinned_signatures_still_hold():
    for fn in (sj.encode_images, sj.compress_images, sj.riskiness_images):
        sig = inspect.signature(fn).parameters
        assert list(sig)[0] == "images" and list(sig)[-1] == "layout" and sig["layout"].default == "hwc", fn.__name__
    sig = inspect.signature(sj.encode_images_full).parameters
    want = dict(quality=75.0, yuv_mode=sj.YUV_AUTO, method=4, use_trellis=False, target_size=None, target_psnr=None,
                passes=10, tolerance=1.0, qmin=0.0, qmax=100.0, min_quant=None, q_bias=0x78, dmax_luma=12, dmax_chroma=1,
                engine=None, packed=False)
    assert list(sig)[0] == "images" and list(sig)[1:] == list(want)
    for k, v in want.items():
        assert sig[k].default == v or sig[k].default is v, k
    assert list(inspect.signature(sj.encode_images_full_chw).parameters) == list(sig)
    assert list(inspect.signature(sj.encode_images_full_meta).parameters) == ["images", "metadata", "layout", "params"]
    assert list(inspect.signature(sj.encode_images).parameters) == [
        "images", "quality", "yuv_mode", "engine", "method", "min_quant", "q_bias", "dmax_luma", "dmax_chroma", "target_size",
        "target_psnr", "passes", "tolerance", "qmin", "qmax", "use_trellis", "packed", "metadata", "layout"]
    assert list(inspect.signature(sj.compress_images).parameters) == ["images", "quality", "engine", "use_trellis", "packed",
                                                                      "metadata", "layout"]
    assert list(inspect.signature(sj.riskiness_images).parameters) == ["images", "engine", "layout"]
    assert list(inspect.signature(sj.FloatPixels).parameters) == ["images", "scale", "bias"]
    # the new names
    assert list(inspect.signature(sj.Reduced).parameters) == ["images", "factor"]
    assert list(inspect.signature(sj.reduce_images).parameters) == ["images", "factor", "engine", "layout"]
    assert inspect.signature(sj.reduce_images).parameters["layout"].default == "hwc"
    assert list(inspect.signature(sj.reduced_size).parameters) == ["w", "h", "factor"]
    assert list(inspect.signature(sj.Engine.reduce_ragged).parameters)[:5] == ["self", "fmt", "planes_per_frame", "dims", "factors"]
    for name in ("encode_ragged_reduced", "encode_ragged_reduced_packed"):
        assert list(inspect.signature(getattr(sj.Engine, name)).parameters)[:5] == ["self", "fmt", "planes_per_frame", "dims", "factors"]
