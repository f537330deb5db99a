"""Pictures resized inside the ragged call (sjpeg_hip_resize_ragged_src, sjpeg_hip_encode_ragged_resized_src, Resized)
without a GPU: the fitted size, the layout of the resized buffer, every argument check before any device work (the
frame named), the exports, and the Resized wrapper."""
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
NEW = ("sjpeg_hip_fit_size", "sjpeg_hip_resize_ragged_bytes", "sjpeg_hip_resize_ragged_src",
       "sjpeg_hip_encode_ragged_resized_src", "sjpeg_hip_encode_ragged_resized_packed_src")
RESIZE = "sjpeg_hip_resize_ragged_src"
ENCODE = "sjpeg_hip_encode_ragged_resized_src"
PACKED = "sjpeg_hip_encode_ragged_resized_packed_src"


def _err():
    return sj.lib().sjpeg_hip_last_error().decode()


def _refused(rc, who, *words):
    assert rc == EINVAL
    msg = _err()
    assert who in msg, msg
    for w in words:
        assert w in msg, (w, msg)


# ---- the fitted size

def _fit(W, H, bw, bh):
    """the issue's three lines, restated"""
    if W <= bw and H <= bh:
        return W, H
    if W * bh >= H * bw:
        return bw, max(1, (H * bw + W // 2) // W)
    return max(1, (W * bh + H // 2) // H), bh


def test_fit_size():
    # a box at least as large as the picture: never larger
    assert sj.fit_size(100, 50, (256, 256)) == (100, 50)
    assert sj.fit_size(256, 256, (256, 256)) == (256, 256)
    assert sj.fit_size(1, 1, (65535, 65535)) == (1, 1)
    # bound by the width, by the height, and one side inside the box already
    assert sj.fit_size(4000, 3000, (256, 256)) == (256, 192)
    assert sj.fit_size(3000, 4000, (256, 256)) == (192, 256)
    assert sj.fit_size(4000, 100, (320, 65535)) == (320, 8)
    assert sj.fit_size(100, 4000, (256, 1024)) == (26, 1024)
    assert sj.fit_size(1000, 1000, (300, 200)) == (200, 200)
    # the tie goes up: 5 * 2 / 4 = 2.5 and 3 * 2 / 4 = 1.5
    assert sj.fit_size(4, 5, (4, 2)) == (2, 2) and _fit(4, 5, 4, 2) == (2, 2)
    assert sj.fit_size(4, 3, (2, 3)) == (2, 2)
    assert sj.fit_size(5, 4, (2, 4)) == (2, 2)
    assert sj.fit_size(8, 5, (4, 5)) == (4, 3)          # 2.5 -> 3
    assert sj.fit_size(8, 3, (4, 3)) == (4, 2)          # 1.5 -> 2
    assert sj.fit_size(8, 1, (4, 1)) == (4, 1)          # 0.5 -> 1
    # the clamp: a side that rounds to 0 is 1
    assert sj.fit_size(65535, 1, (256, 256)) == (256, 1)
    assert sj.fit_size(1, 65535, (256, 256)) == (1, 256)
    assert sj.fit_size(1000, 1, (2, 2)) == (2, 1)
    assert sj.fit_size(65535, 65535, (1, 1)) == (1, 1)
    rng = np.random.default_rng(5)
    for _ in range(2000):
        W, H, bw, bh = (int(v) for v in rng.integers(1, 65536, 4))
        if rng.integers(0, 2):
            bw, bh = 1 + bw % 300, 1 + bh % 300
        w, h = sj.fit_size(W, H, (bw, bh))
        assert (w, h) == _fit(W, H, bw, bh) and 1 <= w <= min(W, bw) and 1 <= h <= min(H, bh), (W, H, bw, bh, w, h)


def test_fit_size_refusals():
    L = sj.lib()
    fw, fh = C.c_int(7), C.c_int(7)
    for (w, h) in ((0, 4), (4, 0), (65536, 4), (4, 65536), (-1, 4)):
        _refused(L.sjpeg_hip_fit_size(w, h, 16, 16, C.byref(fw), C.byref(fh)), "sjpeg_hip_fit_size", "dimensions")
        _refused(L.sjpeg_hip_fit_size(16, 16, w, h, C.byref(fw), C.byref(fh)), "sjpeg_hip_fit_size", "box")
    _refused(L.sjpeg_hip_fit_size(16, 16, 4, 4, None, C.byref(fh)), "sjpeg_hip_fit_size", "NULL")
    _refused(L.sjpeg_hip_fit_size(16, 16, 4, 4, C.byref(fw), None), "sjpeg_hip_fit_size", "NULL")
    assert (fw.value, fh.value) == (7, 7)          # nothing was written
    with pytest.raises(sj.SjpegError, match="bad box 0x5"):
        sj.fit_size(16, 16, (0, 5))
    with pytest.raises(sj.SjpegError, match="pair"):
        sj.fit_size(16, 16, 256)


# ---- the resized buffer

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


def _sizes(sizes):
    if sizes is None:
        return None, None
    arr = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(len(sizes), 2))
    return arr, arr.ctypes.data


def _bytes(fmt, frames, sizes):
    keep, ptr = _sizes(sizes)
    return sj.lib().sjpeg_hip_resize_ragged_bytes(fmt, len(frames), frames, ptr)


def _layout(sizes, channels):
    """The documented layout, restated: rows a multiple of 4 apart, pictures at multiples of 16.  Returns the bytes and,
    per picture, (base, row stride, w', h')."""
    at, out = 0, []
    for (w2, h2) in sizes:
        rs = (w2 * channels + 3) & ~3
        out.append((at, rs, w2, h2))
        at += (rs * h2 + 15) & ~15
    return at, out


@pytest.mark.parametrize("fmt,channels,planes", [(sj.SRC_RGB, 3, 1), (sj.SRC_BGRA, 3, 1), (sj.SRC_RGB_PLANAR, 3, 3),
                                                 (sj.SRC_GRAY, 1, 1), (sj.SRC_GRAY_F16, 1, 1), (sj.SRC_RGBA_BF16, 3, 1)])
def test_resize_ragged_bytes_holds_every_row_and_padded_store(fmt, channels, planes):
    cases = [([(8, 9)], [(1, 2)]), ([(17, 9)], [(3, 9)]), ([(1, 1)], [(1, 1)]),
             ([(5, 3)], [(5, 3)]), ([(10, 7)], [(5, 1)]), ([(40, 2)], [(7, 2)]),
             ([(8, 8)], [(4, 4)]), ([(64, 5)], [(8, 5)]), ([(1030, 9)], [(1029, 8)]),
             ([(8, 9), (10, 7), (64, 5), (130, 70), (300, 40)], [(2, 9), (5, 3), (63, 1), (129, 1), (7, 3)])]
    for dims, sizes in cases:
        got = _bytes(fmt, _frames(dims, fmt, planes), sizes)
        want, pics = _layout(sizes, channels)
        assert got == want and got % 16 == 0, (dims, sizes, got, want)
        for k, (base, rs, w2, h2) in enumerate(pics):
            assert base % 16 == 0 and rs % 4 == 0 and rs >= w2 * channels
            # the kernel stores the dwords that hold a byte of the row, whatever the tile: the furthest ends at the
            # row's end at most, and the last row's inside the picture's slot
            last = (w2 * channels + 3) // 4 * 4
            assert last <= rs
            assert base + (h2 - 1) * rs + last <= (pics[k + 1][0] if k + 1 < len(pics) else got)
    # sizes NULL: every frame at its own size
    assert _bytes(fmt, _frames([(5, 3), (9, 2)], fmt, planes), None) == _layout([(5, 3), (9, 2)], channels)[0]


def test_resize_ragged_bytes_is_zero_on_bad_arguments():
    fr = _frames([(16, 16)])
    assert _bytes(sj.SRC_RGB, fr, [(0, 4)]) == 0 and "size 0x4" in _err()
    assert _bytes(sj.SRC_RGB, fr, [(4, -1)]) == 0 and "frame 0" in _err()
    assert _bytes(sj.SRC_RGB, fr, [(17, 4)]) == 0 and "size 17x4" in _err()
    assert _bytes(sj.SRC_RGB, fr, [(4, 17)]) == 0 and "above the source's 16x16" in _err()
    assert _bytes(99, fr, [(4, 4)]) == 0
    assert _bytes(sj.SRC_NV12, _frames([(16, 16)], planes=2), [(8, 8)]) == 0 and "SJPEG_HIP_SRC_NV12" in _err()
    assert sj.lib().sjpeg_hip_resize_ragged_bytes(sj.SRC_RGB, 1, None, None) == 0
    assert sj.lib().sjpeg_hip_resize_ragged_bytes(sj.SRC_RGB, 0, fr, None) == 0
    bad = _frames([(0, 16)])
    assert _bytes(sj.SRC_RGB, bad, [(1, 1)]) == 0 and "frame 0" in _err()


# ---- argument checks with a stand-in engine: nothing touches it

def _params(mode, method=4):
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, method, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    p._keep = q
    return p


def _resize(frames, fmt, sizes, resized_bytes=1 << 30, d_resized=1 << 28):
    n = len(frames)
    keep, ptr = _sizes(sizes)
    out = (sj.RaggedFrame * n)()
    rfmt = C.c_int(-7)
    rc = sj.lib().sjpeg_hip_resize_ragged_src(FAKE, fmt, n, frames, ptr, d_resized, resized_bytes, out, C.byref(rfmt), None)
    assert rfmt.value == -7                       # refused: nothing was reported
    return rc


def _encode(frames, fmt, sizes, mode=sj.YUV_420):
    keep, ptr = _sizes(sizes)
    p = _params(mode)
    return sj.lib().sjpeg_hip_encode_ragged_resized_src(FAKE, fmt, len(frames), frames, C.byref(p), ptr, None, 0, 1 << 16, 1 << 12,
                                                        None, None, None, None)


def _packed(frames, fmt, sizes, mode=sj.YUV_420):
    keep, ptr = _sizes(sizes)
    p = _params(mode)
    return sj.lib().sjpeg_hip_encode_ragged_resized_packed_src(FAKE, fmt, len(frames), frames, C.byref(p), ptr, None, 0, 1 << 16,
                                                               1 << 20, 1 << 12, 1 << 13, None, None, None, None)


ALL = [(_resize, RESIZE), (_encode, ENCODE), (_packed, PACKED)]


@pytest.mark.parametrize("call,who", ALL)
def test_a_size_below_1_names_the_frame(call, who):
    fr = _frames([(16, 16), (17, 9), (8, 8)])
    _refused(call(fr, sj.SRC_RGB, [(8, 8), (0, 4), (4, 4)]), who, "frame 1", "size 0x4", "below 1")
    _refused(call(fr, sj.SRC_RGB, [(8, 8), (17, 9), (4, -3)]), who, "frame 2", "size 4x-3", "below 1")
    _refused(call(fr, sj.SRC_RGBA_F16, [(0, 0), (1, 1), (1, 1)]), who, "frame 0", "below 1")


@pytest.mark.parametrize("call,who", ALL)
def test_a_size_above_the_source_names_the_frame(call, who):
    fr = _frames([(16, 16), (17, 9), (8, 8)])
    _refused(call(fr, sj.SRC_RGB, [(8, 8), (18, 9), (4, 4)]), who, "frame 1", "size 18x9", "above the source's 17x9")
    _refused(call(fr, sj.SRC_RGB, [(8, 8), (17, 9), (8, 9)]), who, "frame 2", "size 8x9", "above the source's 8x8")
    _refused(call(fr, sj.SRC_GRAY, [(65535, 1), (1, 1), (1, 1)], *(() if call is _resize else (sj.YUV_400,))), who, "frame 0", "above")


@pytest.mark.parametrize("call,who", ALL)
def test_yuv_plane_formats_are_not_resized(call, who):
    for fmt, name, planes in ((sj.SRC_NV12, "SJPEG_HIP_SRC_NV12", 2), (sj.SRC_NV21, "SJPEG_HIP_SRC_NV21", 2),
                              (sj.SRC_YUV420, "SJPEG_HIP_SRC_YUV420", 3), (sj.SRC_YUV444, "SJPEG_HIP_SRC_YUV444", 3)):
        mode = sj.YUV_444 if fmt == sj.SRC_YUV444 else sj.YUV_420
        fr = _frames([(16, 16), (32, 8)], planes=planes)
        sizes = [(16, 16), (16, 8)]
        args = (fr, fmt, sizes) if call is _resize else (fr, fmt, sizes, mode)
        _refused(call(*args), who, name, "not resized")


@pytest.mark.parametrize("call,inner", [(_encode, "sjpeg_hip_encode_ragged_full_src"), (_packed, "sjpeg_hip_encode_ragged_full_packed_src")])
def test_own_sizes_are_the_plain_call_with_its_own_checks(call, inner):
    """NV12 with every size the frame's own (or no sizes) is not refused for its format: the call is the _full_ call,
    whose own checks answer -- here, in its own name, for a sampling NV12 does not have and for a frame out of order."""
    fr = _frames([(16, 16), (32, 8)], planes=2)
    for sizes in ([(16, 16), (32, 8)], None):
        _refused(call(fr, sj.SRC_NV12, sizes, sj.YUV_444), inner, "yuv_mode does not match the source format")
        bad = _frames([(16, 16), (32, 8)], planes=2)
        bad[1].row_stride[1] = 8
        _refused(call(bad, sj.SRC_NV12, sizes, sj.YUV_420), inner, "frame 1", "row_stride")


@pytest.mark.parametrize("call,who", [(_encode, ENCODE), (_packed, PACKED)])
def test_gray_is_400_only(call, who):
    for fmt in (sj.SRC_GRAY, sj.SRC_GRAY_F32, sj.SRC_GRAY_F16, sj.SRC_GRAY_BF16):
        for mode in (sj.YUV_420, sj.YUV_444):
            _refused(call(_frames([(16, 16)]), fmt, [(5, 7)], mode), who, "yuv_mode")
        for mode in (sj.YUV_AUTO, sj.YUV_SHARP):
            assert call(_frames([(16, 16)]), fmt, [(5, 7)], mode) == EINVAL and who in _err()


def test_resized_bytes_one_short():
    dims, sizes = [(17, 9), (130, 70), (8, 8)], [(3, 2), (129, 1), (8, 8)]
    fr = _frames(dims)
    need = _bytes(sj.SRC_RGB, fr, sizes)
    assert need == _layout(sizes, 3)[0]
    _refused(_resize(fr, sj.SRC_RGB, sizes, resized_bytes=need - 1), RESIZE, "resized_bytes", str(need))
    _refused(_resize(fr, sj.SRC_RGB, sizes, resized_bytes=0), RESIZE, "resized_bytes")
    _refused(_resize(fr, sj.SRC_RGB, sizes, d_resized=(1 << 28) + 4), RESIZE, "multiple of 16")


@pytest.mark.parametrize("call,who", ALL)
def test_the_frame_checks_of_the_ragged_entries(call, who):
    def two():
        return _frames([(16, 16), (16, 16)])
    s = [(5, 7), (16, 3)]
    f = two(); f[1].plane[0] = None
    _refused(call(f, sj.SRC_RGB, s), who, "frame 1", "null plane")
    f = two(); f[1].row_stride[0] = 47
    _refused(call(f, sj.SRC_RGB, s), who, "frame 1", "row_stride")
    f = two(); f[1].row_stride[0] = -47
    _refused(call(f, sj.SRC_RGB, s), who, "frame 1", "row_stride")
    f = two(); f[0].width = 0
    _refused(call(f, sj.SRC_RGB, s), who, "frame 0", "dimensions")
    f = two(); f[1].row_stride[0] = 1025
    _refused(call(f, sj.SRC_RGB_F16, s), who, "frame 1", "row_stride[0]", "element size")
    f = two(); f[1].out_offset, f[1].out_capacity = 2 ** 64 - 1, 2
    _refused(call(f, sj.SRC_RGB, s), who, "frame 1", "out_offset + out_capacity")
    # planar RGB: one pitch
    f = _frames([(16, 16), (16, 16)], planes=3); f[1].row_stride[2] = 1 << 18
    _refused(call(f, sj.SRC_RGB_PLANAR, s), who, "frame 1", "row_stride[2]")


def test_null_arguments():
    L = sj.lib()
    fr = _frames([(16, 16)])
    keep, sz = _sizes([(5, 7)])
    out = (sj.RaggedFrame * 1)()
    rfmt = C.c_int(0)
    p = _params(sj.YUV_420)
    assert L.sjpeg_hip_resize_ragged_src(None, 0, 1, fr, sz, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_resize_ragged_src(FAKE, 0, 1, None, sz, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_resize_ragged_src(FAKE, 0, 1, fr, None, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_resize_ragged_src(FAKE, 0, 1, fr, sz, None, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_resize_ragged_src(FAKE, 0, 1, fr, sz, 1 << 28, 1 << 20, None, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_resize_ragged_src(FAKE, 0, 1, fr, sz, 1 << 28, 1 << 20, out, None, None) == EINVAL
    assert RESIZE in _err() and "NULL" in _err()
    assert L.sjpeg_hip_resize_ragged_src(FAKE, 0, 0, fr, sz, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_resize_ragged_src(FAKE, 99, 1, fr, sz, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    for args in ((None, 0, 1, fr, C.byref(p), sz, None, 0, 1 << 16, 1 << 12), (FAKE, 0, 1, fr, None, sz, None, 0, 1 << 16, 1 << 12),
                 (FAKE, 0, 1, None, C.byref(p), sz, None, 0, 1 << 16, 1 << 12), (FAKE, 0, 1, fr, C.byref(p), sz, None, 0, None, 1 << 12),
                 (FAKE, 0, 1, fr, C.byref(p), sz, None, 0, 1 << 16, None), (FAKE, 0, 0, fr, C.byref(p), sz, None, 0, 1 << 16, 1 << 12)):
        assert L.sjpeg_hip_encode_ragged_resized_src(*args, None, None, None, None) == EINVAL
        assert ENCODE in _err()
    for args in ((None, 0, 1, fr, C.byref(p), sz, None, 0, 1 << 16, 1 << 20, 1 << 12, 1 << 13),
                 (FAKE, 0, 1, fr, None, sz, None, 0, 1 << 16, 1 << 20, 1 << 12, 1 << 13),
                 (FAKE, 0, 1, None, C.byref(p), sz, None, 0, 1 << 16, 1 << 20, 1 << 12, 1 << 13),
                 (FAKE, 0, 1, fr, C.byref(p), sz, None, 0, None, 1 << 20, 1 << 12, 1 << 13),
                 (FAKE, 0, 1, fr, C.byref(p), sz, None, 0, 1 << 16, 1 << 20, None, 1 << 13),
                 (FAKE, 0, 1, fr, C.byref(p), sz, None, 0, 1 << 16, 1 << 20, 1 << 12, None)):
        assert L.sjpeg_hip_encode_ragged_resized_packed_src(*args, None, None, None, None) == EINVAL
        assert PACKED in _err() and "NULL" in _err()
    # the inner call's parameter checks come before any device work too
    bad = _params(sj.YUV_420, method=9)
    assert L.sjpeg_hip_encode_ragged_resized_src(FAKE, 0, 1, fr, C.byref(bad), sz, None, 0, 1 << 16, 1 << 12, None, None, None, None) == EINVAL
    assert "method" in _err()
    assert L.sjpeg_hip_encode_ragged_resized_packed_src(FAKE, 0, 1, fr, C.byref(p), sz, None, 0, (1 << 16) + 8, 1 << 20, 1 << 12, 1 << 13,
                                                        None, None, None, None) == EINVAL
    assert "multiple of 16" in _err()


# ---- exports

def test_symbols_are_exported_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    declared = set(re.findall(r"\b(sjpeg_hip_[a-z_0-9]+)\s*\(", text.split("namespace sjpeg")[0]))
    for name in NEW:
        assert name in sj.EXPORTED_C_SYMBOLS and name in declared, name
        assert getattr(sj.lib(), name).argtypes is not None, name
    assert declared == set(n for n in sj.EXPORTED_C_SYMBOLS if n.startswith("sjpeg_hip_"))
    assert re.search(r"#define\s+SJPEG_HIP_ABI_VERSION\s+18\b", text) and sj.lib().sjpeg_hip_abi_version() == 18
    # no new source format
    assert "SJPEG_HIP_SRC_GRAY_BF16 = 20\n};" in text


# ---- Resized

def test_resized_wrapper():
    ims = [np.zeros((8, 8, 3), np.uint8), np.zeros((4, 6, 3), np.uint8), np.zeros((3, 3, 3), np.uint8)]
    r = sj.Resized(ims, (2, 3))
    assert r.sizes == [(2, 3)] * 3 and r.images == ims
    assert sj.Resized(ims, [(8, 8), (5, 1), (3, 2)]).sizes == [(8, 8), (5, 1), (3, 2)]
    assert sj.Resized(ims, np.array([[1, 2], [3, 4], [3, 1]])).sizes == [(1, 2), (3, 4), (3, 1)]
    assert sj.Resized(tuple(ims), [np.int64(3), 2]).sizes == [(3, 2)] * 3
    assert sj.Resized(ims[:2], [(1, 2), (3, 4)]).sizes == [(1, 2), (3, 4)]
    with pytest.raises(sj.SjpegError, match="sizes for 3 pictures"):
        sj.Resized(ims, [(2, 2), (2, 2)])
    with pytest.raises(sj.SjpegError, match="sizes for 3 pictures"):
        sj.Resized(ims, 4)
    for bad in ((0, 2), (2, 65536), (2.0, 2), (1, 2, 3), 5):
        with pytest.raises(sj.SjpegError, match="picture 1"):
            sj.Resized(ims, [(1, 1), bad, (1, 1)])
    # a wrapped FloatPixels keeps its transform
    fp = sj.FloatPixels(ims, 127.5, 127.5)
    r = sj.Resized(fp, (2, 2))
    assert r.images is fp and r.sizes == [(2, 2)] * 3
    assert sj._resized(r) == (fp, [(2, 2)] * 3) and sj._resized(ims) == (ims, None)
    # one wrapper a picture
    for outer, inner in ((sj.Resized, sj.Reduced(ims, 2)), (sj.Resized, sj.Resized(ims, (1, 1)))):
        with pytest.raises(sj.SjpegError, match="already"):
            outer(inner, (1, 1))
    with pytest.raises(sj.SjpegError, match="Resized already"):
        sj.Reduced(sj.Resized(ims, (1, 1)), 2)
    with pytest.raises(sj.SjpegError, match="already"):
        sj.Resized.fit(sj.Reduced(ims, 2), (2, 2))


def test_resized_fit():
    hwc = [np.zeros((30, 40, 3), np.uint8), np.zeros((4, 6, 3), np.uint8), np.zeros((100, 10, 3), np.uint8)]
    assert sj.Resized.fit(hwc, (16, 16)).sizes == [(16, 12), (6, 4), (2, 16)]
    chw = [np.zeros((3, 30, 40), np.uint8), np.zeros((3, 4, 6), np.uint8)]
    assert sj.Resized.fit(chw, (16, 16), layout="chw").sizes == [(16, 12), (6, 4)]
    fp = sj.FloatPixels([np.zeros((3, 30, 40), np.float32), np.zeros((30, 40), np.float32)])
    assert sj.Resized.fit(fp, (16, 16)).sizes == [(16, 12), (16, 12)]
    with pytest.raises(sj.SjpegError, match="bad box"):
        sj.Resized.fit(hwc, (0, 16))
    with pytest.raises(sj.SjpegError, match="pair"):
        sj.Resized.fit(hwc, 16)
    with pytest.raises(sj.SjpegError, match="layout"):
        sj.Resized.fit(hwc, (16, 16), layout="nhwc")


def test_resized_goes_through_the_calls_own_checks():
    """A Resized is unwrapped first: the calls answer for its pictures as they answer for plain ones."""
    hwc = [np.zeros((8, 8, 3), np.uint8)]
    for call in (lambda r: sj.encode_images(r), lambda r: sj.compress_images(r), lambda r: sj.encode_images_full(r),
                 lambda r: sj.encode_images_full_meta(r, None), lambda r: sj.resize_images(hwc, (2, 2))):
        with pytest.raises(sj.SjpegError, match="image 0"):
            call(sj.Resized(hwc, (2, 2)))
    with pytest.raises(sj.SjpegError, match="image 0 is not a CUDA tensor"):
        sj.encode_images_full_chw(sj.Resized([np.zeros((3, 8, 8), np.uint8)], (2, 2)))
    with pytest.raises(sj.SjpegError, match="layout='chw'"):
        sj.encode_images(sj.Resized(sj.FloatPixels(hwc), (2, 2)))
    with pytest.raises(sj.SjpegError, match="layout"):
        sj.resize_images(hwc, (2, 2), layout="nhwc")
    with pytest.raises(sj.SjpegError, match="picture 0"):
        sj.resize_images(hwc, (0, 2))


def test_riskiness_images_refuses_resized():
    ims = [np.zeros((8, 8, 3), np.uint8)]
    for layout in ("hwc", "chw"):
        with pytest.raises(sj.SjpegError, match="resize first"):
            sj.riskiness_images(sj.Resized(ims, (2, 2)), layout=layout)
    with pytest.raises(sj.SjpegError, match="resize_images"):
        sj.riskiness_images(sj.Resized(ims, (8, 8)))


def test_signatures():
    assert list(inspect.signature(sj.Resized).parameters) == ["images", "sizes"]
    assert list(inspect.signature(sj.Resized.fit).parameters)[:2] == ["images", "box"]
    assert list(inspect.signature(sj.fit_size).parameters) == ["w", "h", "box"]
    assert list(inspect.signature(sj.resize_images).parameters) == ["images", "sizes", "engine", "layout"]
    assert inspect.signature(sj.resize_images).parameters["layout"].default == "hwc"
    for name in ("resize_ragged", "encode_ragged_resized", "encode_ragged_resized_packed"):
        assert list(inspect.signature(getattr(sj.Engine, name)).parameters)[:5] == ["self", "fmt", "planes_per_frame", "dims", "sizes"]
    assert sj._reduced(sj.Reduced([np.zeros((8, 8, 3), np.uint8)], 1))[1] is None          # (still a 2-tuple)
