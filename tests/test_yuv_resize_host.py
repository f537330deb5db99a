"""Decoded video resized and turned inside the ragged call (sjpeg_hip_resize_ragged_yuv_src,
sjpeg_hip_encode_ragged_yuv_resized_src, encode_yuv_frames) without a GPU: the size of a plane, the layout of the made
planes, every argument check before any device work (the frame named), the pass-through, the exports -- and the
refusals of the entries of before, which still make one interleaved plane and take no YUV-plane format."""
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
NEW = ("sjpeg_hip_yuv_plane_size", "sjpeg_hip_resize_ragged_yuv_bytes", "sjpeg_hip_resize_ragged_yuv_src",
       "sjpeg_hip_encode_ragged_yuv_resized_src", "sjpeg_hip_encode_ragged_yuv_resized_packed_src")
RESIZE = "sjpeg_hip_resize_ragged_yuv_src"
ENCODE = "sjpeg_hip_encode_ragged_yuv_resized_src"
PACKED = "sjpeg_hip_encode_ragged_yuv_resized_packed_src"
FORMATS = [(sj.SRC_YUV444, "SJPEG_HIP_SRC_YUV444", 3), (sj.SRC_YUV420, "SJPEG_HIP_SRC_YUV420", 3),
           (sj.SRC_NV12, "SJPEG_HIP_SRC_NV12", 2), (sj.SRC_NV21, "SJPEG_HIP_SRC_NV21", 2)]


def _err():
    return sj.lib().sjpeg_hip_last_error().decode()


def _refused(rc, who, *words):
    assert rc == EINVAL
    msg = _err()
    assert who in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def _mode(fmt):
    return sj.YUV_444 if fmt == sj.SRC_YUV444 else sj.YUV_420


# ---- the size of a plane

def _plane(fmt, w, h, plane):
    """the issue's definition, restated"""
    if plane == 0 or fmt == sj.SRC_YUV444:
        return w, h
    return (w + 1) // 2, (h + 1) // 2


def test_yuv_plane_size():
    for fmt, _, _ in FORMATS:
        for (w, h) in ((1, 1), (2, 1), (1, 2), (2, 2), (3, 3), (16, 16), (37, 23), (640, 6), (20001, 3), (65535, 65535), (65534, 1)):
            for plane in range(3):
                assert sj.yuv_plane_size(fmt, w, h, plane) == _plane(fmt, w, h, plane), (fmt, w, h, plane)
    assert sj.yuv_plane_size(sj.SRC_NV12, 37, 23, 1) == (19, 12) and sj.yuv_plane_size(sj.SRC_YUV444, 37, 23, 2) == (37, 23)


def test_yuv_plane_size_refusals():
    L = sj.lib()
    pw, ph = C.c_int(7), C.c_int(7)
    who = "sjpeg_hip_yuv_plane_size"
    for fmt, name in ((sj.SRC_RGB, "SJPEG_HIP_SRC_RGB"), (sj.SRC_GRAY, "SJPEG_HIP_SRC_GRAY"), (sj.SRC_RGB_PLANAR, "SJPEG_HIP_SRC_RGB_PLANAR"),
                      (sj.SRC_RGBA_F16, "SJPEG_HIP_SRC_RGBA_F16")):
        _refused(L.sjpeg_hip_yuv_plane_size(fmt, 8, 8, 0, C.byref(pw), C.byref(ph)), who, name)
    _refused(L.sjpeg_hip_yuv_plane_size(99, 8, 8, 0, C.byref(pw), C.byref(ph)), who, "unknown source format")
    for (w, h) in ((0, 4), (4, 0), (65536, 4), (4, 65536), (-1, 4)):
        _refused(L.sjpeg_hip_yuv_plane_size(sj.SRC_NV12, w, h, 0, C.byref(pw), C.byref(ph)), who, "dimensions")
    for plane in (-1, 3):
        _refused(L.sjpeg_hip_yuv_plane_size(sj.SRC_NV12, 8, 8, plane, C.byref(pw), C.byref(ph)), who, "plane")
    _refused(L.sjpeg_hip_yuv_plane_size(sj.SRC_NV12, 8, 8, 0, None, C.byref(ph)), who, "NULL")
    _refused(L.sjpeg_hip_yuv_plane_size(sj.SRC_NV12, 8, 8, 0, C.byref(pw), None), who, "NULL")
    assert (pw.value, ph.value) == (7, 7)          # nothing was written
    with pytest.raises(sj.SjpegError, match="SJPEG_HIP_SRC_BGRA"):
        sj.yuv_plane_size(sj.SRC_BGRA, 8, 8, 0)


# ---- the made planes' buffer

def _frames(dims, planes=3):
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


def _orients(orientations):
    if orientations is None:
        return None, None
    arr = np.ascontiguousarray(np.asarray(orientations, np.uint8))
    return arr, arr.ctypes.data


def _bytes(fmt, frames, sizes, orientations):
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    return sj.lib().sjpeg_hip_resize_ragged_yuv_bytes(fmt, len(frames), frames, ptr, optr)


def _layout(fmt, sizes, orientations):
    """The documented layout, restated: for frame after frame Y, U, V; every UPRIGHT plane at a multiple of 16, its rows
    align4(plane width) apart."""
    at = 0
    for (w2, h2), o in zip(sizes, orientations):
        for plane in range(3):
            pw, ph = _plane(fmt, w2, h2, plane)
            uw, uh = (ph, pw) if o >= 5 else (pw, ph)
            at += (((uw + 3) & ~3) * uh + 15) & ~15
    return at


@pytest.mark.parametrize("fmt,name,planes", FORMATS)
def test_bytes_is_the_layout_of_the_upright_planes(fmt, name, planes):
    dims = [(8, 9), (17, 9), (1, 1), (5, 3), (64, 5), (130, 70), (300, 40), (1030, 9), (37, 23)]
    sizes = [(1, 2), (3, 9), (1, 1), (5, 3), (63, 1), (129, 1), (7, 3), (1029, 8), (13, 9)]
    fr = _frames(dims, planes)
    for o in range(1, 9):
        assert _bytes(fmt, fr, sizes, [o] * len(dims)) == _layout(fmt, sizes, [o] * len(dims)), o
    mixed = [1 + (k * 3) % 8 for k in range(len(dims))]
    assert _bytes(fmt, fr, sizes, mixed) == _layout(fmt, sizes, mixed)
    # sizes NULL: every frame at its own size; orientations NULL: all 1
    assert _bytes(fmt, fr, None, mixed) == _layout(fmt, dims, mixed)
    assert _bytes(fmt, fr, sizes, None) == _layout(fmt, sizes, [1] * len(dims)) == _bytes(fmt, fr, sizes, [1] * len(dims))
    assert _bytes(fmt, fr, None, None) == _layout(fmt, dims, [1] * len(dims))
    # 13 x 9 turned: luma rows of 12 bytes instead of 16; 4:2:0 chroma 7 x 5 turned is 5 wide: rows of 8 either way
    one = _bytes(fmt, _frames([(37, 23)], planes), [(13, 9)], [6])
    assert one == 160 + 2 * (160 if fmt == sj.SRC_YUV444 else 64), one          # (12 * 13 -> 160; 8 * 7 -> 64)


def test_bytes_is_zero_on_bad_arguments():
    fr = _frames([(16, 16), (8, 8)], 2)
    assert _bytes(sj.SRC_NV12, fr, None, [1, 0]) == 0 and "frame 1" in _err() and "orientation 0" in _err()
    assert _bytes(sj.SRC_NV12, fr, None, [9, 1]) == 0 and "frame 0" in _err() and "orientation 9" in _err()
    assert _bytes(sj.SRC_NV12, fr, [(17, 4), (8, 8)], [6, 6]) == 0 and "above the source's 16x16" in _err()
    assert _bytes(sj.SRC_NV12, fr, [(16, 16), (8, 0)], None) == 0 and "frame 1" in _err() and "below 1" in _err()
    assert _bytes(sj.SRC_RGB, _frames([(16, 16)], 1), None, [6]) == 0 and "SJPEG_HIP_SRC_RGB" in _err()
    assert _bytes(sj.SRC_GRAY, _frames([(16, 16)], 1), None, None) == 0 and "SJPEG_HIP_SRC_GRAY" in _err()
    assert _bytes(99, fr, None, None) == 0 and "unknown source format" in _err()
    assert sj.lib().sjpeg_hip_resize_ragged_yuv_bytes(sj.SRC_NV12, 1, None, None, None) == 0 and "NULL" in _err()
    assert sj.lib().sjpeg_hip_resize_ragged_yuv_bytes(sj.SRC_NV12, 0, fr, None, None) == 0 and "nframes" in _err()


# ---- argument checks with a stand-in engine: nothing touches it

def _params(mode, method=4):
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, method, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    p._keep = q
    return p


def _resize(frames, fmt, sizes, orientations, mode=None, out_bytes=1 << 30, d_out=1 << 28):
    n = len(frames)
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    out = (sj.RaggedFrame * n)()
    rfmt = C.c_int(-7)
    rc = sj.lib().sjpeg_hip_resize_ragged_yuv_src(FAKE, fmt, n, frames, ptr, optr, d_out, out_bytes, out, C.byref(rfmt), None)
    assert rfmt.value == -7                       # refused: nothing was reported
    return rc


def _encode(frames, fmt, sizes, orientations, mode=None):
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    p = _params(mode if mode is not None else _mode(fmt))
    return sj.lib().sjpeg_hip_encode_ragged_yuv_resized_src(FAKE, fmt, len(frames), frames, C.byref(p), ptr, optr, None, 0, 1 << 16,
                                                            1 << 12, None, None, None, None)


def _packed(frames, fmt, sizes, orientations, mode=None):
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    p = _params(mode if mode is not None else _mode(fmt))
    return sj.lib().sjpeg_hip_encode_ragged_yuv_resized_packed_src(FAKE, fmt, len(frames), frames, C.byref(p), ptr, optr, None, 0,
                                                                   1 << 16, 1 << 20, 1 << 12, 1 << 13, None, None, None, None)


ALL = [(_resize, RESIZE), (_encode, ENCODE), (_packed, PACKED)]


@pytest.mark.parametrize("call,who", ALL)
def test_an_rgb_like_or_gray_format_is_refused_by_name(call, who):
    for fmt, name, planes in ((sj.SRC_RGB, "SJPEG_HIP_SRC_RGB", 1), (sj.SRC_BGRA, "SJPEG_HIP_SRC_BGRA", 1),
                              (sj.SRC_GRAY, "SJPEG_HIP_SRC_GRAY", 1), (sj.SRC_RGB_PLANAR, "SJPEG_HIP_SRC_RGB_PLANAR", 3),
                              (sj.SRC_RGB_F32, "SJPEG_HIP_SRC_RGB_F32", 1), (sj.SRC_GRAY_BF16, "SJPEG_HIP_SRC_GRAY_BF16", 1)):
        fr = _frames([(16, 16), (32, 8)], planes)
        for sizes, orientations in ((None, None), ([(8, 8), (32, 8)], [6, 1]), ([(16, 16), (32, 8)], [1, 1])):
            _refused(call(fr, fmt, sizes, orientations, sj.YUV_420), who, name + " is not a YUV-plane format", "sjpeg_hip_orient_ragged_src")
    _refused(call(_frames([(16, 16)], 1), 99, None, None, sj.YUV_420), who, "unknown source format")


@pytest.mark.parametrize("call,who", ALL)
@pytest.mark.parametrize("fmt,name,planes", FORMATS)
def test_a_size_outside_the_source_names_the_frame(call, who, fmt, name, planes):
    """sizes are in the STORED orientation: 9 x 17 is above a 17 x 9 source whatever the orientation"""
    fr = _frames([(16, 16), (17, 9), (8, 8)], planes)
    _refused(call(fr, fmt, [(8, 8), (9, 17), (4, 4)], [6, 6, 6]), who, "frame 1", "size 9x17", "above the source's 17x9")
    _refused(call(fr, fmt, [(8, 8), (17, 9), (8, 9)], None), who, "frame 2", "size 8x9", "above the source's 8x8")
    _refused(call(fr, fmt, [(0, 8), (17, 9), (8, 8)], [5, 8, 3]), who, "frame 0", "size 0x8", "below 1")
    _refused(call(fr, fmt, [(8, 8), (17, -1), (8, 8)], None), who, "frame 1", "size 17x-1", "below 1")


@pytest.mark.parametrize("call,who", ALL)
@pytest.mark.parametrize("fmt,name,planes", FORMATS)
def test_an_orientation_outside_1_to_8_names_the_frame(call, who, fmt, name, planes):
    fr = _frames([(16, 16), (17, 9), (8, 8)], planes)
    for sizes in (None, [(8, 8), (17, 9), (4, 4)]):
        _refused(call(fr, fmt, sizes, [1, 0, 6]), who, "frame 1", "orientation 0", "1..8")
        _refused(call(fr, fmt, sizes, [6, 8, 9]), who, "frame 2", "orientation 9", "1..8")
        _refused(call(fr, fmt, sizes, [255, 1, 1]), who, "frame 0", "orientation 255")


def test_bytes_one_short_and_alignment():
    dims, sizes, orientations = [(17, 9), (130, 70), (8, 8)], [(3, 2), (129, 1), (8, 8)], [6, 5, 2]
    for fmt, name, planes in FORMATS:
        fr = _frames(dims, planes)
        need = _bytes(fmt, fr, sizes, orientations)
        assert need == _layout(fmt, sizes, orientations) > 0
        _refused(_resize(fr, fmt, sizes, orientations, out_bytes=need - 1), RESIZE, "bytes " + str(need - 1), str(need),
                 "sjpeg_hip_resize_ragged_yuv_bytes")
        _refused(_resize(fr, fmt, sizes, orientations, d_out=(1 << 28) + 4), RESIZE, "multiple of 16")


@pytest.mark.parametrize("call,who", ALL)
def test_the_frame_checks_of_the_ragged_entries(call, who):
    def two():
        return _frames([(16, 16), (16, 16)], 2)
    s, o = [(5, 7), (16, 3)], [6, 3]
    f = two(); f[1].plane[0] = None
    _refused(call(f, sj.SRC_NV12, s, o), who, "frame 1", "null plane")
    f = two(); f[1].plane[1] = None
    _refused(call(f, sj.SRC_NV12, s, o), who, "frame 1", "null plane")
    f = two(); f[1].row_stride[1] = 15                      # (a row of the UV plane of a 16-wide picture is 16 bytes)
    _refused(call(f, sj.SRC_NV12, s, o), who, "frame 1", "row_stride")
    f = two(); f[0].width = 0
    _refused(call(f, sj.SRC_NV12, s, o), who, "frame 0", "dimensions")
    f = _frames([(16, 16), (16, 16)], 3); f[0].plane[2] = None
    _refused(call(f, sj.SRC_YUV420, s, o), who, "frame 0", "null plane")


def test_null_arguments():
    L = sj.lib()
    fr = _frames([(16, 16)], 2)
    keep, sz = _sizes([(5, 7)])
    okeep, op = _orients([6])
    out = (sj.RaggedFrame * 1)()
    rfmt = C.c_int(0)
    p = _params(sj.YUV_420)
    nv = sj.SRC_NV12
    assert L.sjpeg_hip_resize_ragged_yuv_src(None, nv, 1, fr, sz, op, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_resize_ragged_yuv_src(FAKE, nv, 1, None, sz, op, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_resize_ragged_yuv_src(FAKE, nv, 1, fr, sz, op, None, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_resize_ragged_yuv_src(FAKE, nv, 1, fr, sz, op, 1 << 28, 1 << 20, None, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_resize_ragged_yuv_src(FAKE, nv, 1, fr, sz, op, 1 << 28, 1 << 20, out, None, None) == EINVAL
    assert RESIZE in _err() and "NULL" in _err()
    assert L.sjpeg_hip_resize_ragged_yuv_src(FAKE, nv, 0, fr, sz, op, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert "nframes" in _err()
    for args in ((None, nv, 1, fr, C.byref(p), sz, op, None, 0, 1 << 16, 1 << 12), (FAKE, nv, 1, fr, None, sz, op, None, 0, 1 << 16, 1 << 12),
                 (FAKE, nv, 1, None, C.byref(p), sz, op, None, 0, 1 << 16, 1 << 12), (FAKE, nv, 1, fr, C.byref(p), sz, op, None, 0, None, 1 << 12),
                 (FAKE, nv, 1, fr, C.byref(p), sz, op, None, 0, 1 << 16, None), (FAKE, nv, 0, fr, C.byref(p), sz, op, None, 0, 1 << 16, 1 << 12)):
        assert L.sjpeg_hip_encode_ragged_yuv_resized_src(*args, None, None, None, None) == EINVAL
        assert ENCODE in _err()
    for args in ((None, nv, 1, fr, C.byref(p), sz, op, None, 0, 1 << 16, 1 << 20, 1 << 12, 1 << 13),
                 (FAKE, nv, 1, fr, C.byref(p), sz, op, None, 0, None, 1 << 20, 1 << 12, 1 << 13),
                 (FAKE, nv, 1, fr, C.byref(p), sz, op, None, 0, 1 << 16, 1 << 20, None, 1 << 13),
                 (FAKE, nv, 1, fr, C.byref(p), sz, op, None, 0, 1 << 16, 1 << 20, 1 << 12, None)):
        assert L.sjpeg_hip_encode_ragged_yuv_resized_packed_src(*args, None, None, None, None) == EINVAL
        assert PACKED in _err() and "NULL" in _err()
    assert L.sjpeg_hip_encode_ragged_yuv_resized_packed_src(FAKE, nv, 1, fr, C.byref(p), sz, op, None, 0, (1 << 16) + 8, 1 << 20, 1 << 12,
                                                            1 << 13, None, None, None, None) == EINVAL
    assert "multiple of 16" in _err()
    # the inner call's parameter checks come before any device work too
    bad = _params(sj.YUV_420, method=9)
    assert L.sjpeg_hip_encode_ragged_yuv_resized_src(FAKE, nv, 1, fr, C.byref(bad), sz, op, None, 0, 1 << 16, 1 << 12, None, None, None, None) == EINVAL
    assert "method" in _err()


@pytest.mark.parametrize("call,who,inner", [(_encode, ENCODE, "sjpeg_hip_encode_ragged_full_src"),
                                            (_packed, PACKED, "sjpeg_hip_encode_ragged_full_packed_src")])
def test_the_pass_through_reaches_the_inner_call(call, who, inner):
    """own sizes and all-1 orientations (or both NULL): the _full_meta_ call on the caller's frames, whose own checks
    answer in its own name; with a size or a turn the yuv entry answers, in the same words"""
    for fmt, name, planes in FORMATS:
        wrong = sj.YUV_420 if fmt == sj.SRC_YUV444 else sj.YUV_444
        fr = _frames([(16, 16), (32, 8)], planes)
        for orientations in (None, [1, 1]):
            for sizes in ([(16, 16), (32, 8)], None):
                _refused(call(fr, fmt, sizes, orientations, wrong), inner, "yuv_mode does not match the source format")
        for sizes, orientations in (([(16, 16), (16, 8)], None), (None, [1, 6])):
            _refused(call(fr, fmt, sizes, orientations, wrong), who, "yuv_mode does not match the source format")
            _refused(call(fr, fmt, sizes, orientations, sj.YUV_400), who, "yuv_mode does not match the source format")
            assert "gray" not in _err()


def test_the_entries_of_before_still_refuse_nv12_by_name():
    """they make ONE interleaved plane: a careless generalisation of the plan would show here"""
    L = sj.lib()
    fr = _frames([(16, 16), (32, 8)], 2)
    keep, sz = _sizes([(16, 16), (16, 8)])
    okeep, op = _orients([1, 6])
    fkeep = np.asarray([1, 2], np.uint8)
    out = (sj.RaggedFrame * 2)()
    rfmt = C.c_int(-7)
    p = _params(sj.YUV_420)
    nv, name = sj.SRC_NV12, "SJPEG_HIP_SRC_NV12"
    _refused(L.sjpeg_hip_resize_ragged_src(FAKE, nv, 2, fr, sz, 1 << 28, 1 << 30, out, C.byref(rfmt), None),
             "sjpeg_hip_resize_ragged_src", name, "not resized")
    _refused(L.sjpeg_hip_orient_ragged_src(FAKE, nv, 2, fr, sz, op, 1 << 28, 1 << 30, out, C.byref(rfmt), None),
             "sjpeg_hip_orient_ragged_src", name, "not oriented")
    assert rfmt.value == -7
    assert L.sjpeg_hip_resize_ragged_bytes(nv, 2, fr, sz) == 0 and name in _err() and "not resized" in _err()
    assert L.sjpeg_hip_orient_ragged_bytes(nv, 2, fr, sz, op) == 0 and name in _err() and "not oriented" in _err()
    _refused(L.sjpeg_hip_encode_ragged_resized_src(FAKE, nv, 2, fr, C.byref(p), sz, None, 0, 1 << 16, 1 << 12, None, None, None, None),
             "sjpeg_hip_encode_ragged_resized_src", name, "not resized")
    _refused(L.sjpeg_hip_encode_ragged_oriented_src(FAKE, nv, 2, fr, C.byref(p), sz, op, None, 0, 1 << 16, 1 << 12, None, None, None, None),
             "sjpeg_hip_encode_ragged_oriented_src", name, "not oriented")
    assert L.sjpeg_hip_encode_ragged_reduced_src(FAKE, nv, 2, fr, C.byref(p), fkeep.ctypes.data, None, 0, 1 << 16, 1 << 12, None, None,
                                                 None, None) == EINVAL
    assert "sjpeg_hip_encode_ragged_reduced_src" in _err() and name in _err()
    _refused(L.sjpeg_hip_encode_ragged_resized_packed_src(FAKE, nv, 2, fr, C.byref(p), sz, None, 0, 1 << 16, 1 << 20, 1 << 12, 1 << 13,
                                                          None, None, None, None),
             "sjpeg_hip_encode_ragged_resized_packed_src", name, "not resized")
    _refused(L.sjpeg_hip_encode_ragged_oriented_packed_src(FAKE, nv, 2, fr, C.byref(p), sz, op, None, 0, 1 << 16, 1 << 20, 1 << 12,
                                                           1 << 13, None, None, None, None),
             "sjpeg_hip_encode_ragged_oriented_packed_src", name, "not oriented")


# ---- exports and signatures

def test_symbols_are_exported_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    declared = set(re.findall(r"\b(sjpeg_hip_[a-z_0-9]+)\s*\(", text.split("namespace sjpeg")[0]))
    for name in NEW:
        assert name in sj.EXPORTED_C_SYMBOLS and name in declared, name
        assert getattr(sj.lib(), name).argtypes is not None, name
    assert declared == set(n for n in sj.EXPORTED_C_SYMBOLS if n.startswith("sjpeg_hip_"))
    assert sj.lib().sjpeg_hip_abi_version() == 18          # (entries were added, none changed)


def test_signatures():
    assert list(inspect.signature(sj.yuv_plane_size).parameters) == ["fmt", "w", "h", "plane"]
    assert list(inspect.signature(sj.Engine.resize_ragged_yuv).parameters) == ["self", "fmt", "planes_per_frame", "dims", "sizes",
                                                                                "orientations", "out"]
    for new, old in (("encode_ragged_yuv_resized", "encode_ragged_oriented"), ("encode_ragged_yuv_resized_packed", "encode_ragged_oriented_packed")):
        assert inspect.signature(getattr(sj.Engine, new)) == inspect.signature(getattr(sj.Engine, old)), new
    sig = inspect.signature(sj.encode_yuv_frames)
    assert list(sig.parameters) == ["frames", "fmt", "sizes", "box", "orientations", "quality", "method", "target_size", "target_psnr",
                                    "packed", "metadata", "engine"]
    assert sig.parameters["fmt"].default == sj.SRC_NV12 and sig.parameters["quality"].default == 75.0
    assert sig.parameters["method"].default == 4 and sig.parameters["packed"].default is False


def test_the_plan_file_has_no_hip_in_it():
    text = open(os.path.join(ROOT, "sjpeg_amd", "csrc", "yuv_resize_plan.cc")).read()
    assert "__global__" not in text and "__device__" not in text and "hipLaunch" not in text
