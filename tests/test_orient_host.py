"""Pictures turned upright inside the ragged call (sjpeg_hip_orient_ragged_src, sjpeg_hip_encode_ragged_oriented_src,
Oriented) without a GPU: the upright size, the EXIF Orientation read and reset against tests/golden/exif_orientation.json,
the layout of the oriented buffer, every argument check before any device work (the frame named), the exports, and the
Oriented wrapper."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import sjpeg_amd as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = C.c_void_p(1 << 20)          # (the checks come before the engine is touched: any non-NULL value stands in for one)
NEW = ("sjpeg_hip_oriented_size", "sjpeg_hip_orient_ragged_bytes", "sjpeg_hip_orient_ragged_src",
       "sjpeg_hip_encode_ragged_oriented_src", "sjpeg_hip_encode_ragged_oriented_packed_src",
       "sjpeg_hip_exif_orientation", "sjpeg_hip_exif_reset_orientation")
ORIENT = "sjpeg_hip_orient_ragged_src"
ENCODE = "sjpeg_hip_encode_ragged_oriented_src"
PACKED = "sjpeg_hip_encode_ragged_oriented_packed_src"


def _err():
    return sj.lib().sjpeg_hip_last_error().decode()


def _refused(rc, who, *words):
    assert rc == EINVAL
    msg = _err()
    assert who in msg, msg
    for w in words:
        assert w in msg, (w, msg)


# ---- the upright size

def test_oriented_size():
    for o in (1, 2, 3, 4):
        assert sj.oriented_size(3, 2, o) == (3, 2) and sj.oriented_size(65535, 1, o) == (65535, 1)
    for o in (5, 6, 7, 8):
        assert sj.oriented_size(3, 2, o) == (2, 3) and sj.oriented_size(65535, 1, o) == (1, 65535)
    L = sj.lib()
    ow, oh = C.c_int(7), C.c_int(7)
    for o in (0, 9, -1, 256 + 6):
        _refused(L.sjpeg_hip_oriented_size(3, 2, o, C.byref(ow), C.byref(oh)), "sjpeg_hip_oriented_size", "orientation", "1..8")
    for (w, h) in ((0, 4), (4, 0), (65536, 4), (4, 65536)):
        _refused(L.sjpeg_hip_oriented_size(w, h, 6, C.byref(ow), C.byref(oh)), "sjpeg_hip_oriented_size", "dimensions")
    _refused(L.sjpeg_hip_oriented_size(3, 2, 6, None, C.byref(oh)), "sjpeg_hip_oriented_size", "NULL")
    assert (ow.value, oh.value) == (7, 7)          # nothing was written
    with pytest.raises(sj.SjpegError, match="orientation 9"):
        sj.oriented_size(3, 2, 9)


# ---- the EXIF tag

@pytest.fixture(scope="module")
def exif_cases():
    with open(os.path.join(ROOT, "tests", "golden", "exif_orientation.json")) as f:
        return json.load(f)["cases"]


def test_exif_fixture_covers_what_it_should(exif_cases):
    names = [c["name"] for c in exif_cases]
    for o in range(1, 9):
        assert "pillow big-endian %d" % o in names and "little-endian %d" % o in names
    for word in ("behind Make", "no Orientation", "type LONG", "next IFD past the end"):
        assert any(word in n for n in names), word
    assert {c["orientation"] for c in exif_cases} == set(range(9))


def test_exif_orientation_and_reset(exif_cases):
    for c in exif_cases:
        b = bytes.fromhex(c["hex"])
        assert sj.exif_orientation(b) == c["orientation"], c["name"]
        after = sj.exif_reset_orientation(b)
        assert after.hex() == c["reset_hex"], c["name"]
        assert sj.exif_orientation(after) == (1 if c["orientation"] else 0), c["name"]
        # in place, through the C entry: the old value comes back, and 0 changes nothing
        buf = (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0")
        assert sj.lib().sjpeg_hip_exif_reset_orientation(buf, len(b)) == c["orientation"], c["name"]
        assert bytes(buf)[:len(b)].hex() == c["reset_hex"], c["name"]
    assert sj.lib().sjpeg_hip_exif_orientation(None, 0) == 0 and sj.lib().sjpeg_hip_exif_orientation(None, 40) == 0
    assert sj.lib().sjpeg_hip_exif_reset_orientation(None, 40) == 0


# ---- the oriented buffer

def _frames(dims, planes=1):
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
    return sj.lib().sjpeg_hip_orient_ragged_bytes(fmt, len(frames), frames, ptr, optr)


def _layout(sizes, orientations, channels):
    """The documented layout, restated: the UPRIGHT picture's rows a multiple of 4 apart, pictures at multiples of 16"""
    at = 0
    for (w2, h2), o in zip(sizes, orientations):
        uw, uh = (h2, w2) if o >= 5 else (w2, h2)
        at += (((uw * channels + 3) & ~3) * uh + 15) & ~15
    return at


@pytest.mark.parametrize("fmt,channels,planes", [(sj.SRC_RGB, 3, 1), (sj.SRC_BGRA, 3, 1), (sj.SRC_RGB_PLANAR, 3, 3),
                                                 (sj.SRC_GRAY, 1, 1), (sj.SRC_GRAY_F16, 1, 1), (sj.SRC_RGBA_BF16, 3, 1)])
def test_orient_ragged_bytes_is_the_upright_layout(fmt, channels, planes):
    dims = [(8, 9), (17, 9), (1, 1), (5, 3), (64, 5), (130, 70), (300, 40), (1030, 9)]
    sizes = [(1, 2), (3, 9), (1, 1), (5, 3), (63, 1), (129, 1), (7, 3), (1029, 8)]
    fr = _frames(dims, planes)
    for o in range(1, 9):
        assert _bytes(fmt, fr, sizes, [o] * len(dims)) == _layout(sizes, [o] * len(dims), channels), o
    mixed = [1 + (k * 3) % 8 for k in range(len(dims))]
    assert _bytes(fmt, fr, sizes, mixed) == _layout(sizes, mixed, channels)
    # 5 x 3 turned is 3 wide: rows of 12 bytes instead of 16 (RGB), 4 instead of 8 (gray)
    assert _bytes(fmt, _frames([(5, 3)], planes), None, [6]) == (((3 * channels + 3) & ~3) * 5 + 15) & ~15
    # sizes NULL: every frame at its own size; orientations NULL: the resize's value
    assert _bytes(fmt, fr, None, mixed) == _layout(dims, mixed, channels)
    keep, ptr = _sizes(sizes)
    plain = sj.lib().sjpeg_hip_resize_ragged_bytes(fmt, len(dims), fr, ptr)
    assert plain > 0 and _bytes(fmt, fr, sizes, None) == plain == _bytes(fmt, fr, sizes, [1] * len(dims))
    assert _bytes(fmt, fr, None, None) == sj.lib().sjpeg_hip_resize_ragged_bytes(fmt, len(dims), fr, None)


def test_orient_ragged_bytes_is_zero_on_bad_arguments():
    fr = _frames([(16, 16), (8, 8)])
    assert _bytes(sj.SRC_RGB, fr, None, [1, 0]) == 0 and "frame 1" in _err() and "orientation 0" in _err()
    assert _bytes(sj.SRC_RGB, fr, None, [9, 1]) == 0 and "frame 0" in _err() and "orientation 9" in _err()
    assert _bytes(sj.SRC_RGB, fr, [(17, 4), (8, 8)], [6, 6]) == 0 and "above the source's 16x16" in _err()
    assert _bytes(sj.SRC_NV12, _frames([(16, 16)], planes=2), None, [6]) == 0 and "SJPEG_HIP_SRC_NV12" in _err()
    assert sj.lib().sjpeg_hip_orient_ragged_bytes(sj.SRC_RGB, 1, None, None, None) == 0


# ---- argument checks with a stand-in engine: nothing touches it

def _params(mode, method=4):
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, method, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    p._keep = q
    return p


def _orient(frames, fmt, sizes, orientations, mode=None, out_bytes=1 << 30, d_out=1 << 28):
    n = len(frames)
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    out = (sj.RaggedFrame * n)()
    rfmt = C.c_int(-7)
    rc = sj.lib().sjpeg_hip_orient_ragged_src(FAKE, fmt, n, frames, ptr, optr, d_out, out_bytes, out, C.byref(rfmt), None)
    assert rfmt.value == -7                       # refused: nothing was reported
    return rc


def _encode(frames, fmt, sizes, orientations, mode=sj.YUV_420):
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    p = _params(mode if mode is not None else sj.YUV_420)
    return sj.lib().sjpeg_hip_encode_ragged_oriented_src(FAKE, fmt, len(frames), frames, C.byref(p), ptr, optr, None, 0, 1 << 16,
                                                         1 << 12, None, None, None, None)


def _packed(frames, fmt, sizes, orientations, mode=sj.YUV_420):
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    p = _params(mode if mode is not None else sj.YUV_420)
    return sj.lib().sjpeg_hip_encode_ragged_oriented_packed_src(FAKE, fmt, len(frames), frames, C.byref(p), ptr, optr, None, 0,
                                                                1 << 16, 1 << 20, 1 << 12, 1 << 13, None, None, None, None)


ALL = [(_orient, ORIENT), (_encode, ENCODE), (_packed, PACKED)]


@pytest.mark.parametrize("call,who", ALL)
def test_an_orientation_outside_1_to_8_names_the_frame(call, who):
    fr = _frames([(16, 16), (17, 9), (8, 8)])
    for sizes in (None, [(8, 8), (17, 9), (4, 4)]):
        _refused(call(fr, sj.SRC_RGB, sizes, [1, 0, 6]), who, "frame 1", "orientation 0", "1..8")
        _refused(call(fr, sj.SRC_RGB, sizes, [6, 8, 9]), who, "frame 2", "orientation 9", "1..8")
        _refused(call(fr, sj.SRC_RGBA_F16, sizes, [255, 1, 1]), who, "frame 0", "orientation 255")


@pytest.mark.parametrize("call,who", ALL)
def test_yuv_plane_formats_are_not_oriented(call, who):
    for fmt, name, planes in ((sj.SRC_NV12, "SJPEG_HIP_SRC_NV12", 2), (sj.SRC_NV21, "SJPEG_HIP_SRC_NV21", 2),
                              (sj.SRC_YUV420, "SJPEG_HIP_SRC_YUV420", 3), (sj.SRC_YUV444, "SJPEG_HIP_SRC_YUV444", 3)):
        mode = sj.YUV_444 if fmt == sj.SRC_YUV444 else sj.YUV_420
        fr = _frames([(16, 16), (32, 8)], planes=planes)
        for sizes in (None, [(16, 16), (32, 8)]):
            _refused(call(fr, fmt, sizes, [1, 6], mode), who, name, "not oriented")
            _refused(call(fr, fmt, sizes, [3, 1], mode), who, name, "not oriented")


@pytest.mark.parametrize("call,who", ALL)
def test_a_size_above_the_source_names_the_frame(call, who):
    """sizes are in the STORED orientation: 9 x 17 is above a 17 x 9 source whatever the orientation"""
    fr = _frames([(16, 16), (17, 9), (8, 8)])
    _refused(call(fr, sj.SRC_RGB, [(8, 8), (9, 17), (4, 4)], [6, 6, 6]), who, "frame 1", "size 9x17", "above the source's 17x9")
    _refused(call(fr, sj.SRC_RGB, [(8, 8), (17, 9), (8, 9)], [1, 8, 3]), who, "frame 2", "size 8x9", "above the source's 8x8")
    _refused(call(fr, sj.SRC_RGB, [(0, 8), (17, 9), (8, 8)], [5, 8, 3]), who, "frame 0", "size 0x8", "below 1")


@pytest.mark.parametrize("call,inner", [(_encode, "sjpeg_hip_encode_ragged_full_src"), (_packed, "sjpeg_hip_encode_ragged_full_packed_src")])
def test_all_ones_is_the_resized_call(call, inner):
    """orientations NULL or all 1: the resized call on the same arguments -- NV12 at its own sizes goes on to the _full_
    call, whose own checks answer in its own name; with a size of its own the resized call refuses the format in ITS name"""
    fr = _frames([(16, 16), (32, 8)], planes=2)
    for orientations in (None, [1, 1]):
        for sizes in ([(16, 16), (32, 8)], None):
            _refused(call(fr, sj.SRC_NV12, sizes, orientations, sj.YUV_444), inner, "yuv_mode does not match the source format")
        resized = "sjpeg_hip_encode_ragged_resized_packed_src" if call is _packed else "sjpeg_hip_encode_ragged_resized_src"
        _refused(call(fr, sj.SRC_NV12, [(16, 16), (16, 8)], orientations, sj.YUV_420), resized, "SJPEG_HIP_SRC_NV12", "not resized")


@pytest.mark.parametrize("call,who", [(_encode, ENCODE), (_packed, PACKED)])
def test_gray_is_400_only(call, who):
    for fmt in (sj.SRC_GRAY, sj.SRC_GRAY_F16):
        for mode in (sj.YUV_420, sj.YUV_444):
            _refused(call(_frames([(16, 16)]), fmt, None, [6], mode), who, "yuv_mode")


def test_bytes_one_short_and_alignment():
    dims, sizes, orientations = [(17, 9), (130, 70), (8, 8)], [(3, 2), (129, 1), (8, 8)], [6, 5, 2]
    fr = _frames(dims)
    need = _bytes(sj.SRC_RGB, fr, sizes, orientations)
    assert need == _layout(sizes, orientations, 3)
    _refused(_orient(fr, sj.SRC_RGB, sizes, orientations, out_bytes=need - 1), ORIENT, "bytes", str(need))
    _refused(_orient(fr, sj.SRC_RGB, sizes, orientations, d_out=(1 << 28) + 4), ORIENT, "multiple of 16")


@pytest.mark.parametrize("call,who", ALL)
def test_the_frame_checks_of_the_ragged_entries(call, who):
    def two():
        return _frames([(16, 16), (16, 16)])
    s, o = [(5, 7), (16, 3)], [6, 3]
    f = two(); f[1].plane[0] = None
    _refused(call(f, sj.SRC_RGB, s, o), who, "frame 1", "null plane")
    f = two(); f[1].row_stride[0] = 47
    _refused(call(f, sj.SRC_RGB, s, o), who, "frame 1", "row_stride")
    f = two(); f[0].width = 0
    _refused(call(f, sj.SRC_RGB, s, o), who, "frame 0", "dimensions")


def test_null_arguments():
    L = sj.lib()
    fr = _frames([(16, 16)])
    keep, sz = _sizes([(5, 7)])
    okeep, op = _orients([6])
    out = (sj.RaggedFrame * 1)()
    rfmt = C.c_int(0)
    p = _params(sj.YUV_420)
    assert L.sjpeg_hip_orient_ragged_src(None, 0, 1, fr, sz, op, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_orient_ragged_src(FAKE, 0, 1, None, sz, op, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_orient_ragged_src(FAKE, 0, 1, fr, sz, op, None, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_orient_ragged_src(FAKE, 0, 1, fr, sz, op, 1 << 28, 1 << 20, None, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_orient_ragged_src(FAKE, 0, 1, fr, sz, op, 1 << 28, 1 << 20, out, None, None) == EINVAL
    assert ORIENT in _err() and "NULL" in _err()
    assert L.sjpeg_hip_orient_ragged_src(FAKE, 0, 0, fr, sz, op, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    assert L.sjpeg_hip_orient_ragged_src(FAKE, 99, 1, fr, sz, op, 1 << 28, 1 << 20, out, C.byref(rfmt), None) == EINVAL
    for args in ((None, 0, 1, fr, C.byref(p), sz, op, None, 0, 1 << 16, 1 << 12), (FAKE, 0, 1, fr, None, sz, op, None, 0, 1 << 16, 1 << 12),
                 (FAKE, 0, 1, None, C.byref(p), sz, op, None, 0, 1 << 16, 1 << 12), (FAKE, 0, 1, fr, C.byref(p), sz, op, None, 0, None, 1 << 12),
                 (FAKE, 0, 1, fr, C.byref(p), sz, op, None, 0, 1 << 16, None), (FAKE, 0, 0, fr, C.byref(p), sz, op, None, 0, 1 << 16, 1 << 12)):
        assert L.sjpeg_hip_encode_ragged_oriented_src(*args, None, None, None, None) == EINVAL
        assert ENCODE in _err()
    for args in ((None, 0, 1, fr, C.byref(p), sz, op, None, 0, 1 << 16, 1 << 20, 1 << 12, 1 << 13),
                 (FAKE, 0, 1, fr, C.byref(p), sz, op, None, 0, None, 1 << 20, 1 << 12, 1 << 13),
                 (FAKE, 0, 1, fr, C.byref(p), sz, op, None, 0, 1 << 16, 1 << 20, None, 1 << 13),
                 (FAKE, 0, 1, fr, C.byref(p), sz, op, None, 0, 1 << 16, 1 << 20, 1 << 12, None)):
        assert L.sjpeg_hip_encode_ragged_oriented_packed_src(*args, None, None, None, None) == EINVAL
        assert PACKED in _err() and "NULL" in _err()
    # the inner call's parameter checks come before any device work too
    bad = _params(sj.YUV_420, method=9)
    assert L.sjpeg_hip_encode_ragged_oriented_src(FAKE, 0, 1, fr, C.byref(bad), sz, op, None, 0, 1 << 16, 1 << 12, None, None, None, None) == EINVAL
    assert "method" in _err()


# ---- exports

def test_symbols_are_exported_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    declared = set(re.findall(r"\b(sjpeg_hip_[a-z_0-9]+)\s*\(", text.split("namespace sjpeg")[0]))
    for name in NEW:
        assert name in sj.EXPORTED_C_SYMBOLS and name in declared, name
        assert getattr(sj.lib(), name).argtypes is not None, name
    assert declared == set(n for n in sj.EXPORTED_C_SYMBOLS if n.startswith("sjpeg_hip_"))
    assert re.search(r"#define\s+SJPEG_HIP_ABI_VERSION\s+18\b", text) and sj.lib().sjpeg_hip_abi_version() == 18


def test_the_exif_file_has_no_hip_in_it():
    text = open(os.path.join(ROOT, "sjpeg_amd", "csrc", "exif_orientation.cc")).read()
    assert "hip_runtime" not in text and "__global__" not in text and "__device__" not in text


# ---- Oriented

def test_oriented_wrapper():
    ims = [np.zeros((8, 8, 3), np.uint8), np.zeros((4, 6, 3), np.uint8), np.zeros((3, 3, 3), np.uint8)]
    r = sj.Oriented(ims, 6)
    assert r.orientations == [6] * 3 and r.sizes is None and r.images == ims
    r = sj.Oriented(ims, [1, 8, np.int64(3)], (2, 3))
    assert r.orientations == [1, 8, 3] and r.sizes == [(2, 3)] * 3
    assert sj.Oriented(tuple(ims), np.array([5, 6, 7]), [(8, 8), (5, 1), (3, 2)]).sizes == [(8, 8), (5, 1), (3, 2)]
    with pytest.raises(sj.SjpegError, match="2 orientations for 3 pictures"):
        sj.Oriented(ims, [6, 6])
    for bad in (0, 9, 6.0, "6", None):
        with pytest.raises(sj.SjpegError, match="picture 1"):
            sj.Oriented(ims, [1, bad, 1])
    with pytest.raises(sj.SjpegError, match="picture 1"):
        sj.Oriented(ims, 6, [(1, 1), (0, 2), (1, 1)])
    # what the calls unwrap: nothing turned is the Resized (or the pictures themselves)
    assert sj._oriented(ims) == (ims, None)
    assert sj._oriented(sj.Oriented(ims, 1)) == (ims, None)
    inner, turned = sj._oriented(sj.Oriented(ims, [1, 6, 1], (2, 2)))
    assert isinstance(inner, sj.Resized) and inner.sizes == [(2, 2)] * 3 and turned == [1, 6, 1]
    inner, turned = sj._oriented(sj.Oriented(ims, 1, (2, 2)))
    assert isinstance(inner, sj.Resized) and turned is None
    fp = sj.FloatPixels(ims, 127.5, 127.5)
    assert sj._oriented(sj.Oriented(fp, 3)) == (fp, [3] * 3)
    # one wrapper a picture
    for inner in (sj.Reduced(ims, 2), sj.Resized(ims, (1, 1)), sj.Oriented(ims, 6)):
        with pytest.raises(sj.SjpegError, match="already"):
            sj.Oriented(inner, 6)
    for outer in (lambda x: sj.Reduced(x, 2), lambda x: sj.Resized(x, (1, 1)), lambda x: sj.Resized.fit(x, (2, 2))):
        with pytest.raises(sj.SjpegError, match="Oriented already"):
            outer(sj.Oriented(ims, 6))


def test_oriented_fit_takes_the_upright_box():
    hwc = [np.zeros((30, 40, 3), np.uint8), np.zeros((4, 6, 3), np.uint8), np.zeros((100, 10, 3), np.uint8)]
    # a 32 x 16 box: as stored, 40 x 30 fits as 21 x 16; turned, the stored picture is fitted into 16 x 32
    f = sj.Oriented.fit(hwc, [1, 3, 2], (32, 16))
    assert f.sizes == [sj.fit_size(40, 30, (32, 16)), (6, 4), sj.fit_size(10, 100, (32, 16))] and f.sizes[0] == (21, 16)
    f = sj.Oriented.fit(hwc, [6, 8, 5], (32, 16))
    assert f.sizes == [sj.fit_size(40, 30, (16, 32)), (6, 4), sj.fit_size(10, 100, (16, 32))] and f.sizes[0] == (16, 12)
    for (w, h), o in zip(f.sizes, f.orientations):
        uw, uh = sj.oriented_size(w, h, o)
        assert uw <= 32 and uh <= 16
    chw = [np.zeros((3, 30, 40), np.uint8)]
    assert sj.Oriented.fit(chw, 7, (32, 16), layout="chw").sizes == [(16, 12)]
    with pytest.raises(sj.SjpegError, match="pair"):
        sj.Oriented.fit(hwc, 6, 16)
    with pytest.raises(sj.SjpegError, match="layout"):
        sj.Oriented.fit(hwc, 6, (16, 16), layout="nhwc")


def test_oriented_from_metadata(exif_cases):
    by_name = {c["name"]: bytes.fromhex(c["hex"]) for c in exif_cases}
    ims = [np.zeros((30, 40, 3), np.uint8)] * 5
    metas = [sj.PictureMetadata(exif=by_name["pillow big-endian 6"], xmp=b"<x:xmpmeta>kept</x:xmpmeta>"), None,
             sj.PictureMetadata(exif=by_name["little-endian 8"], iccp=b"profile"),
             sj.PictureMetadata(exif=by_name["little-endian, type LONG"]), sj.PictureMetadata()]
    made, out = sj.Oriented.from_metadata(ims, metas)
    assert made.orientations == [6, 1, 8, 1, 1] and made.sizes is None
    assert out[1] is None and out[0] is not metas[0]
    assert [sj.exif_orientation(m.exif) for m in (out[0], out[2])] == [1, 1]
    assert sj.exif_orientation(metas[0].exif) == 6                       # (the caller's objects are not written to)
    assert out[0].xmp == metas[0].xmp and out[2].iccp == b"profile" and out[3].exif == metas[3].exif and out[4].exif == b""
    made, out = sj.Oriented.from_metadata(ims, metas, box=(16, 16))
    assert made.sizes == [(16, 12), (16, 12), (16, 12), (16, 12), (16, 12)]
    made, out = sj.Oriented.from_metadata(ims, metas, box=(32, 16))
    assert made.sizes == [(16, 12), (21, 16), (16, 12), (21, 16), (21, 16)]
    one, out = sj.Oriented.from_metadata(ims, metas[0])
    assert one.orientations == [6] * 5 and len(out) == 5
    with pytest.raises(sj.SjpegError, match="one metadata entry per image"):
        sj.Oriented.from_metadata(ims, metas[:2])


def test_oriented_goes_through_the_calls_own_checks():
    hwc = [np.zeros((8, 8, 3), np.uint8)]
    for call in (lambda r: sj.encode_images(r), lambda r: sj.compress_images(r), lambda r: sj.encode_images_full(r),
                 lambda r: sj.encode_images_full_meta(r, None), lambda r: sj.orient_images(hwc, 6, (2, 2))):
        with pytest.raises(sj.SjpegError, match="image 0"):
            call(sj.Oriented(hwc, 6, (2, 2)))
    with pytest.raises(sj.SjpegError, match="layout"):
        sj.orient_images(hwc, 6, layout="nhwc")
    with pytest.raises(sj.SjpegError, match="picture 0"):
        sj.orient_images(hwc, 0)
    with pytest.raises(sj.SjpegError, match="turn them first"):
        sj.riskiness_images(sj.Oriented(hwc, 6))


def test_signatures():
    assert list(inspect.signature(sj.Oriented).parameters) == ["images", "orientations", "sizes"]
    assert inspect.signature(sj.Oriented).parameters["sizes"].default is None
    assert list(inspect.signature(sj.Oriented.fit).parameters) == ["images", "orientations", "box", "layout"]
    assert list(inspect.signature(sj.Oriented.from_metadata).parameters) == ["images", "metadata", "box", "layout"]
    assert list(inspect.signature(sj.orient_images).parameters) == ["images", "orientations", "sizes", "engine", "layout"]
    for name in ("orient_ragged", "encode_ragged_oriented", "encode_ragged_oriented_packed"):
        assert list(inspect.signature(getattr(sj.Engine, name)).parameters)[:6] == ["self", "fmt", "planes_per_frame", "dims", "sizes",
                                                                                     "orientations"]
    # the wrappers of before are what they were
    assert list(inspect.signature(sj.Resized).parameters) == ["images", "sizes"]
    assert sj._resized(sj.Resized([np.zeros((8, 8, 3), np.uint8)], (1, 1)))[1] == [(1, 1)]
