"""Contact sheets (sjpeg_hip_sheet_size, sjpeg_hip_sheet_places, sjpeg_hip_sheet_ragged_src,
sjpeg_hip_encode_ragged_sheet_src) without a GPU: the formulae of the sheet's size and of every thumbnail's place
against the model in tests/sheet_model.py -- the spare sample on the right and at the bottom, the even rounding for the
4:2:0 formats, the fit with the orientations 5..8 --, the layout of the sheets' buffer, every argument check before any
device work with the frame or the field named, the exports, and the ABI version, which stays 18."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sheet_model as sm
import sjpeg_amd as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = C.c_void_p(1 << 20)          # (the checks come before the engine is touched: any non-NULL value stands in for one)
NEW = ("sjpeg_hip_sheet_size", "sjpeg_hip_sheet_places", "sjpeg_hip_sheet_ragged_bytes", "sjpeg_hip_sheet_ragged_src",
       "sjpeg_hip_encode_ragged_sheet_src", "sjpeg_hip_encode_ragged_sheet_packed_src")
MAKE, ENCODE, PACKED = NEW[3], NEW[4], NEW[5]
KINDS = {"rgb": (sj.SRC_RGB, 1), "gray": (sj.SRC_GRAY, 1), "yuv444": (sj.SRC_YUV444, 3), "yuv420": (sj.SRC_YUV420, 3),
         "nv12": (sj.SRC_NV12, 2), "nv21": (sj.SRC_NV21, 2)}
BG = (0x11, 0x7E, 0xEF)


def _err():
    return sj.lib().sjpeg_hip_last_error().decode()


def _refused(rc, who, *words):
    assert rc == EINVAL
    msg = _err()
    assert who in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def _frames(dims, planes=3):
    f = (sj.RaggedFrame * len(dims))()
    for k, (w, h) in enumerate(dims):
        f[k].width, f[k].height = w, h
        for i in range(planes):
            f[k].plane[i] = (1 << 30) + (i << 24)
            f[k].row_stride[i] = 1 << 19
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


def _params(mode, method=4):
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, method, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    p._keep = q
    return p


def _mode(fmt):
    return {sj.SRC_RGB: sj.YUV_444, sj.SRC_GRAY: sj.YUV_400, sj.SRC_YUV444: sj.YUV_444}.get(fmt, sj.YUV_420)


# ---- the formulae

GRIDS = [(3, 2, (14, 14), 1, 0), (4, 2, (14, 14), 1, 3), (1, 1, (1, 1), 0, 0), (2, 3, (16, 10), 2, 4), (5, 1, (6, 8), 0, 2),
         (2, 2, (160, 90), 6, 10)]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_sheet_size_and_places_are_the_models(kind):
    fmt, _ = KINDS[kind]
    dims = [(37, 23), (23, 37), (640, 6), (5, 3), (1, 1), (16, 16), (20001, 3), (13, 14), (14, 13), (1920, 1080), (7, 9)]
    for cols, rows, cell, gutter, margin in GRIDS:
        if kind in sm.YUV420_LIKE and (cell[0] % 2 or cell[1] % 2 or gutter % 2 or margin % 2):
            cell, gutter, margin = (cell[0] + cell[0] % 2, cell[1] + cell[1] % 2), gutter + gutter % 2, margin + margin % 2
        sheet = sj.Sheet(cols, rows, cell, gutter, margin, BG)
        assert sj.sheet_size(sheet, fmt) == sm.sheet_size(cols, rows, cell, gutter, margin)
        for orientations in ([1] * len(dims), [1 + (3 * k) % 8 for k in range(len(dims))], [6] * len(dims)):
            sizes = sm.fitted_sizes(dims, cell, orientations)
            want = sm.places(kind, cols, rows, cell, gutter, margin, sizes, orientations)
            # sizes NULL: the fit, the box turned with the frame; the same sizes given: the same places
            assert sj.sheet_places(sheet, dims, fmt, None, orientations) == want, (cell, orientations)
            assert sj.sheet_places(sheet, dims, fmt, sizes, orientations) == want
        assert sj.sheet_places(sheet, dims, fmt) == sm.places(kind, cols, rows, cell, gutter, margin,
                                                              sm.fitted_sizes(dims, cell, [1] * len(dims)), [1] * len(dims))


def test_the_spare_sample_is_on_the_right_and_at_the_bottom():
    sheet = sj.Sheet(2, 1, (14, 14), 1, 3, BG)
    # 13 x 9 in a 14 x 14 cell: one spare column, five spare rows -> offsets 0 and 2; the second cell starts at 3 + 15
    assert sj.sheet_places(sheet, [(37, 23)] * 2, sj.SRC_RGB, [(13, 9)] * 2) == [(0, 3, 5, 13, 9), (0, 18, 5, 13, 9)]
    assert sj.sheet_places(sheet, [(37, 23)], sj.SRC_RGB, [(13, 9)], [6]) == [(0, 3 + 2, 3, 9, 13)]
    assert sj.sheet_places(sheet, [(37, 23)] * 3, sj.SRC_RGB, [(1, 1)] * 3)[2] == (1, 3 + 6, 3 + 6, 1, 1)      # a second sheet


def test_the_centring_offset_is_rounded_down_to_even_for_420():
    sheet = sj.Sheet(2, 1, (14, 14), 2, 2, BG)
    for fmt in (sj.SRC_NV12, sj.SRC_NV21, sj.SRC_YUV420):
        # 9 x 5: (14 - 9) / 2 = 2, (14 - 5) / 2 = 4; 7 x 9: 3 -> 2 and 2; 1 x 1: 6 and 6; 11 x 3: 1 -> 0, 5 -> 4
        got = sj.sheet_places(sheet, [(37, 23)] * 4, fmt, [(9, 5), (7, 9), (1, 1), (11, 3)])
        assert got == [(0, 2 + 2, 2 + 4, 9, 5), (0, 18 + 2, 2 + 2, 7, 9), (1, 2 + 6, 2 + 6, 1, 1), (1, 18 + 0, 2 + 4, 11, 3)]
        assert all(x % 2 == 0 and y % 2 == 0 for _, x, y, _, _ in got)
    # 4:4:4 and RGB have no evenness rule
    for fmt in (sj.SRC_YUV444, sj.SRC_RGB):
        assert sj.sheet_places(sheet, [(37, 23)] * 2, fmt, [(7, 9), (11, 3)]) == [(0, 2 + 3, 2 + 2, 7, 9), (0, 18 + 1, 2 + 5, 11, 3)]


def test_the_fit_turns_the_box_with_the_frame():
    sheet = sj.Sheet(1, 1, (160, 90), 0, 0, BG)
    # 1920 x 1080 stored: upright as stored it fills the cell; lying on its side it is fitted into 90 x 160
    assert sj.sheet_places(sheet, [(1920, 1080)], sj.SRC_NV12, None, [1]) == [(0, 0, 0, 160, 90)]
    w, h = sm.fit(1920, 1080, 90, 160)
    assert (w, h) == (90, 51) == sj.fit_size(1920, 1080, (90, 160))
    assert sj.sheet_places(sheet, [(1920, 1080)], sj.SRC_NV12, None, [6]) == [(0, (160 - 51) // 2 & ~1, 0, 51, 90)]
    assert sj.sheet_places(sheet, [(1920, 1080)], sj.SRC_RGB, None, [8]) == [(0, (160 - 51) // 2, 0, 51, 90)]
    # never larger: a picture smaller than its cell stays as it is
    assert sj.sheet_places(sheet, [(31, 17)], sj.SRC_RGB) == [(0, 64, 36, 31, 17)]
    assert sj.sheet_places(sheet, [(31, 17)], sj.SRC_RGB, None, [5]) == [(0, 71, 29, 17, 31)]


# ---- the sheets' buffer

def _bytes(fmt, frames, sheet, sizes, orientations):
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    st = sheet._struct()
    return sj.lib().sjpeg_hip_sheet_ragged_bytes(fmt, len(frames), frames, C.addressof(st), ptr, optr)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_bytes_is_the_layout_of_the_sheets(kind):
    fmt, planes = KINDS[kind]
    for cols, rows, cell, gutter, margin in ((3, 2, (14, 14), 2, 2), (1, 1, (2, 2), 0, 0), (2, 2, (160, 90), 6, 10)):
        sheet = sj.Sheet(cols, rows, cell, gutter, margin, BG)
        SW, SH = sm.sheet_size(cols, rows, cell, gutter, margin)
        half = kind in sm.YUV420_LIKE
        if kind in ("rgb", "gray"):
            per = ((SW * (3 if kind == "rgb" else 1) + 3) & ~3) * SH + 15 & ~15
        else:
            cw, ch = (SW // 2, SH // 2) if half else (SW, SH)
            per = ((((SW + 3) & ~3) * SH + 15) & ~15) + 2 * ((((cw + 3) & ~3) * ch + 15) & ~15)
        for n in (1, cols * rows, cols * rows + 1, 3 * cols * rows):
            nsheets = -(-n // (cols * rows))
            assert _bytes(fmt, _frames([(37, 23)] * n, planes), sheet, None, None) == per * nsheets, (cell, n)


def test_bytes_is_zero_on_bad_arguments():
    sheet = sj.Sheet(2, 1, (14, 14), 2, 2, BG)
    fr = _frames([(37, 23), (16, 16)], 2)
    assert _bytes(sj.SRC_NV12, fr, sheet, None, [1, 9]) == 0 and "frame 1" in _err() and "orientation 9" in _err()
    assert _bytes(sj.SRC_NV12, fr, sheet, [(38, 4), (8, 8)], None) == 0 and "above the source's 37x23" in _err()
    assert _bytes(sj.SRC_NV12, fr, sheet, [(13, 9), (16, 16)], None) == 0 and "frame 1" in _err() and "16x16" in _err() and "14x14" in _err()
    assert _bytes(99, fr, sheet, None, None) == 0 and "unknown source format" in _err()
    st = sheet._struct()
    assert sj.lib().sjpeg_hip_sheet_ragged_bytes(sj.SRC_NV12, 2, None, C.addressof(st), None, None) == 0 and "frames == NULL" in _err()
    assert sj.lib().sjpeg_hip_sheet_ragged_bytes(sj.SRC_NV12, 2, fr, None, None, None) == 0 and "sheet == NULL" in _err()
    assert sj.lib().sjpeg_hip_sheet_ragged_bytes(sj.SRC_NV12, 0, fr, C.addressof(st), None, None) == 0 and "nframes" in _err()


# ---- the sheet's own checks: the field named

def _size_rc(sheet_struct, fmt):
    w, h = C.c_int(-7), C.c_int(-7)
    rc = sj.lib().sjpeg_hip_sheet_size(C.byref(sheet_struct), fmt, C.byref(w), C.byref(h))
    if rc != 0:
        assert (w.value, h.value) == (-7, -7)          # refused: nothing was written
    return rc


def test_sheet_fields_out_of_range_are_named():
    who = "sjpeg_hip_sheet_size"
    good = dict(cols=2, rows=2, cell_width=16, cell_height=10, gutter=2, margin=2)
    for field, lo in (("cols", 1), ("rows", 1), ("cell_width", 1), ("cell_height", 1), ("gutter", 0), ("margin", 0)):
        for bad in (lo - 1, 65536, -5):
            st = sj.Sheet(1, 1, (1, 1))._struct()
            for k, v in good.items():
                setattr(st, k, v)
            setattr(st, field, bad)
            _refused(_size_rc(st, sj.SRC_RGB), who, "%s %d" % (field, bad), "%d..65535" % lo)
    st = sj.Sheet(2, 2, (16, 10), 2, 2)._struct()
    st.reserved = 1
    _refused(_size_rc(st, sj.SRC_RGB), who, "reserved")
    _refused(_size_rc(sj.Sheet(4096, 1, (16, 10))._struct(), sj.SRC_RGB), who, "65536x10", "above 65535")
    _refused(_size_rc(sj.Sheet(1, 3, (16, 21845), 1, 0)._struct(), sj.SRC_RGB), who, "above 65535")
    assert _size_rc(sj.Sheet(1, 3, (16, 21845), 0, 0)._struct(), sj.SRC_RGB) == 0
    _refused(_size_rc(sj.Sheet(2, 2, (16, 10))._struct(), 99), who, "unknown source format")
    w = C.c_int(0)
    assert sj.lib().sjpeg_hip_sheet_size(None, sj.SRC_RGB, C.byref(w), C.byref(w)) == EINVAL and "sheet == NULL" in _err()
    st = sj.Sheet(2, 2, (16, 10))._struct()
    assert sj.lib().sjpeg_hip_sheet_size(C.byref(st), sj.SRC_RGB, None, C.byref(w)) == EINVAL and "NULL" in _err()


def test_odd_values_with_a_420_format_are_named():
    who = "sjpeg_hip_sheet_size"
    for fmt, name in ((sj.SRC_NV12, "SJPEG_HIP_SRC_NV12"), (sj.SRC_NV21, "SJPEG_HIP_SRC_NV21"), (sj.SRC_YUV420, "SJPEG_HIP_SRC_YUV420")):
        _refused(_size_rc(sj.Sheet(2, 2, (15, 10), 2, 2)._struct(), fmt), who, "cell_width 15 is odd", name)
        _refused(_size_rc(sj.Sheet(2, 2, (16, 9), 2, 2)._struct(), fmt), who, "cell_height 9 is odd")
        _refused(_size_rc(sj.Sheet(2, 2, (16, 10), 1, 2)._struct(), fmt), who, "gutter 1 is odd")
        _refused(_size_rc(sj.Sheet(2, 2, (16, 10), 2, 3)._struct(), fmt), who, "margin 3 is odd")
        assert _size_rc(sj.Sheet(3, 3, (16, 10), 2, 2)._struct(), fmt) == 0            # (cols and rows may be odd)
    for fmt in (sj.SRC_YUV444, sj.SRC_RGB, sj.SRC_GRAY, sj.SRC_RGB_PLANAR_F16):
        assert sj.sheet_size(sj.Sheet(2, 2, (15, 9), 1, 3), fmt) == (6 + 30 + 1, 6 + 18 + 1)
    with pytest.raises(sj.SjpegError, match="cell_width 15 is odd"):
        sj.sheet_size(sj.Sheet(2, 2, (15, 10)), sj.SRC_NV12)


# ---- argument checks of the device entries with a stand-in engine: nothing touches it

def _make(frames, fmt, sheet, sizes, orientations, mode=None, out_bytes=1 << 30, d_out=1 << 28):
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    st = sheet._struct()
    out = (sj.RaggedFrame * 64)()
    ns, rfmt = C.c_int(-7), C.c_int(-7)
    rc = sj.lib().sjpeg_hip_sheet_ragged_src(FAKE, fmt, len(frames), frames, C.addressof(st), ptr, optr, d_out, out_bytes, out,
                                             C.byref(ns), C.byref(rfmt), None)
    assert (ns.value, rfmt.value) == (-7, -7)          # refused: nothing was reported
    return rc


def _encode(frames, fmt, sheet, sizes, orientations, mode=None):
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    st = sheet._struct()
    p = _params(mode if mode is not None else _mode(fmt))
    return sj.lib().sjpeg_hip_encode_ragged_sheet_src(FAKE, fmt, len(frames), frames, C.byref(p), C.addressof(st), ptr, optr, None, 0,
                                                      1 << 16, 1 << 20, 1 << 12, None, None, None, None)


def _packed(frames, fmt, sheet, sizes, orientations, mode=None):
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    st = sheet._struct()
    p = _params(mode if mode is not None else _mode(fmt))
    return sj.lib().sjpeg_hip_encode_ragged_sheet_packed_src(FAKE, fmt, len(frames), frames, C.byref(p), C.addressof(st), ptr, optr,
                                                             None, 0, 1 << 16, 1 << 20, 1 << 12, 1 << 13, None, None, None, None)


ALL = [(_make, MAKE), (_encode, ENCODE), (_packed, PACKED)]
SHEET = sj.Sheet(2, 1, (14, 14), 2, 2, BG)


@pytest.mark.parametrize("call,who", ALL)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_plans_checks_name_the_frame(call, who, kind):
    fmt, planes = KINDS[kind]
    fr = _frames([(16, 16), (17, 9), (8, 8)], planes)
    _refused(call(fr, fmt, SHEET, [(8, 8), (9, 17), (4, 4)], [6, 6, 6]), who, "frame 1", "size 9x17", "above the source's 17x9")
    _refused(call(fr, fmt, SHEET, [(0, 8), (13, 9), (8, 8)], None), who, "frame 0", "size 0x8", "below 1")
    for sizes in (None, [(8, 8), (13, 9), (4, 4)]):
        _refused(call(fr, fmt, SHEET, sizes, [1, 0, 6]), who, "frame 1", "orientation 0", "1..8")
        _refused(call(fr, fmt, SHEET, sizes, [6, 8, 9]), who, "frame 2", "orientation 9", "1..8")
    f = _frames([(16, 16), (17, 9)], planes); f[1].plane[0] = None
    _refused(call(f, fmt, SHEET, None, None), who, "frame 1", "null plane")
    f = _frames([(16, 16), (17, 9)], planes); f[0].width = 0
    _refused(call(f, fmt, SHEET, None, None), who, "frame 0", "dimensions")
    _refused(call(fr, 99, SHEET, None, None, sj.YUV_420), who, "unknown source format")


@pytest.mark.parametrize("call,who", ALL)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_thumbnail_larger_than_its_cell_names_frame_sizes_and_orientation(call, who, kind):
    fmt, planes = KINDS[kind]
    fr = _frames([(64, 40), (64, 40), (64, 40)], planes)
    _refused(call(fr, fmt, SHEET, [(14, 14), (15, 9), (4, 4)], None), who, "frame 1", "15x9", "14x14", "orientation 1")
    # 14 x 10 stored is 10 x 14 upright: it fits; 10 x 15 stored is 15 x 10 upright: it does not
    _refused(call(fr, fmt, SHEET, [(14, 10), (14, 10), (10, 15)], [6, 1, 8]), who, "frame 2", "10x15", "15x10", "14x14", "orientation 8")


@pytest.mark.parametrize("call,who", ALL)
def test_the_sheet_checks_come_through_every_entry(call, who):
    fr = _frames([(64, 40)] * 2, 2)
    _refused(call(fr, sj.SRC_NV12, sj.Sheet(2, 1, (15, 14), 2, 2), None, None), who, "cell_width 15 is odd")
    _refused(call(fr, sj.SRC_NV12, sj.Sheet(2, 1, (14, 14), 2, 1), None, None), who, "margin 1 is odd")
    _refused(call(fr, sj.SRC_NV12, sj.Sheet(0, 1, (14, 14), 2, 2), None, None), who, "cols 0")
    _refused(call(fr, sj.SRC_NV12, sj.Sheet(2, 1, (14, 65536), 2, 2), None, None), who, "cell_height 65536")
    _refused(call(fr, sj.SRC_NV12, sj.Sheet(4096, 1, (16, 14), 2, 2), None, None), who, "above 65535")

    class Reserved(sj.Sheet):
        def _struct(self):
            st = sj.Sheet._struct(self)
            st.reserved = 3
            return st
    _refused(call(fr, sj.SRC_NV12, Reserved(2, 1, (14, 14), 2, 2), None, None), who, "reserved")


def test_bytes_one_short_and_alignment():
    for kind, (fmt, planes) in KINDS.items():
        fr = _frames([(37, 23)] * 3, planes)
        need = _bytes(fmt, fr, SHEET, None, None)
        assert need > 0
        _refused(_make(fr, fmt, SHEET, None, None, out_bytes=need - 1), MAKE, "bytes " + str(need - 1), str(need), "sjpeg_hip_sheet_ragged_bytes")
        _refused(_make(fr, fmt, SHEET, None, None, d_out=(1 << 28) + 4), MAKE, "multiple of 16")


def test_yuv_mode_must_be_the_formats_own():
    for call, who in ALL[1:]:
        fr = _frames([(37, 23)] * 3, 2)
        _refused(call(fr, sj.SRC_NV12, SHEET, None, None, sj.YUV_444), who, "yuv_mode does not match the source format")
        assert "gray" not in _err()
        _refused(call(_frames([(37, 23)], 1), sj.SRC_GRAY, SHEET, None, None, sj.YUV_420), who, "yuv_mode does not match", "gray pictures are coded 4:0:0 only")
        _refused(call(_frames([(37, 23)], 1), sj.SRC_GRAY_F16, SHEET, None, None, sj.YUV_AUTO), who, "yuv_mode does not match")
        _refused(call(fr, sj.SRC_NV12, SHEET, None, None, sj.YUV_AUTO), who, "yuv_mode does not match")


def test_null_arguments_and_out_stride():
    L = sj.lib()
    fr = _frames([(37, 23)], 1)
    st = SHEET._struct()
    sp = C.addressof(st)
    out = (sj.RaggedFrame * 1)()
    ns, rfmt = C.c_int(0), C.c_int(0)
    p = _params(sj.YUV_444)
    rgb = sj.SRC_RGB
    for args in ((None, rgb, 1, fr, sp, None, None, 1 << 28, 1 << 20, out, C.byref(ns), C.byref(rfmt)),
                 (FAKE, rgb, 1, None, sp, None, None, 1 << 28, 1 << 20, out, C.byref(ns), C.byref(rfmt)),
                 (FAKE, rgb, 1, fr, None, None, None, 1 << 28, 1 << 20, out, C.byref(ns), C.byref(rfmt)),
                 (FAKE, rgb, 1, fr, sp, None, None, None, 1 << 20, out, C.byref(ns), C.byref(rfmt)),
                 (FAKE, rgb, 1, fr, sp, None, None, 1 << 28, 1 << 20, None, C.byref(ns), C.byref(rfmt)),
                 (FAKE, rgb, 1, fr, sp, None, None, 1 << 28, 1 << 20, out, None, C.byref(rfmt)),
                 (FAKE, rgb, 1, fr, sp, None, None, 1 << 28, 1 << 20, out, C.byref(ns), None)):
        assert L.sjpeg_hip_sheet_ragged_src(*args, None) == EINVAL
        assert MAKE in _err() and "NULL" in _err()
    assert L.sjpeg_hip_sheet_ragged_src(FAKE, rgb, 0, fr, sp, None, None, 1 << 28, 1 << 20, out, C.byref(ns), C.byref(rfmt), None) == EINVAL
    assert "nframes" in _err()
    good = (FAKE, rgb, 1, fr, C.byref(p), sp, None, None, None, 0, 1 << 16, 1 << 20, 1 << 12)
    for k in (0, 3, 4, 5, 10, 12):
        args = list(good)
        args[k] = None
        assert L.sjpeg_hip_encode_ragged_sheet_src(*args, None, None, None, None) == EINVAL
        assert ENCODE in _err() and "NULL" in _err(), (k, _err())
    for stride in (0,):
        args = list(good)
        args[11] = stride
        assert L.sjpeg_hip_encode_ragged_sheet_src(*args, None, None, None, None) == EINVAL
        assert ENCODE in _err() and "out_stride" in _err()
    args = list(good); args[2] = 0
    assert L.sjpeg_hip_encode_ragged_sheet_src(*args, None, None, None, None) == EINVAL and "nframes" in _err()
    goodp = (FAKE, rgb, 1, fr, C.byref(p), sp, None, None, None, 0, 1 << 16, 1 << 20, 1 << 12, 1 << 13)
    for k in (0, 3, 4, 5, 10, 12, 13):
        args = list(goodp)
        args[k] = None
        assert L.sjpeg_hip_encode_ragged_sheet_packed_src(*args, None, None, None, None) == EINVAL
        assert PACKED in _err() and "NULL" in _err(), (k, _err())
    args = list(goodp); args[10] = (1 << 16) + 8
    assert L.sjpeg_hip_encode_ragged_sheet_packed_src(*args, None, None, None, None) == EINVAL and "multiple of 16" in _err()
    # the inner call's parameter checks come before any device work too, and count SHEETS
    bad = _params(sj.YUV_444, method=9)
    args = list(good); args[4] = C.byref(bad)
    assert L.sjpeg_hip_encode_ragged_sheet_src(*args, None, None, None, None) == EINVAL and "method" in _err()
    search = (sj.SearchParams * 2)(sj.SearchParams(1, 4000.0, 10, 1.0, 0.0, 100.0), sj.SearchParams(7, 1.0, 10, 1.0, 0.0, 100.0))
    q = np.ones((2, 2, 64), np.uint8)
    per_sheet = sj.RaggedParams(sj.YUV_444, 4, q.ctypes.data, 1, None, 0x78, 12, 1, search, 1)
    three = _frames([(37, 23)] * 3, 1)                       # 2 cells a sheet: two sheets, search[1] is the second sheet's
    args = list(good); args[2], args[3], args[4] = 3, three, C.byref(per_sheet)
    assert L.sjpeg_hip_encode_ragged_sheet_src(*args, None, None, None, None) == EINVAL and "search[1]" in _err() and "target_mode" in _err()


# ---- the Python layer

def test_python_layer_refusals():
    with pytest.raises(sj.SjpegError, match="background"):
        sj.Sheet(2, 2, (16, 10), background=(0, 256, 0))
    with pytest.raises(sj.SjpegError, match="cell"):
        sj.Sheet(2, 2, 16)
    with pytest.raises(sj.SjpegError, match="not a Sheet"):
        sj.sheet_size((2, 2, (16, 10)))
    with pytest.raises(sj.SjpegError, match="frame 0"):
        sj.sheet_places(sj.Sheet(1, 1, (4, 4)), [(8, 8)], sj.SRC_RGB, [(5, 4)])
    s = sj.Sheet(3, 2, (14, 12), gutter=1, margin=2, background=BG)
    assert (s.cols, s.rows, s.cell, s.gutter, s.margin, s.background) == (3, 2, (14, 12), 1, 2, BG)
    st = s._struct()
    assert C.sizeof(st) == 28 and bytes(st.background) == bytes(BG) and st.reserved == 0


def test_symbols_are_exported_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    declared = set(re.findall(r"\b(sjpeg_hip_[a-z_0-9]+)\s*\(", text.split("namespace sjpeg")[0]))
    for name in NEW:
        assert name in sj.EXPORTED_C_SYMBOLS and name in declared, name
        assert getattr(sj.lib(), name).argtypes is not None, name
    assert declared == set(n for n in sj.EXPORTED_C_SYMBOLS if n.startswith("sjpeg_hip_"))
    for name in ("Sheet", "sheet_size", "sheet_places", "make_sheets", "encode_sheets", "encode_yuv_sheets"):
        assert hasattr(sj, name), name
    for name in ("sheet_ragged", "encode_ragged_sheet", "encode_ragged_sheet_packed"):
        assert hasattr(sj.Engine, name), name
    assert sj.lib().sjpeg_hip_abi_version() == 18          # (entries were added, none changed)
    assert "#define SJPEG_HIP_ABI_VERSION 18" in text
