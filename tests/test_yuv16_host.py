"""10-bit video in the ragged call (sjpeg_hip_convert_ragged_yuv16_src and the other _yuv16 entries, sjpeg_amd.video)
without a GPU: the own-size formula over all 65536 words for every shift against the model, every refusal before any
device work with its message -- the depth's fields, the alignment of planes and strides, short rows, the formats that
are not YUV planes by name, NULLs --, the exports against the declarations, and VideoDepth."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import sjpeg_amd as sj
import sjpeg_amd.video as sv
import yuv16_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = C.c_void_p(1 << 20)          # (the checks come before the engine is touched: any non-NULL value stands in for one)
SAMPLES = "sjpeg_hip_yuv16_samples"
CONVERT = "sjpeg_hip_convert_ragged_yuv16_src"
ENCODE = "sjpeg_hip_encode_ragged_yuv16_src"
PACKED = "sjpeg_hip_encode_ragged_yuv16_packed_src"
SHEET = "sjpeg_hip_sheet_ragged_yuv16_src"
SHEET_ENCODE = "sjpeg_hip_encode_ragged_sheet_yuv16_src"
SHEET_PACKED = "sjpeg_hip_encode_ragged_sheet_yuv16_packed_src"
NEW = (SAMPLES, CONVERT, ENCODE, PACKED, SHEET, SHEET_ENCODE, SHEET_PACKED)
ENTRIES = NEW[1:]
FORMATS = [(sj.SRC_YUV444, "SJPEG_HIP_SRC_YUV444", 3), (sj.SRC_YUV420, "SJPEG_HIP_SRC_YUV420", 3),
           (sj.SRC_NV12, "SJPEG_HIP_SRC_NV12", 2), (sj.SRC_NV21, "SJPEG_HIP_SRC_NV21", 2)]
SHEET44 = sj.Sheet(2, 2, (16, 16), gutter=2, margin=2, background=(16, 128, 128))
P010 = (2, 8)
BT709 = (1, 1)
L = sv._lib()


def _err():
    return L.sjpeg_hip_last_error().decode()


def _refused(rc, who, *words):
    assert rc == EINVAL
    msg = _err()
    assert msg.startswith(who + ": "), msg
    for w in words:
        assert w in msg, (w, msg)


def _frames(dims, planes=3, stride=1 << 19):
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


def _mode(fmt):
    return sj.YUV_444 if fmt == sj.SRC_YUV444 else sj.YUV_420


def _call(who, frames, fmt, sizes=None, orientations=None, colour=BT709, depth=P010, mode=None, sheet=SHEET44, engine=FAKE,
          out_bytes=1 << 30, d_out=1 << 28):
    """one of the six entries on a stand-in engine; depth: (bytes, shift[, reserved]) or None for NULL"""
    n = len(frames)
    k1, sp = _ptr(sizes, np.int32, (-1, 2))
    k2, op = _ptr(orientations, np.uint8, (-1,))
    cst = None if colour is None else sv._ColourStruct(*colour)
    dst = None if depth is None else sv._DepthStruct(*depth)
    cp, dp = (None if cst is None else C.addressof(cst)), (None if dst is None else C.addressof(dst))
    st = sj._sheet_struct("test", sheet) if sheet is not None else None
    shp = None if st is None else C.addressof(st)
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode if mode is not None else _mode(fmt), 4, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    out = (sj.RaggedFrame * 8)()
    ns, rfmt = C.c_int(-7), C.c_int(-7)
    if who == CONVERT:
        rc = L.sjpeg_hip_convert_ragged_yuv16_src(engine, fmt, n, frames, sp, op, cp, 0, dp, d_out, out_bytes, out, C.byref(rfmt), None)
    elif who == SHEET:
        rc = L.sjpeg_hip_sheet_ragged_yuv16_src(engine, fmt, n, frames, shp, sp, op, cp, 0, dp, d_out, out_bytes, out, C.byref(ns),
                                                C.byref(rfmt), None)
    elif who == ENCODE:
        rc = L.sjpeg_hip_encode_ragged_yuv16_src(engine, fmt, n, frames, C.byref(p), sp, op, cp, 0, dp, None, 0, 1 << 16, 1 << 12,
                                                 None, None, None, None)
    elif who == PACKED:
        rc = L.sjpeg_hip_encode_ragged_yuv16_packed_src(engine, fmt, n, frames, C.byref(p), sp, op, cp, 0, dp, None, 0, 1 << 16, 1 << 20,
                                                        1 << 12, 1 << 13, None, None, None, None)
    elif who == SHEET_ENCODE:
        rc = L.sjpeg_hip_encode_ragged_sheet_yuv16_src(engine, fmt, n, frames, C.byref(p), shp, sp, op, cp, 0, dp, None, 0, 1 << 16,
                                                       1 << 20, 1 << 12, None, None, None, None)
    else:
        assert who == SHEET_PACKED
        rc = L.sjpeg_hip_encode_ragged_sheet_yuv16_packed_src(engine, fmt, n, frames, C.byref(p), shp, sp, op, cp, 0, dp, None, 0, 1 << 16,
                                                              1 << 20, 1 << 12, 1 << 13, None, None, None, None)
    assert (ns.value, rfmt.value) == (-7, -7)       # refused: nothing was reported
    return rc


# ---- the arithmetic

@pytest.mark.parametrize("shift", range(9))
def test_the_own_size_formula_on_every_word(shift):
    words = np.arange(65536, dtype=np.uint16)
    st = sv._DepthStruct(2, shift)
    got = np.empty(65536, np.uint8)
    assert L.sjpeg_hip_yuv16_samples(C.addressof(st), 65536, words.ctypes.data, got.ctypes.data) == 0
    want = dm.own_size(words, shift)
    assert np.array_equal(got, want)
    # ... which is the contract's formula with S = x, A = 1, and the area model on a one-sample picture
    assert want.tolist() == [dm.round_deep(x, 1, shift) for x in range(65536)]
    assert want[0] == 0 and want[-1] == 255 and (np.diff(want.astype(int)) >= 0).all()
    if shift == 8:
        assert (want[0x7f], want[0x80], want[0xff7f], want[0xff80]) == (0, 1, 255, 255)      # 0xff80: 256 before the clamp
    if shift == 0:
        assert np.array_equal(want, np.minimum(words, 255))


def test_the_model_itself():
    """own size is the own-size formula; a whole ratio is a box average of the words, rounded once"""
    rs = np.random.RandomState(3)
    p = rs.randint(0, 65536, (6, 8)).astype(np.uint16)
    for shift in (0, 2, 8):
        assert np.array_equal(dm.area16(p, 8, 6, shift), dm.own_size(p, shift))
        box = p.astype(np.int64).reshape(3, 2, 4, 2).sum((1, 3))
        want = np.minimum(255, (2 * box + (4 << shift)) // (4 << (shift + 1)))
        assert np.array_equal(dm.area16(p, 4, 3, shift), want.astype(np.uint8))
    # rounding once: 0x7f and 0x80 both halves of a cell average to 0x7f.8 -> 0 at shift 8; rounded first they give 0 and 1 -> 1
    two = np.array([[0x7f, 0x80]], np.uint16)
    assert dm.area16(two, 1, 1, 8)[0, 0] == 0 and dm.narrowed_then_averaged(two, 1, 1, 8)[0, 0] == 1
    assert dm.area16(np.full((2, 2), 0xffff, np.uint16), 1, 1, 8)[0, 0] == 255


def test_samples_refusals_and_the_wrapper():
    buf = np.zeros(4, np.uint16)
    out = np.zeros(4, np.uint8)
    ok = sv._DepthStruct(2, 8)
    _refused(L.sjpeg_hip_yuv16_samples(None, 4, buf.ctypes.data, out.ctypes.data), SAMPLES, "depth == NULL")
    _refused(L.sjpeg_hip_yuv16_samples(C.addressof(ok), 4, None, out.ctypes.data), SAMPLES, "in or out == NULL")
    _refused(L.sjpeg_hip_yuv16_samples(C.addressof(ok), 4, buf.ctypes.data, None), SAMPLES, "in or out == NULL")
    for st, words in ((sv._DepthStruct(1, 8), "depth: bytes 1 is not 2"), (sv._DepthStruct(2, 9), "depth: shift 9 is not one of 0..8"),
                      (sv._DepthStruct(2, 8, (0, 1)), "depth: reserved must be 0")):
        _refused(L.sjpeg_hip_yuv16_samples(C.addressof(st), 4, buf.ctypes.data, out.ctypes.data), SAMPLES, words)
    assert L.sjpeg_hip_yuv16_samples(C.addressof(ok), 0, None, None) == 0
    # any 2-byte integer dtype, the bits read as unsigned; any shape
    x = np.array([[0xffff, 0x7fff], [0x80, 940 << 6]], np.uint16).view(np.int16)
    assert sv.yuv16_samples(x).tolist() == [[255, 128], [1, 235]]
    assert sv.yuv16_samples(np.array([64, 940, 1023, 4095], np.uint16), sv.VideoDepth.YUV10).tolist() == [16, 235, 255, 255]
    with pytest.raises(sj.SjpegError, match="2-byte integer"):
        sv.yuv16_samples(np.zeros(4, np.uint8))
    with pytest.raises(sj.SjpegError, match="2-byte integer"):
        sv.yuv16_samples(np.zeros(4, np.float16))
    with pytest.raises(sj.SjpegError, match="VideoDepth"):
        sv.yuv16_samples(x, 10)


# ---- argument checks with a stand-in engine: nothing touches it

@pytest.mark.parametrize("who", ENTRIES)
@pytest.mark.parametrize("fmt,name,planes", FORMATS)
def test_a_bad_depth_is_refused_and_names_the_field(who, fmt, name, planes):
    fr = _frames([(16, 16), (16, 8)], planes)
    sizes = [(8, 8), (8, 4)]
    _refused(_call(who, fr, fmt, sizes, depth=None), who, "depth == NULL")
    _refused(_call(who, fr, fmt, sizes, depth=(1, 0)), who, "depth: bytes 1 is not 2")
    _refused(_call(who, fr, fmt, sizes, depth=(0, 8)), who, "depth: bytes 0 is not 2")
    _refused(_call(who, fr, fmt, sizes, depth=(4, 8)), who, "depth: bytes 4 is not 2")
    _refused(_call(who, fr, fmt, sizes, depth=(2, 9)), who, "depth: shift 9 is not one of 0..8")
    _refused(_call(who, fr, fmt, sizes, depth=(2, 255)), who, "depth: shift 255")
    _refused(_call(who, fr, fmt, sizes, depth=(2, 8, (1, 0))), who, "depth: reserved must be 0")
    _refused(_call(who, fr, fmt, sizes, depth=(2, 2, (0, 3)), colour=None), who, "depth: reserved must be 0")


@pytest.mark.parametrize("who", ENTRIES)
@pytest.mark.parametrize("fmt,name,planes", FORMATS)
def test_planes_and_strides_by_the_element_size(who, fmt, name, planes):
    """the rules of the 8-bit entries with elements of 2 bytes: |row_stride| at least twice the 8-bit row; every plane
    and row stride a multiple of 2, frame and plane named; NULL planes"""
    dims = [(16, 16), (16, 8)]
    tail = " must be a multiple of the element size (2 bytes)"
    for i in range(planes):
        fr = _frames(dims, planes)
        fr[1].plane[i] += 1
        _refused(_call(who, fr, fmt), who, "frame 1: plane[%d]" % i + tail)
        for stride in (4097, -4097):
            fr = _frames(dims, planes)
            fr[0].row_stride[i] = stride
            _refused(_call(who, fr, fmt), who, "frame 0: row_stride[%d]" % i + tail)
        fr = _frames(dims, planes)
        fr[1].plane[i] = 0
        _refused(_call(who, fr, fmt), who, "frame 1: null plane pointer")
        # a row of plane i in bytes: 16 luma samples, 8 chroma samples or 8 pairs -- all of two bytes
        row = 2 * (16 if i == 0 or fmt == sj.SRC_YUV444 else 16 if planes == 2 else 8)
        for sign in (1, -1):
            fr = _frames(dims, planes)
            fr[1].row_stride[i] = sign * (row - 2)
            _refused(_call(who, fr, fmt), who, "frame 1: |row_stride| smaller than a row of the plane")
            fr[1].row_stride[i] = sign * row         # exactly a row: in order -- the next check speaks
            _refused(_call(who, fr, fmt, [(8, 8), (17, 4)]), who, "frame 1", "size 17x4")
    # what is a whole row of bytes is half a row of words
    fr = _frames(dims, planes, stride=16)
    _refused(_call(who, fr, fmt), who, "frame 0: |row_stride| smaller than a row of the plane")


@pytest.mark.parametrize("who", ENTRIES)
def test_a_format_that_is_no_yuv_plane_format_is_refused_by_name(who):
    for fmt, name, planes in ((sj.SRC_RGB, "SJPEG_HIP_SRC_RGB", 1), (sj.SRC_BGRA, "SJPEG_HIP_SRC_BGRA", 1),
                              (sj.SRC_GRAY, "SJPEG_HIP_SRC_GRAY", 1), (sj.SRC_RGB_PLANAR, "SJPEG_HIP_SRC_RGB_PLANAR", 3),
                              (sj.SRC_RGB_F16, "SJPEG_HIP_SRC_RGB_F16", 1), (sj.SRC_GRAY_BF16, "SJPEG_HIP_SRC_GRAY_BF16", 1)):
        fr = _frames([(16, 16), (16, 8)], planes)
        for colour in (BT709, None):
            _refused(_call(who, fr, fmt, [(8, 8), (8, 4)], colour=colour, mode=sj.YUV_420), who, name + " is not a YUV-plane format")
    _refused(_call(who, _frames([(16, 16)], 1), 99, mode=sj.YUV_420), who, "unknown source format")
    _refused(_call(who, _frames([(16, 16)], 1), 21, mode=sj.YUV_420), who, "unknown source format")     # (no format was added)


@pytest.mark.parametrize("who", ENTRIES)
@pytest.mark.parametrize("fmt,name,planes", FORMATS)
def test_what_the_counterpart_refuses_in_this_entrys_name(who, fmt, name, planes):
    fr = _frames([(16, 16), (17, 9), (8, 8)], planes)
    _refused(_call(who, fr, fmt, [(8, 8), (9, 17), (4, 4)], [6, 6, 6]), who, "frame 1", "size 9x17", "above the source's 17x9")
    _refused(_call(who, fr, fmt, [(0, 8), (16, 8), (8, 8)]), who, "frame 0", "size 0x8", "below 1")
    _refused(_call(who, fr, fmt, [(8, 8), (16, 8), (8, 8)], [1, 0, 6]), who, "frame 1", "orientation 0", "1..8")
    _refused(_call(who, fr, fmt, engine=None), who, "engine == NULL")
    _refused(_call(who, fr, fmt, colour=(2, 0)), who, "colour: matrix 2 is not one of 0..1")
    _refused(_call(who, fr, fmt, colour=(1, 1, (0, 1))), who, "colour: reserved must be 0")
    _refused(_call(who, (sj.RaggedFrame * 1)(), fmt), who, "frame 0")      # (a frame of no size, no planes)
    if who in (ENCODE, PACKED, SHEET_ENCODE, SHEET_PACKED):
        other = sj.YUV_420 if fmt == sj.SRC_YUV444 else sj.YUV_444
        _refused(_call(who, fr, fmt, [(8, 8), (16, 8), (8, 8)], mode=other), who, "yuv_mode does not match the source format")
    if who in (SHEET, SHEET_ENCODE, SHEET_PACKED):
        _refused(_call(who, fr, fmt, sheet=None), who, "sheet")
        if fmt != sj.SRC_YUV444:
            _refused(_call(who, fr, fmt, sheet=sj.Sheet(2, 2, (15, 16))), who, "sheet: cell_width 15 is odd")
        _refused(_call(who, fr, fmt, [(16, 16), (17, 8), (8, 8)]), who, "frame 1", "the thumbnail of size 17x8", "above the cell's 16x16")


def test_there_is_no_pass_through_and_no_identity_route():
    """own sizes, orientation 1 and no colour (or JFIF's own) still answer under the deep entry's name: every frame goes
    through the kernel"""
    fr = _frames([(16, 16), (17, 9)], 2)
    bad = [(16, 16), (9, 17)]
    for who in ENTRIES:
        for colour in (None, (0, 0)):
            _refused(_call(who, fr, sj.SRC_NV12, bad, colour=colour), who, "frame 1", "size 9x17")
            _refused(_call(who, fr, sj.SRC_NV12, None, [1, 9], colour=colour), who, "frame 1", "orientation 9")


def test_the_shape_entries_check_their_buffer_sized_by_the_8_bit_function():
    fr = _frames([(16, 16), (16, 8)], 2)
    sizes = [(8, 8), (8, 4)]
    need = L.sjpeg_hip_resize_ragged_yuv_bytes(sj.SRC_NV12, 2, fr, _ptr(sizes, np.int32, (-1, 2))[1], None)
    assert need == 64 + 16 + 16 + 32 + 16 + 16       # the made planes are bytes
    _refused(_call(CONVERT, fr, sj.SRC_NV12, sizes, out_bytes=need - 1), CONVERT, "bytes %d is below the %d bytes" % (need - 1, need),
             "sjpeg_hip_resize_ragged_yuv_bytes")
    _refused(_call(CONVERT, fr, sj.SRC_NV12, sizes, d_out=(1 << 28) + 8), CONVERT, "d_out must be a multiple of 16")
    _refused(_call(SHEET, fr, sj.SRC_NV12, sizes, out_bytes=100), SHEET, "bytes 100 is below", "sjpeg_hip_sheet_ragged_bytes")
    _refused(_call(CONVERT, fr, sj.SRC_NV12, sizes, d_out=None), CONVERT, "NULL")


# ---- exports, the struct and the module's names

def test_symbols_are_exported_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    declared = set(re.findall(r"\b(sjpeg_hip_[a-z_0-9]+)\s*\(", text.split("namespace sjpeg")[0]))
    for name in NEW:
        assert name in sj.EXPORTED_C_SYMBOLS and name in declared, name
        assert getattr(L, name).argtypes is not None, name
    assert declared == set(n for n in sj.EXPORTED_C_SYMBOLS if n.startswith("sjpeg_hip_"))
    assert L.sjpeg_hip_abi_version() == 18           # (entries were added, none changed)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sj.LIB_PATH]).decode()
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, out), name
    # no source format was added for the depth
    assert "SJPEG_HIP_SRC_P010" not in text and re.search(r"SJPEG_HIP_SRC_GRAY_BF16\s*=\s*20\b", text)


def test_the_struct_is_four_bytes(tmp_path):
    assert C.sizeof(sv._DepthStruct) == 4
    assert (sv._DepthStruct.bytes.offset, sv._DepthStruct.shift.offset, sv._DepthStruct.reserved.offset) == (0, 1, 2)
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "sjpeg_hip.h"\n_Static_assert(sizeof(sjpeg_hip_yuv_depth) == 4, "4 bytes");\n'
                   '_Static_assert(offsetof(sjpeg_hip_yuv_depth, shift) == 1 && offsetof(sjpeg_hip_yuv_depth, reserved) == 2, "fields");\n')
    subprocess.check_call(["gcc", "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_video_depth_maps_as_stated():
    D = sv.VideoDepth
    assert (D().bytes, D().shift) == (2, 8) and D() == D.P010 and D(10, "msb") == D.P010
    for bits in range(8, 17):
        assert (D(bits, "msb").bytes, D(bits, "msb").shift) == (2, 8)
        assert (D(bits, "lsb").bytes, D(bits, "lsb").shift) == (2, bits - 8)
    assert (D.P010.shift, D.P016.shift, D.YUV10.shift, D.YUV12.shift) == (8, 8, 2, 4)
    assert (D.P016.bits, D.YUV12.bits, D.YUV12.align) == (16, 12, "lsb")
    st = D.YUV12._struct()
    assert (st.bytes, st.shift, list(st.reserved)) == (2, 4, [0, 0])
    assert repr(D.YUV10) == "VideoDepth(10, 'lsb')" and D.YUV10 != D.P010 and len({D.P010, D(10), D.YUV10}) == 2
    for bad in (7, 17, 10.0, True, "10"):
        with pytest.raises(sj.SjpegError, match="bits"):
            D(bad)
    with pytest.raises(sj.SjpegError, match="align"):
        D(10, "high")


def test_the_new_functions_take_their_twins_arguments_plus_depth():
    for deep, twin in (("convert_deep_frames", "convert_yuv_frames"), ("encode_deep_video_frames", "encode_video_frames"),
                       ("make_deep_video_sheets", "make_video_sheets"), ("encode_deep_video_sheets", "encode_video_sheets")):
        a, b = inspect.signature(getattr(sv, deep)), inspect.signature(getattr(sv, twin))
        assert list(a.parameters)[:-1] == list(b.parameters) and list(a.parameters)[-1] == "depth", deep
        assert a.parameters["depth"].default == sv.VideoDepth.P010
        for name in b.parameters:
            assert a.parameters[name].default == b.parameters[name].default or name == "colour", (deep, name)
    # the 8-bit twins kept their signatures
    assert str(inspect.signature(sv.encode_video_frames)).endswith("packed=False, metadata=None, engine=None)")
    assert "depth" not in inspect.signature(sv.convert_yuv_frames).parameters


def test_the_binding_refuses_what_is_no_deep_frame():
    """before any device work: frames that are no CUDA tensors of a 2-byte integer dtype, a depth that is none"""
    import torch
    y = torch.zeros((4, 4), dtype=torch.int16)
    uv = torch.zeros((2, 2, 2), dtype=torch.int16)
    for fn in (sv.convert_deep_frames, sv.encode_deep_video_frames):
        with pytest.raises(sj.SjpegError, match="depth 10 is not a VideoDepth"):
            fn([(y, uv)], depth=10)
        with pytest.raises(sj.SjpegError, match="2-byte integer dtype"):
            fn([(y, uv)])                            # (on the host)
        with pytest.raises(sj.SjpegError, match="no frames"):
            fn([])
        with pytest.raises(sj.SjpegError, match="has 2 planes, the format takes 3"):
            fn([(y, uv)], fmt=sj.SRC_YUV420)
        with pytest.raises(sj.SjpegError, match="is not SRC_NV12"):
            fn([(y, uv)], fmt=sj.SRC_RGB)
