"""Video colour converted inside the ragged call (sjpeg_hip_convert_ragged_yuv_src and the other _yuv_converted_ /
_yuv_colour entries, sjpeg_amd.video) without a GPU: the formula on all 2^24 triples against the numpy model, the
tables against the float64 chain they are rounded from, the distance to the exactly rounded result, every argument
check before any device work (the frame named), the routes that convert nothing, the exports and the module's names."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import sjpeg_amd as sj
import sjpeg_amd.video as sv
import yuv_colour_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = C.c_void_p(1 << 20)          # (the checks come before the engine is touched: any non-NULL value stands in for one)
SAMPLES = "sjpeg_hip_yuv_colour_samples"
CONVERT = "sjpeg_hip_convert_ragged_yuv_src"
ENCODE = "sjpeg_hip_encode_ragged_yuv_converted_src"
PACKED = "sjpeg_hip_encode_ragged_yuv_converted_packed_src"
SHEET = "sjpeg_hip_sheet_ragged_yuv_colour_src"
SHEET_ENCODE = "sjpeg_hip_encode_ragged_sheet_yuv_colour_src"
SHEET_PACKED = "sjpeg_hip_encode_ragged_sheet_yuv_colour_packed_src"
NEW = (SAMPLES, CONVERT, ENCODE, PACKED, SHEET, SHEET_ENCODE, SHEET_PACKED)
FORMATS = [(sj.SRC_YUV444, "SJPEG_HIP_SRC_YUV444", 3), (sj.SRC_YUV420, "SJPEG_HIP_SRC_YUV420", 3),
           (sj.SRC_NV12, "SJPEG_HIP_SRC_NV12", 2), (sj.SRC_NV21, "SJPEG_HIP_SRC_NV21", 2)]
L = sv._lib()


def _err():
    return L.sjpeg_hip_last_error().decode()


def _refused(rc, who, *words):
    assert rc == EINVAL
    msg = _err()
    assert msg.startswith(who + ": "), msg
    for w in words:
        assert w in msg, (w, msg)


# ---- the arithmetic

@pytest.fixture(scope="module")
def triples():
    """all 2^24 (Y, U, V), Y slowest; never written to"""
    a = np.arange(256, dtype=np.uint8)
    y, u, v = np.meshgrid(a, a, a, indexing="ij")
    t = np.stack([y.ravel(), u.ravel(), v.ravel()], axis=1)
    t.setflags(write=False)
    return t


@pytest.mark.parametrize("src", cm.SOURCES, ids=[cm.NAMES[s] for s in cm.SOURCES])
def test_the_formula_on_every_triple(triples, src):
    """ONE call per source: the model bit for bit; and against the exactly rounded float64 result every output within 1,
    at most 0.5 % of the triples off per channel -- conditions on the fixed tables (measured: 0.39 % at most, the
    chroma of BT.601 limited; 0.19 % the luma of the two BT.709 sources)"""
    got = sv.yuv_colour_samples(triples, sv.VideoColour(*src))
    want = np.stack(cm.convert_samples(triples[:, 0], triples[:, 1], triples[:, 2], *src), axis=1)
    assert got.shape == want.shape == (1 << 24, 3) and np.array_equal(got, want)
    if src == (cm.BT601, cm.FULL):
        assert np.array_equal(got, triples)
    y0 = cm.TABLES[src][0]
    x = triples.astype(np.float64) - np.array([y0, 128.0, 128.0])
    exact = np.clip(np.rint(x @ cm.derive_matrix(*src).T + np.array([0.0, 128.0, 128.0])), 0, 255)
    off = np.abs(exact - got)
    rates = (off != 0).mean(axis=0)
    print(cm.NAMES[src], "largest distance", off.max(), "share of triples off per channel", rates)
    assert off.max() <= 1 and (rates <= 0.005).all()


def test_the_tables_are_the_rounded_matrices():
    for src in cm.SOURCES:
        y0, k = cm.TABLES[src]
        assert np.array_equal(np.rint(cm.derive_matrix(*src) * 16384.0).astype(np.int64), np.asarray(k, np.int64)), cm.NAMES[src]
        assert y0 == (16 if src[1] == cm.LIMITED else 0)
        assert k[1][0] == 0 and k[2][0] == 0         # the chroma rows never read luma
    # ... and the header states them as the model does
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    for src in cm.SOURCES[1:]:
        rows = ", ".join("{%d, %d, %d}" % r for r in cm.TABLES[src][1])
        assert rows in text, rows
    # the model on planes: luma (x, y) takes the chroma at (x / 2, y / 2)
    y = np.full((3, 5), 100, np.uint8)
    u = np.array([[128, 0, 255], [128, 128, 128]], np.uint8)
    v = np.full((2, 3), 128, np.uint8)
    yo, uo, vo = cm.convert_planes(y, u, v, cm.BT709, cm.FULL)
    assert yo[0].tolist() == [100, 100, 87, 87, 113] and yo[2].tolist() == [100] * 5 and uo[0].tolist() == [128, 1, 254]


def test_samples_refusals_and_shapes():
    ok = sv._ColourStruct(1, 1)
    buf = np.zeros((4, 3), np.uint8)
    _refused(L.sjpeg_hip_yuv_colour_samples(None, 4, buf.ctypes.data, buf.ctypes.data), SAMPLES, "colour == NULL")
    _refused(L.sjpeg_hip_yuv_colour_samples(C.addressof(ok), 4, None, buf.ctypes.data), SAMPLES, "NULL")
    _refused(L.sjpeg_hip_yuv_colour_samples(C.addressof(ok), 4, buf.ctypes.data, None), SAMPLES, "NULL")
    for st, words in ((sv._ColourStruct(2, 0), ("matrix 2", "0..1")), (sv._ColourStruct(0, 3), ("range 3", "0..1")),
                      (sv._ColourStruct(1, 1, (0, 1)), ("reserved must be 0",)), (sv._ColourStruct(1, 1, (7, 0)), ("reserved must be 0",))):
        _refused(L.sjpeg_hip_yuv_colour_samples(C.addressof(st), 4, buf.ctypes.data, buf.ctypes.data), SAMPLES, "colour: ", *words)
    assert L.sjpeg_hip_yuv_colour_samples(C.addressof(ok), 0, None, None) == 0
    # in place, any leading shape
    x = np.array([[[16, 128, 128], [235, 128, 128]], [[81, 90, 240], [0, 0, 0]]], np.uint8)
    want = sv.yuv_colour_samples(x)
    assert want.shape == x.shape and want[0].tolist() == [[0, 128, 128], [255, 128, 128]]
    y = x.copy()
    assert L.sjpeg_hip_yuv_colour_samples(C.addressof(ok), 4, y.ctypes.data, y.ctypes.data) == 0 and np.array_equal(y, want)
    with pytest.raises(sj.SjpegError, match="triples"):
        sv.yuv_colour_samples(np.zeros((4, 2), np.uint8))
    with pytest.raises(sj.SjpegError, match="VideoColour"):
        sv.yuv_colour_samples(x, "bt709")


# ---- argument checks with a stand-in engine: nothing touches it

def _frames(dims, planes=3):
    f = (sj.RaggedFrame * len(dims))()
    for k, (w, h) in enumerate(dims):
        f[k].width, f[k].height = w, h
        for i in range(planes):
            f[k].plane[i] = (1 << 30) + (i << 24)
            f[k].row_stride[i] = 1 << 19
        f[k].out_offset = (1 << 20) * k
        f[k].out_capacity = 1 << 20
    return f


def _ptr(values, dtype, shape):
    if values is None:
        return None, None
    arr = np.ascontiguousarray(np.asarray(values, dtype).reshape(shape))
    return arr, arr.ctypes.data


def _colours(colours):
    """None, one (matrix, range[, reserved]) for all frames, or a list of one per frame"""
    if colours is None:
        return None, None, 0
    per = isinstance(colours, list)
    arr = (sv._ColourStruct * (len(colours) if per else 1))(*[sv._ColourStruct(*c) for c in (colours if per else [colours])])
    return arr, C.addressof(arr), int(per)


def _params(mode, method=4):
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, method, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    p._keep = q
    return p


def _mode(fmt):
    return sj.YUV_444 if fmt == sj.SRC_YUV444 else sj.YUV_420


SHEET44 = sj.Sheet(2, 2, (16, 16), gutter=2, margin=2, background=(16, 128, 128))


def _sheet_struct(sheet):
    return sj._sheet_struct("test", sheet)


def _convert(frames, fmt, sizes, orientations, colours, mode=None, out_bytes=1 << 30, d_out=1 << 28, sheet=SHEET44, engine=FAKE):
    n = len(frames)
    k1, sp = _ptr(sizes, np.int32, (-1, 2))
    k2, op = _ptr(orientations, np.uint8, (-1,))
    k3, cp, per = _colours(colours)
    out = (sj.RaggedFrame * n)()
    rfmt = C.c_int(-7)
    rc = L.sjpeg_hip_convert_ragged_yuv_src(engine, fmt, n, frames, sp, op, cp, per, d_out, out_bytes, out, C.byref(rfmt), None)
    assert rfmt.value == -7                          # refused: nothing was reported
    return rc


def _encode(frames, fmt, sizes, orientations, colours, mode=None, sheet=SHEET44, engine=FAKE):
    k1, sp = _ptr(sizes, np.int32, (-1, 2))
    k2, op = _ptr(orientations, np.uint8, (-1,))
    k3, cp, per = _colours(colours)
    p = _params(mode if mode is not None else _mode(fmt))
    return L.sjpeg_hip_encode_ragged_yuv_converted_src(engine, fmt, len(frames), frames, C.byref(p), sp, op, cp, per, None, 0, 1 << 16,
                                                       1 << 12, None, None, None, None)


def _packed(frames, fmt, sizes, orientations, colours, mode=None, sheet=SHEET44, engine=FAKE):
    k1, sp = _ptr(sizes, np.int32, (-1, 2))
    k2, op = _ptr(orientations, np.uint8, (-1,))
    k3, cp, per = _colours(colours)
    p = _params(mode if mode is not None else _mode(fmt))
    return L.sjpeg_hip_encode_ragged_yuv_converted_packed_src(engine, fmt, len(frames), frames, C.byref(p), sp, op, cp, per, None, 0,
                                                              1 << 16, 1 << 20, 1 << 12, 1 << 13, None, None, None, None)


def _sheet(frames, fmt, sizes, orientations, colours, mode=None, out_bytes=1 << 30, d_out=1 << 28, sheet=SHEET44, engine=FAKE):
    k1, sp = _ptr(sizes, np.int32, (-1, 2))
    k2, op = _ptr(orientations, np.uint8, (-1,))
    k3, cp, per = _colours(colours)
    st = _sheet_struct(sheet) if sheet is not None else None
    out = (sj.RaggedFrame * 8)()
    ns, rfmt = C.c_int(-7), C.c_int(-7)
    rc = L.sjpeg_hip_sheet_ragged_yuv_colour_src(engine, fmt, len(frames), frames, None if st is None else C.addressof(st), sp, op, cp, per,
                                                 d_out, out_bytes, out, C.byref(ns), C.byref(rfmt), None)
    assert (ns.value, rfmt.value) == (-7, -7)
    return rc


def _sheet_encode(frames, fmt, sizes, orientations, colours, mode=None, sheet=SHEET44, engine=FAKE):
    k1, sp = _ptr(sizes, np.int32, (-1, 2))
    k2, op = _ptr(orientations, np.uint8, (-1,))
    k3, cp, per = _colours(colours)
    st = _sheet_struct(sheet) if sheet is not None else None
    p = _params(mode if mode is not None else _mode(fmt))
    return L.sjpeg_hip_encode_ragged_sheet_yuv_colour_src(engine, fmt, len(frames), frames, C.byref(p), None if st is None else C.addressof(st),
                                                          sp, op, cp, per, None, 0, 1 << 16, 1 << 20, 1 << 12, None, None, None, None)


def _sheet_packed(frames, fmt, sizes, orientations, colours, mode=None, sheet=SHEET44, engine=FAKE):
    k1, sp = _ptr(sizes, np.int32, (-1, 2))
    k2, op = _ptr(orientations, np.uint8, (-1,))
    k3, cp, per = _colours(colours)
    st = _sheet_struct(sheet) if sheet is not None else None
    p = _params(mode if mode is not None else _mode(fmt))
    return L.sjpeg_hip_encode_ragged_sheet_yuv_colour_packed_src(engine, fmt, len(frames), frames, C.byref(p),
                                                                 None if st is None else C.addressof(st), sp, op, cp, per, None, 0, 1 << 16,
                                                                 1 << 20, 1 << 12, 1 << 13, None, None, None, None)


FRAMES = [(_convert, CONVERT), (_encode, ENCODE), (_packed, PACKED)]
SHEETS = [(_sheet, SHEET), (_sheet_encode, SHEET_ENCODE), (_sheet_packed, SHEET_PACKED)]
ALL = FRAMES + SHEETS
BT709 = (1, 1)


@pytest.mark.parametrize("call,who", ALL)
@pytest.mark.parametrize("fmt,name,planes", FORMATS)
def test_a_bad_colour_is_refused_and_names_the_frame(call, who, fmt, name, planes):
    fr = _frames([(16, 16), (16, 8), (8, 8)], planes)
    sizes = [(8, 8), (8, 4), (8, 8)]
    _refused(call(fr, fmt, sizes, None, (2, 0)), who, "colour: matrix 2 is not one of 0..1", "SJPEG_HIP_MATRIX_BT601")
    _refused(call(fr, fmt, sizes, None, (0, 2)), who, "colour: range 2 is not one of 0..1", "SJPEG_HIP_RANGE_FULL")
    _refused(call(fr, fmt, sizes, None, (255, 255)), who, "colour: matrix 255")
    _refused(call(fr, fmt, sizes, None, (0, 0, (1, 0))), who, "colour: reserved must be 0")
    _refused(call(fr, fmt, sizes, [6, 1, 3], (1, 1, (0, 9))), who, "colour: reserved must be 0")
    assert "frame" not in _err()                     # (one colour for all frames: there is no frame to name)
    _refused(call(fr, fmt, sizes, None, [BT709, (1, 2), (3, 0)]), who, "frame 1: colour: range 2")
    _refused(call(fr, fmt, sizes, None, [(0, 0), (0, 0), (0, 0, (0, 1))]), who, "frame 2: colour: reserved must be 0")
    _refused(call(fr, fmt, None, None, [(2, 0), (0, 0), (0, 0)]), who, "frame 0: colour: matrix 2")


@pytest.mark.parametrize("call,who", ALL)
def test_an_rgb_like_or_gray_format_is_refused_by_name(call, who):
    for fmt, name, planes in ((sj.SRC_RGB, "SJPEG_HIP_SRC_RGB", 1), (sj.SRC_BGRA, "SJPEG_HIP_SRC_BGRA", 1),
                              (sj.SRC_GRAY, "SJPEG_HIP_SRC_GRAY", 1), (sj.SRC_RGB_PLANAR, "SJPEG_HIP_SRC_RGB_PLANAR", 3),
                              (sj.SRC_RGB_F32, "SJPEG_HIP_SRC_RGB_F32", 1), (sj.SRC_GRAY_BF16, "SJPEG_HIP_SRC_GRAY_BF16", 1)):
        fr = _frames([(16, 16), (16, 8)], planes)
        for colours in (BT709, [BT709, (0, 0)]):
            _refused(call(fr, fmt, [(8, 8), (8, 4)], None, colours, sj.YUV_420), who, name + " is not a YUV-plane format",
                     "sjpeg_hip_orient_ragged_src")
    _refused(call(_frames([(16, 16)], 1), 99, None, None, BT709, sj.YUV_420), who, "unknown source format")


@pytest.mark.parametrize("call,who", SHEETS)
def test_the_sheet_entries_take_no_rgb_format_without_a_colour_either(call, who):
    for colours in (None, (0, 0)):
        _refused(call(_frames([(16, 16)], 1), sj.SRC_RGB, None, None, colours, sj.YUV_420), who, "SJPEG_HIP_SRC_RGB is not a YUV-plane format")


@pytest.mark.parametrize("call,who", ALL)
@pytest.mark.parametrize("fmt,name,planes", FORMATS)
def test_what_the_counterpart_refuses_in_its_words(call, who, fmt, name, planes):
    fr = _frames([(16, 16), (17, 9), (8, 8)], planes)
    _refused(call(fr, fmt, [(8, 8), (9, 17), (4, 4)], [6, 6, 6], BT709), who, "frame 1", "size 9x17", "above the source's 17x9")
    _refused(call(fr, fmt, [(0, 8), (16, 8), (8, 8)], None, BT709), who, "frame 0", "size 0x8", "below 1")
    _refused(call(fr, fmt, [(8, 8), (16, 8), (8, 8)], [1, 0, 6], BT709), who, "frame 1", "orientation 0", "1..8")
    _refused(call(fr, fmt, [(8, 8), (16, 8), (8, 8)], [1, 1, 9], [BT709] * 3), who, "frame 2", "orientation 9", "1..8")
    _refused(call(fr, fmt, None, None, BT709, engine=None), who, "engine == NULL")
    _refused(call((sj.RaggedFrame * 1)(), fmt, None, None, BT709), who, "frame 0")      # (a frame of no size, no planes)
    if call in (_encode, _packed, _sheet_encode, _sheet_packed):
        other = sj.YUV_420 if fmt == sj.SRC_YUV444 else sj.YUV_444
        _refused(call(fr, fmt, [(8, 8), (16, 8), (8, 8)], None, BT709, other), who, "yuv_mode does not match the source format")


@pytest.mark.parametrize("call,who", SHEETS)
def test_the_sheet_checks_come_in_the_sheet_entries_words(call, who):
    fr = _frames([(32, 32), (32, 32)], 2)
    _refused(call(fr, sj.SRC_NV12, None, None, BT709, sheet=None), who, "sheet")
    _refused(call(fr, sj.SRC_NV12, None, None, BT709, sheet=sj.Sheet(2, 2, (15, 16))), who, "sheet: cell_width 15 is odd")
    _refused(call(fr, sj.SRC_NV12, [(32, 32), (8, 8)], None, [BT709, BT709]), who, "frame 0", "the thumbnail of size 32x32", "above the cell's 16x16")


def test_the_shape_entries_check_their_buffer():
    fr = _frames([(16, 16), (16, 8)], 2)
    sizes = [(8, 8), (8, 4)]
    need = L.sjpeg_hip_resize_ragged_yuv_bytes(sj.SRC_NV12, 2, fr, _ptr(sizes, np.int32, (-1, 2))[1], None)
    assert need == 64 + 16 + 16 + 32 + 16 + 16
    _refused(_convert(fr, sj.SRC_NV12, sizes, None, BT709, out_bytes=need - 1), CONVERT, "bytes %d is below the %d bytes" % (need - 1, need),
             "converted planes", "sjpeg_hip_resize_ragged_yuv_bytes")
    _refused(_convert(fr, sj.SRC_NV12, sizes, None, BT709, d_out=(1 << 28) + 8), CONVERT, "d_out must be a multiple of 16")
    _refused(_sheet(fr, sj.SRC_NV12, sizes, None, BT709, out_bytes=100), SHEET, "bytes 100 is below", "sjpeg_hip_sheet_ragged_bytes")
    _refused(_sheet(fr, sj.SRC_NV12, sizes, None, BT709, d_out=(1 << 28) + 4), SHEET, "d_out must be a multiple of 16")
    _refused(_convert(fr, sj.SRC_NV12, sizes, None, BT709, d_out=None), CONVERT, "NULL")


def test_nothing_to_convert_is_the_counterpart_under_its_name():
    """colour NULL, or BT.601 full range for every frame: the messages are the existing entries'"""
    fr = _frames([(16, 16), (17, 9)], 2)
    bad = [(8, 8), (9, 17)]
    for colours in (None, (0, 0), [(0, 0), (0, 0)]):
        _refused(_convert(fr, sj.SRC_NV12, bad, None, colours), "sjpeg_hip_resize_ragged_yuv_src", "frame 1", "size 9x17")
        _refused(_encode(fr, sj.SRC_NV12, bad, None, colours), "sjpeg_hip_encode_ragged_yuv_resized_src", "frame 1", "size 9x17")
        _refused(_packed(fr, sj.SRC_NV12, bad, None, colours), "sjpeg_hip_encode_ragged_yuv_resized_packed_src", "frame 1", "size 9x17")
        _refused(_sheet(fr, sj.SRC_NV12, bad, None, colours), "sjpeg_hip_sheet_ragged_src", "frame 1", "size 9x17")
        _refused(_sheet_encode(fr, sj.SRC_NV12, bad, None, colours), "sjpeg_hip_encode_ragged_sheet_src", "frame 1", "size 9x17")
        _refused(_sheet_packed(fr, sj.SRC_NV12, bad, None, colours), "sjpeg_hip_encode_ragged_sheet_packed_src", "frame 1", "size 9x17")
    # one converting frame among identities: the entry's own name
    _refused(_encode(fr, sj.SRC_NV12, bad, None, [(0, 0), BT709]), ENCODE, "frame 1", "size 9x17")
    # a colour that is not in order is no identity
    _refused(_encode(fr, sj.SRC_NV12, None, None, (0, 0, (0, 1))), ENCODE, "reserved must be 0")


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


def test_the_struct_is_four_bytes(tmp_path):
    assert C.sizeof(sv._ColourStruct) == 4
    assert (sv._ColourStruct.matrix.offset, sv._ColourStruct.range.offset, sv._ColourStruct.reserved.offset) == (0, 1, 2)
    src = tmp_path / "size.c"
    src.write_text('#include "sjpeg_hip.h"\n_Static_assert(sizeof(sjpeg_hip_yuv_colour) == 4, "4 bytes");\n'
                   '_Static_assert(SJPEG_HIP_MATRIX_BT709 == 1 && SJPEG_HIP_RANGE_LIMITED == 1 && SJPEG_HIP_MATRIX_BT601 == 0 && '
                   'SJPEG_HIP_RANGE_FULL == 0, "values");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")])


def test_the_plan_and_math_files_have_no_hip_in_them():
    for f in ("yuv_colour_plan.cc", "yuv_colour_math.h"):
        text = open(os.path.join(ROOT, "sjpeg_amd", "csrc", f)).read()
        assert "__global__" not in text and "hipLaunch" not in text and "hip_runtime" not in text, f


def test_the_video_module():
    for name in ("VideoColour", "convert_yuv_frames", "encode_video_frames", "encode_video_sheets", "yuv_colour_samples", "make_video_sheets"):
        assert hasattr(sv, name), name
    sig = inspect.signature(sv.encode_video_frames)
    assert list(sig.parameters) == ["frames", "fmt", "colour", "sizes", "box", "orientations", "quality", "method", "target_size",
                                    "target_psnr", "packed", "metadata", "engine"]
    assert sig.parameters["fmt"].default == sj.SRC_NV12 and sig.parameters["colour"].default == sv.VideoColour("bt709", "limited")
    sig = inspect.signature(sv.encode_video_sheets)
    assert list(sig.parameters)[:4] == ["frames", "fmt", "sheet", "colour"]
    assert list(inspect.signature(sv.VideoColour).parameters) == ["matrix", "range"]
    c = sv.VideoColour()
    assert (c.matrix, c.range) == (sv.MATRIX_BT709, sv.RANGE_LIMITED) and not c.identity
    assert sv.VideoColour("BT601", "Full").identity and sv.VideoColour(0, 1) == sv.VideoColour("bt601", "limited")
    assert repr(sv.VideoColour(1, 0)) == "VideoColour('bt709', 'full')"
    for bad in (("bt2020", "limited"), ("bt709", "studio"), (2, 0), (0, 2), (None, 0)):
        with pytest.raises(sj.SjpegError, match="VideoColour"):
            sv.VideoColour(*bad)
    # nothing new is defined in the package itself: its pinned names stay what they were
    assert not hasattr(sj, "VideoColour") and not hasattr(sj, "encode_video_frames")
