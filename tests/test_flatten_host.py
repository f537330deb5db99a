"""Alpha flattened inside the ragged call (sjpeg_hip_flatten_ragged_src, sjpeg_hip_encode_ragged_flattened_src, the flat
sheet entries, Flattened) without a GPU: the exports, the struct, every argument check before any device work (the
frame and the word named), flatten == NULL reaching the unflattened entry, the Flattened wrapper, and the sheet
entries' bytes and places."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sjpeg_amd as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = C.c_void_p(1 << 20)          # (the checks come before the engine is touched: any non-NULL value stands in for one)
NEW = ("sjpeg_hip_flatten_ragged_src", "sjpeg_hip_encode_ragged_flattened_src", "sjpeg_hip_encode_ragged_flattened_packed_src",
       "sjpeg_hip_sheet_ragged_flat_src", "sjpeg_hip_encode_ragged_sheet_flat_src", "sjpeg_hip_encode_ragged_sheet_flat_packed_src")
FLATTEN, ENCODE, PACKED, SHEET, SHEET_ENCODE, SHEET_PACKED = NEW
ALPHA = (sj.SRC_BGRA, sj.SRC_RGBA, sj.SRC_RGBA_F32, sj.SRC_RGBA_F16, sj.SRC_RGBA_BF16)
NO_ALPHA = [(sj.SRC_RGB, "SJPEG_HIP_SRC_RGB", 1, sj.YUV_420), (sj.SRC_GRAY, "SJPEG_HIP_SRC_GRAY", 1, sj.YUV_400),
            (sj.SRC_GRAY_F16, "SJPEG_HIP_SRC_GRAY_F16", 1, sj.YUV_400), (sj.SRC_RGB_F32, "SJPEG_HIP_SRC_RGB_F32", 1, sj.YUV_420),
            (sj.SRC_RGB_PLANAR, "SJPEG_HIP_SRC_RGB_PLANAR", 3, sj.YUV_420), (sj.SRC_RGB_PLANAR_BF16, "SJPEG_HIP_SRC_RGB_PLANAR_BF16", 3, sj.YUV_420),
            (sj.SRC_NV12, "SJPEG_HIP_SRC_NV12", 2, sj.YUV_420), (sj.SRC_NV21, "SJPEG_HIP_SRC_NV21", 2, sj.YUV_420),
            (sj.SRC_YUV420, "SJPEG_HIP_SRC_YUV420", 3, sj.YUV_420), (sj.SRC_YUV444, "SJPEG_HIP_SRC_YUV444", 3, sj.YUV_444)]


def _err():
    return sj.lib().sjpeg_hip_last_error().decode()


def _refused(rc, who, *words):
    assert rc == EINVAL
    msg = _err()
    assert who in msg, msg
    for w in words:
        assert w in msg, (w, msg)


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


def _flat(background=(255, 255, 255), premultiplied=0, scale=255.0, bias=0.0):
    return sj._FlattenStruct((C.c_uint8 * 3)(*background), premultiplied, scale, bias)


def _params(mode, method=4):
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, method, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    p._keep = q
    return p


SHEET22 = sj.Sheet(2, 2, (16, 16), gutter=2, margin=2)


def _flatten(frames, fmt, flat, sizes, orientations, mode=None, out_bytes=1 << 30, d_out=1 << 28):
    n = len(frames)
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    out = (sj.RaggedFrame * n)()
    rfmt = C.c_int(-7)
    rc = sj.lib().sjpeg_hip_flatten_ragged_src(FAKE, fmt, n, frames, None if flat is None else C.addressof(flat), ptr, optr, d_out,
                                               out_bytes, out, C.byref(rfmt), None)
    assert rfmt.value == -7                       # refused: nothing was reported
    return rc


def _encode(frames, fmt, flat, sizes, orientations, mode=sj.YUV_420):
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    p = _params(mode if mode is not None else sj.YUV_420)
    return sj.lib().sjpeg_hip_encode_ragged_flattened_src(FAKE, fmt, len(frames), frames, C.byref(p), None if flat is None else C.addressof(flat),
                                                          ptr, optr, None, 0, 1 << 16, 1 << 12, None, None, None, None)


def _packed(frames, fmt, flat, sizes, orientations, mode=sj.YUV_420):
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    p = _params(mode if mode is not None else sj.YUV_420)
    return sj.lib().sjpeg_hip_encode_ragged_flattened_packed_src(FAKE, fmt, len(frames), frames, C.byref(p),
                                                                 None if flat is None else C.addressof(flat), ptr, optr, None, 0, 1 << 16,
                                                                 1 << 20, 1 << 12, 1 << 13, None, None, None, None)


def _sheet(frames, fmt, flat, sizes, orientations, mode=None, sheet=SHEET22):
    n = len(frames)
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    st = sheet._struct()
    out = (sj.RaggedFrame * n)()
    ns, rfmt = C.c_int(-7), C.c_int(-7)
    rc = sj.lib().sjpeg_hip_sheet_ragged_flat_src(FAKE, fmt, n, frames, C.addressof(st), None if flat is None else C.addressof(flat), ptr, optr,
                                                  1 << 28, 1 << 30, out, C.byref(ns), C.byref(rfmt), None)
    assert (ns.value, rfmt.value) == (-7, -7)
    return rc


def _sheet_encode(frames, fmt, flat, sizes, orientations, mode=sj.YUV_420, sheet=SHEET22):
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    st = sheet._struct()
    p = _params(mode if mode is not None else sj.YUV_420)
    return sj.lib().sjpeg_hip_encode_ragged_sheet_flat_src(FAKE, fmt, len(frames), frames, C.byref(p), C.addressof(st),
                                                           None if flat is None else C.addressof(flat), ptr, optr, None, 0, 1 << 16, 1 << 20,
                                                           1 << 12, None, None, None, None)


def _sheet_packed(frames, fmt, flat, sizes, orientations, mode=sj.YUV_420, sheet=SHEET22):
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    st = sheet._struct()
    p = _params(mode if mode is not None else sj.YUV_420)
    return sj.lib().sjpeg_hip_encode_ragged_sheet_flat_packed_src(FAKE, fmt, len(frames), frames, C.byref(p), C.addressof(st),
                                                                  None if flat is None else C.addressof(flat), ptr, optr, None, 0, 1 << 16,
                                                                  1 << 24, 1 << 12, 1 << 13, None, None, None, None)


ALL = [(_flatten, FLATTEN), (_encode, ENCODE), (_packed, PACKED), (_sheet, SHEET), (_sheet_encode, SHEET_ENCODE), (_sheet_packed, SHEET_PACKED)]


# ---- exports and the struct

def test_symbols_are_exported_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    declared = set(re.findall(r"\b(sjpeg_hip_[a-z_0-9]+)\s*\(", text.split("namespace sjpeg")[0]))
    for name in NEW:
        assert name in sj.EXPORTED_C_SYMBOLS and name in declared, name
        assert getattr(sj.lib(), name).argtypes is not None, name


def test_the_struct_is_twelve_bytes(tmp_path):
    assert C.sizeof(sj._FlattenStruct) == 12
    assert (sj._FlattenStruct.premultiplied.offset, sj._FlattenStruct.alpha_scale.offset, sj._FlattenStruct.alpha_bias.offset) == (3, 4, 8)
    # ... and so is the C one
    import subprocess
    src = tmp_path / "size.c"
    src.write_text('#include "sjpeg_hip.h"\n_Static_assert(sizeof(sjpeg_hip_flatten) == 12, "12 bytes");\n'
                   '_Static_assert(__builtin_offsetof(sjpeg_hip_flatten, alpha_scale) == 4, "scale at 4");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")])


def test_the_arithmetic_header_has_no_hip_in_it():
    text = open(os.path.join(ROOT, "sjpeg_amd", "csrc", "flatten_math.h")).read()
    assert "hip_runtime" not in text and "__global__" not in text


# ---- argument checks with a stand-in engine: nothing touches it

@pytest.mark.parametrize("call,who", ALL)
def test_a_format_without_alpha_is_named(call, who):
    for fmt, name, planes, mode in NO_ALPHA:
        fr = _frames([(16, 16), (8, 8)], planes)
        for sizes, orientations in ((None, None), ([(8, 8), (8, 8)], [6, 1])):
            _refused(call(fr, fmt, _flat(), sizes, orientations, mode), who, name, "alpha")


@pytest.mark.parametrize("call,who", ALL)
@pytest.mark.parametrize("fmt", ALPHA)
def test_premultiplied_above_one(call, who, fmt):
    fr = _frames([(16, 16), (8, 8)])
    for v in (2, 255):
        _refused(call(fr, fmt, _flat(premultiplied=v), None, None), who, "premultiplied", str(v))


@pytest.mark.parametrize("call,who", ALL)
def test_the_alpha_transform_must_be_finite_for_floats(call, who):
    fr = _frames([(16, 16), (8, 8)])
    for fmt in (sj.SRC_RGBA_F32, sj.SRC_RGBA_F16, sj.SRC_RGBA_BF16):
        for scale, bias in ((float("nan"), 0.0), (float("inf"), 0.0), (255.0, float("-inf")), (255.0, float("nan"))):
            _refused(call(fr, fmt, _flat(scale=scale, bias=bias), None, None), who, "alpha_scale", "finite")


def test_the_alpha_transform_is_ignored_for_bytes():
    """NaN in a byte format's alpha_scale is not looked at: the call goes on to its next check"""
    fr = _frames([(16, 16), (8, 8)])
    for fmt in (sj.SRC_BGRA, sj.SRC_RGBA):
        _refused(_flatten(fr, fmt, _flat(scale=float("nan"), bias=float("inf")), None, None, out_bytes=16), FLATTEN, "bytes 16")


@pytest.mark.parametrize("call,who", ALL)
def test_a_float_row_one_element_short_names_the_frame_and_alpha(call, who):
    """the unflattened formats read three of a pixel's four elements, so their rows may end behind the last B; under
    flatten the alpha is read"""
    for fmt, esz in ((sj.SRC_RGBA_F32, 4), (sj.SRC_RGBA_F16, 2), (sj.SRC_RGBA_BF16, 2)):
        for sign in (1, -1):
            fr = _frames([(16, 16), (9, 8)])
            fr[1].row_stride[0] = sign * (9 * 4 * esz - esz)
            _refused(call(fr, fmt, _flat(), None, None), who, "frame 1", "alpha", str(9 * 4 * esz))
            fr[1].row_stride[0] = sign * 9 * 4 * esz            # exactly a row: in order (the next check answers)
            fr[0].row_stride[0] = sign * (16 * 4 * esz - esz)
            _refused(call(fr, fmt, _flat(), None, None), who, "frame 0", "alpha")


def test_a_row_that_holds_its_alpha_passes_the_plan():
    """... while the same short row is legal without flatten, and a full one under it (seen at the next check)"""
    fr = _frames([(9, 8)])
    fr[0].row_stride[0] = 9 * 4 * 4 - 4
    out, rfmt = (sj.RaggedFrame * 1)(), C.c_int(-7)
    rc = sj.lib().sjpeg_hip_orient_ragged_src(FAKE, sj.SRC_RGBA_F32, 1, fr, None, None, 1 << 28, 16, out, C.byref(rfmt), None)
    _refused(rc, "sjpeg_hip_orient_ragged_src", "bytes 16")
    fr[0].row_stride[0] = 9 * 4 * 4
    _refused(_flatten(fr, sj.SRC_RGBA_F32, _flat(), None, None, out_bytes=16), FLATTEN, "bytes 16", "sjpeg_hip_orient_ragged_bytes")


@pytest.mark.parametrize("call,who", ALL)
def test_the_inherited_size_and_orientation_checks(call, who):
    fr = _frames([(16, 16), (17, 9), (8, 8)])
    for fmt in (sj.SRC_RGBA, sj.SRC_RGBA_F16):
        _refused(call(fr, fmt, _flat(), None, [1, 0, 6]), who, "frame 1", "orientation 0", "1..8")
        _refused(call(fr, fmt, _flat(), [(8, 8), (9, 17), (4, 4)], [6, 6, 6]), who, "frame 1", "size 9x17", "above the source's 17x9")
        _refused(call(fr, fmt, _flat(), [(0, 8), (16, 9), (8, 8)], None), who, "frame 0", "size 0x8", "below 1")


@pytest.mark.parametrize("call,who", ALL)
def test_the_frame_checks_of_the_ragged_entries(call, who):
    def two():
        return _frames([(16, 16), (16, 16)])
    f = two(); f[1].plane[0] = None
    _refused(call(f, sj.SRC_RGBA, _flat(), None, None), who, "frame 1", "null plane")
    f = two(); f[1].row_stride[0] = 63
    _refused(call(f, sj.SRC_BGRA, _flat(), None, None), who, "frame 1", "row_stride")
    f = two(); f[0].width = 0
    _refused(call(f, sj.SRC_RGBA, _flat(), None, None), who, "frame 0", "dimensions")
    f = two(); f[1].plane[0] = (1 << 30) + 2
    _refused(call(f, sj.SRC_RGBA_F32, _flat(), None, None), who, "frame 1", "element size")


def test_bytes_one_short_and_alignment():
    dims, sizes, orientations = [(17, 9), (130, 70), (8, 8)], [(3, 2), (129, 1), (8, 8)], [6, 5, 2]
    fr = _frames(dims)
    keep, ptr = _sizes(sizes)
    okeep, optr = _orients(orientations)
    need = sj.lib().sjpeg_hip_orient_ragged_bytes(sj.SRC_RGBA, 3, fr, ptr, optr)
    assert need == sj.lib().sjpeg_hip_orient_ragged_bytes(sj.SRC_RGB, 3, fr, ptr, optr) > 0
    _refused(_flatten(fr, sj.SRC_RGBA, _flat(), sizes, orientations, out_bytes=need - 1), FLATTEN, "bytes", str(need))
    _refused(_flatten(fr, sj.SRC_RGBA, _flat(), sizes, orientations, d_out=(1 << 28) + 4), FLATTEN, "multiple of 16")


def test_null_arguments():
    L = sj.lib()
    fr = _frames([(16, 16)])
    fl = _flat()
    out, rfmt, ns = (sj.RaggedFrame * 1)(), C.c_int(0), C.c_int(0)
    p = _params(sj.YUV_420)
    st = SHEET22._struct()
    good = [FAKE, sj.SRC_RGBA, 1, fr, C.addressof(fl), None, None, 1 << 28, 1 << 20, out, C.byref(rfmt), None]
    for k in (0, 3, 4, 7, 9, 10):
        args = list(good); args[k] = None
        assert L.sjpeg_hip_flatten_ragged_src(*args) == EINVAL and FLATTEN in _err() and "NULL" in _err(), k
    good = [FAKE, sj.SRC_RGBA, 1, fr, C.addressof(st), C.addressof(fl), None, None, 1 << 28, 1 << 20, out, C.byref(ns), C.byref(rfmt), None]
    for k in (0, 3, 4, 5, 8, 10, 11, 12):
        args = list(good); args[k] = None
        assert L.sjpeg_hip_sheet_ragged_flat_src(*args) == EINVAL and SHEET in _err() and "NULL" in _err(), k
    good = [FAKE, sj.SRC_RGBA, 1, fr, C.byref(p), C.addressof(fl), None, None, None, 0, 1 << 16, 1 << 12, None, None, None, None]
    for k in (0, 3, 4, 10, 11):
        args = list(good); args[k] = None
        assert L.sjpeg_hip_encode_ragged_flattened_src(*args) == EINVAL and ENCODE in _err() and "NULL" in _err(), k
    good = [FAKE, sj.SRC_RGBA, 1, fr, C.byref(p), C.addressof(fl), None, None, None, 0, 1 << 16, 1 << 20, 1 << 12, 1 << 13, None, None, None, None]
    for k in (0, 3, 4, 10, 12, 13):
        args = list(good); args[k] = None
        assert L.sjpeg_hip_encode_ragged_flattened_packed_src(*args) == EINVAL and PACKED in _err() and "NULL" in _err(), k
    good = [FAKE, sj.SRC_RGBA, 1, fr, C.byref(p), C.addressof(st), C.addressof(fl), None, None, None, 0, 1 << 16, 1 << 20, 1 << 12, None, None, None, None]
    for k in (0, 3, 4, 5, 11, 13):
        args = list(good); args[k] = None
        assert L.sjpeg_hip_encode_ragged_sheet_flat_src(*args) == EINVAL and SHEET_ENCODE in _err() and "NULL" in _err(), k
    # the inner call's parameter checks come before any device work too
    bad = _params(sj.YUV_420, method=9)
    assert L.sjpeg_hip_encode_ragged_flattened_src(FAKE, sj.SRC_RGBA, 1, fr, C.byref(bad), C.addressof(fl), None, None, None, 0, 1 << 16, 1 << 12,
                                                   None, None, None, None) == EINVAL
    assert "method" in _err() and ENCODE in _err()


@pytest.mark.parametrize("call,inner", [(_encode, "sjpeg_hip_encode_ragged_oriented_src"), (_packed, "sjpeg_hip_encode_ragged_oriented_packed_src"),
                                        (_sheet_encode, "sjpeg_hip_encode_ragged_sheet_src"), (_sheet_packed, "sjpeg_hip_encode_ragged_sheet_packed_src")])
def test_flatten_null_is_the_unflattened_call(call, inner):
    """flatten == NULL: the oriented / sheet entry on the same arguments, any format -- its own checks answer in its name"""
    fr = _frames([(16, 16), (17, 9)])
    _refused(call(fr, sj.SRC_RGB, None, None, [1, 9]), inner, "frame 1", "orientation 9")
    _refused(call(fr, sj.SRC_RGBA, None, [(8, 8), (18, 9)], [6, 6]), inner, "frame 1", "size 18x9")
    nv = _frames([(16, 16), (32, 8)], planes=2)
    if "sheet" not in inner:
        _refused(call(nv, sj.SRC_NV12, None, None, [1, 6]), inner, "SJPEG_HIP_SRC_NV12", "not oriented")


@pytest.mark.parametrize("call,who", [(_encode, ENCODE), (_packed, PACKED)])
def test_there_is_no_pass_through_under_flatten(call, who):
    """own sizes and orientation 1 still go through the plan: the inner call's checks see SJPEG_HIP_SRC_RGB pictures and
    answer in the flattened entry's name"""
    fr = _frames([(16, 16), (17, 9)])
    for sizes, orientations in ((None, None), ([(16, 16), (17, 9)], [1, 1])):
        fr[1].row_stride[0] = 17 * 4 - 1
        _refused(call(fr, sj.SRC_RGBA, _flat(), sizes, orientations), who, "frame 1", "row_stride")
        fr[1].row_stride[0] = 1 << 19


# ---- the sheet entries: bytes and places are those of RGB frames

def test_flat_sheets_have_the_bytes_and_places_of_rgb_frames():
    dims = [(40, 30), (9, 7), (64, 64), (5, 100), (33, 1)]
    sheet = sj.Sheet(2, 2, (21, 17), gutter=3, margin=5, background=(1, 2, 3))
    for sizes, orientations in ((None, None), (None, [1, 6, 7, 8, 3]), ([(20, 15), (9, 7), (16, 16), (2, 21), (17, 1)], [1, 2, 1, 5, 1])):
        want = sj.sheet_places(sheet, dims, sj.SRC_RGB, sizes, orientations)
        st = sheet._struct()
        keep, ptr = _sizes(sizes)
        okeep, optr = _orients(orientations)
        rgb_bytes = sj.lib().sjpeg_hip_sheet_ragged_bytes(sj.SRC_RGB, len(dims), _frames(dims), C.addressof(st), ptr, optr)
        assert rgb_bytes > 0
        for fmt in ALPHA:
            assert sj.sheet_places(sheet, dims, fmt, sizes, orientations) == want
            assert sj.lib().sjpeg_hip_sheet_ragged_bytes(fmt, len(dims), _frames(dims), C.addressof(st), ptr, optr) == rgb_bytes
            # ... and the flat entry asks for exactly those bytes
            out, ns, rfmt = (sj.RaggedFrame * 2)(), C.c_int(-7), C.c_int(-7)
            fl = _flat()
            rc = sj.lib().sjpeg_hip_sheet_ragged_flat_src(FAKE, fmt, len(dims), _frames(dims), C.addressof(st), C.addressof(fl), ptr, optr,
                                                          1 << 28, rgb_bytes - 1, out, C.byref(ns), C.byref(rfmt), None)
            _refused(rc, SHEET, "bytes %d" % (rgb_bytes - 1), str(rgb_bytes))


def test_a_thumbnail_above_its_cell_is_refused_under_flatten():
    for call, who in ALL[3:]:
        _refused(call(_frames([(40, 30)]), sj.SRC_RGBA, _flat(), [(20, 15)], None), who, "frame 0", "above the cell's 16x16")


# ---- Flatten, Flattened

def test_flatten_description():
    f = sj.Flatten()
    assert (f.background, f.premultiplied, f.alpha_scale, f.alpha_bias) == ((255, 255, 255), False, 255.0, 0.0)
    st = sj.Flatten((17, 128, 250), True, 1.0, 0.5)._struct()
    assert (tuple(st.background), st.premultiplied, st.alpha_scale, st.alpha_bias) == ((17, 128, 250), 1, 1.0, 0.5)
    for bad in ((1, 2), (1, 2, 256), (-1, 0, 0), "white", None):
        with pytest.raises(sj.SjpegError, match="background"):
            sj.Flatten(bad)
    for bad in (2, -1, "yes", None, 1.0):
        with pytest.raises(sj.SjpegError, match="premultiplied"):
            sj.Flatten(premultiplied=bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(sj.SjpegError, match="finite"):
            sj.Flatten(alpha_scale=bad)
        with pytest.raises(sj.SjpegError, match="finite"):
            sj.Flatten(alpha_bias=bad)


def test_flattened_wrapper():
    ims = [np.zeros((8, 8, 4), np.uint8), np.zeros((4, 6, 4), np.uint8), np.zeros((3, 3, 4), np.uint8)]
    r = sj.Flattened(ims)
    assert r.images == ims and r.orientations is None and r.sizes is None and r.fp is None
    assert r.flatten.background == (255, 255, 255) and r.flatten.premultiplied is False
    r = sj.Flattened(tuple(ims), (0, 0, 0), True, 1.0, 2.0, orientations=[1, 8, np.int64(3)], sizes=(2, 3))
    assert r.orientations == [1, 8, 3] and r.sizes == [(2, 3)] * 3
    assert (r.flatten.background, r.flatten.premultiplied, r.flatten.alpha_scale, r.flatten.alpha_bias) == ((0, 0, 0), True, 1.0, 2.0)
    fp = sj.FloatPixels(ims, 127.5, 127.5)
    r = sj.Flattened(fp, orientations=6)
    assert r.fp is fp and r.images == ims and r.orientations == [6] * 3
    with pytest.raises(sj.SjpegError, match="2 orientations for 3 pictures"):
        sj.Flattened(ims, orientations=[6, 6])
    with pytest.raises(sj.SjpegError, match="picture 1"):
        sj.Flattened(ims, orientations=[1, 9, 1])
    with pytest.raises(sj.SjpegError, match="picture 1"):
        sj.Flattened(ims, sizes=[(1, 1), (0, 2), (1, 1)])
    with pytest.raises(sj.SjpegError, match="background"):
        sj.Flattened(ims, background=(1, 2))
    # what the calls unwrap
    assert sj._flattened("x", ims, False) == (ims, None)
    got, flat = sj._flattened("x", r, False)
    assert got == ims and flat is r
    with pytest.raises(sj.SjpegError, match="'chw' has no alpha format"):
        sj._flattened("encode_images", r, True)
    # one wrapper a picture
    rgb = [np.zeros((8, 8, 3), np.uint8)]
    for inner in (sj.Reduced(rgb, 2), sj.Resized(rgb, (1, 1)), sj.Oriented(rgb, 6), sj.Flattened(ims)):
        with pytest.raises(sj.SjpegError, match="already"):
            sj.Flattened(inner)
    for outer in (lambda x: sj.Reduced(x, 2), lambda x: sj.Resized(x, (1, 1)), lambda x: sj.Resized.fit(x, (2, 2)),
                  lambda x: sj.Oriented(x, 6), lambda x: sj.Oriented.fit(x, 6, (2, 2))):
        with pytest.raises(sj.SjpegError, match="Flattened already"):
            outer(sj.Flattened(ims))


def test_flattened_fit_takes_the_upright_box():
    ims = [np.zeros((30, 40, 4), np.uint8), np.zeros((4, 6, 4), np.uint8), np.zeros((100, 10, 4), np.uint8)]
    f = sj.Flattened.fit(ims, (32, 16))
    assert f.sizes == [(21, 16), (6, 4), sj.fit_size(10, 100, (32, 16))] and f.orientations is None
    f = sj.Flattened.fit(ims, (32, 16), background=(0, 0, 0), orientations=[6, 8, 5])
    assert f.sizes == sj.Oriented.fit([np.zeros(i.shape[:2] + (3,), np.uint8) for i in ims], [6, 8, 5], (32, 16)).sizes
    assert f.sizes[0] == (16, 12) and f.orientations == [6, 8, 5] and f.flatten.background == (0, 0, 0)
    with pytest.raises(sj.SjpegError, match="'chw' has no alpha format"):
        sj.Flattened.fit(ims, (32, 16), layout="chw")
    with pytest.raises(sj.SjpegError, match="pair"):
        sj.Flattened.fit(ims, 16)


def test_flattened_goes_through_the_calls_own_checks():
    ims = [np.zeros((8, 8, 4), np.uint8)]
    for call in (lambda r: sj.encode_images(r), lambda r: sj.compress_images(r), lambda r: sj.encode_images_full(r),
                 lambda r: sj.encode_images_full_meta(r, None), lambda r: sj.flatten_images(ims)):
        with pytest.raises(sj.SjpegError, match="image 0"):
            call(sj.Flattened(ims))
    for call in (lambda r: sj.encode_images(r, layout="chw"), lambda r: sj.compress_images(r, layout="chw"),
                 lambda r: sj.encode_images_full_meta(r, None, layout="chw"), lambda r: sj.flatten_images(r, layout="chw")):
        with pytest.raises(sj.SjpegError, match="'chw' has no alpha format"):
            call(sj.Flattened(ims))
    with pytest.raises(sj.SjpegError, match="Flattened pictures are not taken"):
        sj.riskiness_images(sj.Flattened(ims))
    sheet = sj.Sheet(1, 1, (8, 8))
    for call in (sj.make_sheets, sj.encode_sheets):
        with pytest.raises(sj.SjpegError, match="image 0"):
            call(ims, sheet, flatten=True)
        with pytest.raises(sj.SjpegError, match="'chw' has no alpha format"):
            call(ims, sheet, flatten=True, layout="chw")
        with pytest.raises(sj.SjpegError, match="Flattened pictures are not taken"):
            call(sj.Flattened(ims), sheet)
        with pytest.raises(sj.SjpegError, match="flatten is None, True"):
            call(ims, sheet, flatten="white")


def test_the_flatten_of_a_sheet_call():
    sheet = sj.Sheet(1, 1, (8, 8), background=(9, 8, 7))
    assert sj._sheet_flatten("x", None, sheet) is None
    assert sj._sheet_flatten("x", True, sheet).background == (9, 8, 7)
    assert sj._sheet_flatten("x", (1, 2, 3), sheet).background == (1, 2, 3)
    f = sj._sheet_flatten("x", ((1, 2, 3), True), sheet)
    assert f.background == (1, 2, 3) and f.premultiplied is True
    own = sj.Flatten((4, 5, 6), True)
    assert sj._sheet_flatten("x", own, sheet) is own
    assert sj._sheet_flatten("x", sj.Flattened([np.zeros((2, 2, 4), np.uint8)], (4, 4, 4)), sheet).background == (4, 4, 4)
