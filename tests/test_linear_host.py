"""Resize in linear light (sjpeg_hip_linear_ragged_src and the other _linear entries, sjpeg_amd.light) without a GPU:
the table against a 60-digit evaluation of its formula, every refusal before any device work with its message, the
pass-through of light = 0 under the older entry's name, the module's own refusals, and the exports."""
import ctypes as C
import hashlib
import os
import re
from decimal import ROUND_FLOOR, Decimal, getcontext

import numpy as np
import pytest

import sjpeg_amd as sj
import sjpeg_amd.light as li

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = C.c_void_p(1 << 20)          # (the checks come before the engine is touched: any non-NULL value stands in for one)
SHAPE = "sjpeg_hip_linear_ragged_src"
ENCODE = "sjpeg_hip_encode_ragged_linear_src"
PACKED = "sjpeg_hip_encode_ragged_linear_packed_src"
SHEET = "sjpeg_hip_sheet_ragged_linear_src"
SHEET_ENCODE = "sjpeg_hip_encode_ragged_sheet_linear_src"
SHEET_PACKED = "sjpeg_hip_encode_ragged_sheet_linear_packed_src"
ENTRIES = (SHAPE, ENCODE, PACKED, SHEET, SHEET_ENCODE, SHEET_PACKED)
# what light = 0 answers as: (without a flatten, with one)
OLDER = {SHAPE: ("sjpeg_hip_orient_ragged_src", "sjpeg_hip_flatten_ragged_src"),
         ENCODE: ("sjpeg_hip_encode_ragged_oriented_src", "sjpeg_hip_encode_ragged_flattened_src"),
         PACKED: ("sjpeg_hip_encode_ragged_oriented_packed_src", "sjpeg_hip_encode_ragged_flattened_packed_src"),
         SHEET: ("sjpeg_hip_sheet_ragged_src", "sjpeg_hip_sheet_ragged_flat_src"),
         SHEET_ENCODE: ("sjpeg_hip_encode_ragged_sheet_src", "sjpeg_hip_encode_ragged_sheet_flat_src"),
         SHEET_PACKED: ("sjpeg_hip_encode_ragged_sheet_packed_src", "sjpeg_hip_encode_ragged_sheet_flat_packed_src")}
YUV_FORMATS = [(sj.SRC_YUV444, "SJPEG_HIP_SRC_YUV444", 3), (sj.SRC_YUV420, "SJPEG_HIP_SRC_YUV420", 3),
               (sj.SRC_NV12, "SJPEG_HIP_SRC_NV12", 2), (sj.SRC_NV21, "SJPEG_HIP_SRC_NV21", 2)]
SHEET22 = sj.Sheet(2, 2, (16, 16), gutter=2, margin=2, background=(16, 128, 128))
WHITE = ((255, 255, 255), 0, 255.0, 0.0)
SHA = "fdb7af3c01815a2118db8e50aac3c2304205ccc3f381f8976c588642c1aa60b6"
L = li._lib()


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


def _call(who, frames, fmt=sj.SRC_RGB, light=li.LINEAR_SRGB, sizes=None, orientations=None, flatten=None, mode=sj.YUV_420, sheet=SHEET22,
          engine=FAKE, out_bytes=1 << 30, d_out=1 << 28, nframes=None, params=True, made=True):
    """one of the six entries on a stand-in engine; flatten: (background, premultiplied, alpha_scale, alpha_bias) or None"""
    n = len(frames) if nframes is None else nframes
    k1, sp = _ptr(sizes, np.int32, (-1, 2))
    k2, op = _ptr(orientations, np.uint8, (-1,))
    fst = None if flatten is None else sj._FlattenStruct((C.c_uint8 * 3)(*flatten[0]), flatten[1], flatten[2], flatten[3])
    fp = None if fst is None else C.addressof(fst)
    st = sj._sheet_struct("test", sheet) if sheet is not None else None
    shp = None if st is None else C.addressof(st)
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, 4, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    pp = C.byref(p) if params else None
    out = (sj.RaggedFrame * 8)() if made else None
    ns, rfmt = C.c_int(-7), C.c_int(-7)
    if who == SHAPE:
        rc = L.sjpeg_hip_linear_ragged_src(engine, fmt, n, frames, fp, light, sp, op, d_out, out_bytes, out, C.byref(rfmt), None)
    elif who == SHEET:
        rc = L.sjpeg_hip_sheet_ragged_linear_src(engine, fmt, n, frames, shp, fp, light, sp, op, d_out, out_bytes, out, C.byref(ns),
                                                 C.byref(rfmt), None)
    elif who == ENCODE:
        rc = L.sjpeg_hip_encode_ragged_linear_src(engine, fmt, n, frames, pp, fp, light, sp, op, None, 0, 1 << 16, 1 << 12, None, None,
                                                  None, None)
    elif who == PACKED:
        rc = L.sjpeg_hip_encode_ragged_linear_packed_src(engine, fmt, n, frames, pp, fp, light, sp, op, None, 0, 1 << 16, 1 << 20, 1 << 12,
                                                         1 << 13, None, None, None, None)
    elif who == SHEET_ENCODE:
        rc = L.sjpeg_hip_encode_ragged_sheet_linear_src(engine, fmt, n, frames, pp, shp, fp, light, sp, op, None, 0, 1 << 16, 1 << 20,
                                                        1 << 12, None, None, None, None)
    else:
        assert who == SHEET_PACKED
        rc = L.sjpeg_hip_encode_ragged_sheet_linear_packed_src(engine, fmt, n, frames, pp, shp, fp, light, sp, op, None, 0, 1 << 16, 1 << 20,
                                                               1 << 12, 1 << 13, None, None, None, None)
    assert (ns.value, rfmt.value) == (-7, -7)       # refused: nothing was reported
    return rc


# ---- the table and the inverse

def test_table_is_the_formula_in_60_digits():
    getcontext().prec = 60

    def f(c):
        return c / Decimal("12.92") if c <= Decimal("0.04045") else ((c + Decimal("0.055")) / Decimal("1.055")) ** Decimal("2.4")

    want, margin = [], Decimal(1)
    for b in range(256):
        v = Decimal(65535) * f(Decimal(b) / Decimal(255)) + Decimal("0.5")
        want.append(int(v.to_integral_value(rounding=ROUND_FLOOR)))
        margin = min(margin, abs(v - v.to_integral_value(rounding=ROUND_FLOOR)), abs(v.to_integral_value(rounding=ROUND_FLOOR) + 1 - v))
    assert margin > Decimal("0.0016")               # no entry near a rounding tie: the evaluation is not fragile
    got = li.light_table()
    assert got.dtype == np.uint16 and got.tolist() == want
    assert got[:6].tolist() == [0, 20, 40, 60, 80, 99] and got[252:].tolist() == [63795, 64372, 64952, 65535]
    assert int(got.astype(np.int64).sum()) == 5217863 and int(np.diff(got.astype(np.int64)).min()) == 19
    assert hashlib.sha256(got.astype("<u2").tobytes()).hexdigest() == SHA
    # the double-precision evaluation gives the same table
    c = np.arange(256) / 255.0
    dbl = np.floor(65535.0 * np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4) + 0.5).astype(np.int64)
    assert dbl.tolist() == want
    assert li.light_table(li.CODED).tolist() == list(range(256))
    # the header carries the table's constants as the source does
    text = open(os.path.join(ROOT, "sjpeg_amd", "csrc", "light_math.h")).read()
    body = text[text.index("kLightSrgb[256] = {"):]
    assert [int(x) for x in re.findall(r"\d+", body[body.index("{") + 1:body.index("}")])] == want
    assert "pow(" not in text


def test_round_is_the_counting_definition():
    T = [int(x) for x in li.light_table()]
    rs = np.random.RandomState(5)
    for (W, H) in ((1, 1), (2, 1), (7, 3), (65535, 1), (65535, 65535)):
        A = W * H
        sums = [0, 65535 * A] + [int(rs.randint(0, 1 << 30)) * int(rs.randint(0, 1 << 30)) % (65535 * A + 1) for _ in range(200)]
        sums += [x for k in range(1, 256) for m in [(T[k - 1] + T[k]) * A] for x in (m // 2 - 1, m // 2, -(-m // 2), -(-m // 2) + 1) if 0 <= x <= 65535 * A]
        for S in sums:
            assert li.light_round(S, W, H) == sum(1 for k in range(1, 256) if 2 * S >= (T[k - 1] + T[k]) * A), (S, W, H)
        assert [li.light_round(T[b] * A, W, H) for b in range(256)] == list(range(256))
    # the known answers, and the byte average beside them
    assert li.light_round(2 * T[255], 2, 2) == 188 and li.light_round(2 * 255, 2, 2, li.CODED) == 128
    assert li.light_round(T[255], 2, 2) == 137 and li.light_round(255, 2, 2, li.CODED) == 64
    assert li.light_round(T[100] + T[200], 2, 1) == 160 and li.light_round(300, 2, 1, li.CODED) == 150


def test_helpers_refuse():
    buf = np.zeros(256, np.uint16)
    out = C.c_uint32(7)
    _refused(L.sjpeg_hip_light_table(li.LINEAR_SRGB, None), "sjpeg_hip_light_table", "table == NULL")
    for bad in (2, -1):
        _refused(L.sjpeg_hip_light_table(bad, buf.ctypes.data), "sjpeg_hip_light_table", "light %d is not" % bad)
        _refused(L.sjpeg_hip_light_round(bad, 0, 1, 1, C.byref(out)), "sjpeg_hip_light_round", "light %d is not" % bad)
    _refused(L.sjpeg_hip_light_round(1, 0, 1, 1, None), "sjpeg_hip_light_round", "byte == NULL")
    _refused(L.sjpeg_hip_light_round(1, 0, 0, 1, C.byref(out)), "sjpeg_hip_light_round", "bad dimensions 0x1")
    _refused(L.sjpeg_hip_light_round(1, 0, 1, 65536, C.byref(out)), "sjpeg_hip_light_round", "bad dimensions 1x65536")
    _refused(L.sjpeg_hip_light_round(1, 65535 * 6 + 1, 2, 3, C.byref(out)), "sjpeg_hip_light_round", "is above")
    _refused(L.sjpeg_hip_light_round(0, 255 * 6 + 1, 2, 3, C.byref(out)), "sjpeg_hip_light_round", "is above")
    assert out.value == 7


# ---- the entries' refusals, each before the engine is touched

@pytest.mark.parametrize("who", ENTRIES)
@pytest.mark.parametrize("fmt,name,planes", YUV_FORMATS)
def test_yuv_plane_formats_are_refused_by_name(who, fmt, name, planes):
    mode = sj.YUV_444 if fmt == sj.SRC_YUV444 else sj.YUV_420
    _refused(_call(who, _frames([(32, 16)], planes), fmt, mode=mode), who, "light", name, "not RGB light")


@pytest.mark.parametrize("who", ENTRIES)
@pytest.mark.parametrize("bad", [2, -1])
def test_light_values(who, bad):
    _refused(_call(who, _frames([(32, 16)]), light=bad), who, "light %d is not SJPEG_HIP_LIGHT_CODED (0) or SJPEG_HIP_LIGHT_LINEAR_SRGB (1)" % bad)


@pytest.mark.parametrize("who", ENTRIES)
def test_null_arguments(who):
    fr = _frames([(32, 16)])
    _refused(_call(who, fr, engine=None), who, "engine == NULL")
    _refused(_call(who, None, nframes=1), who, "frames", "== NULL")
    if who in (SHAPE, SHEET):
        _refused(_call(who, fr, d_out=None), who, "d_out", "== NULL")
        _refused(_call(who, fr, made=False), who, "== NULL")
        _refused(_call(who, fr, d_out=(1 << 28) + 4), who, "d_out must be a multiple of 16")
        _refused(_call(who, fr, out_bytes=16), who, "bytes 16 is below the")
    else:
        _refused(_call(who, fr, params=False), who, "params == NULL")
    if who in (SHEET, SHEET_ENCODE, SHEET_PACKED):
        _refused(_call(who, fr, sheet=None), who, "sheet", "NULL")
    _refused(_call(who, fr, nframes=0), who, "nframes must be 1..65535")


@pytest.mark.parametrize("who", (ENCODE, PACKED, SHEET_ENCODE, SHEET_PACKED))
def test_gray_is_coded_400_only(who):
    fr = _frames([(32, 16)])
    _refused(_call(who, fr, sj.SRC_GRAY, mode=sj.YUV_420), who, "yuv_mode does not match the source format", "gray pictures are coded 4:0:0 only")


@pytest.mark.parametrize("who", ENTRIES)
def test_the_plans_own_checks_are_reached(who):
    fr = _frames([(32, 16), (20, 10)])
    _refused(_call(who, fr, sizes=[(8, 4), (21, 10)]), who, "frame 1: size 21x10 is above the source's 20x10")
    _refused(_call(who, fr, sizes=[(0, 4), (20, 10)]), who, "frame 0: size 0x4 is below 1x1")
    _refused(_call(who, fr, orientations=[1, 9]), who, "frame 1: orientation 9 is not one of 1..8")
    _refused(_call(who, fr, 99), who, "unknown source format")
    # flatten's: a format without alpha (named), premultiplied above 1, a float row too short for its alpha
    _refused(_call(who, fr, flatten=WHITE), who, "flatten: SJPEG_HIP_SRC_RGB has no alpha channel")
    _refused(_call(who, fr, sj.SRC_RGBA, flatten=((1, 2, 3), 2, 255.0, 0.0)), who, "flatten: premultiplied 2 is not 0")
    _refused(_call(who, fr, sj.SRC_RGBA_F32, flatten=((1, 2, 3), 0, float("inf"), 0.0)), who, "alpha_scale and alpha_bias must be finite")
    _refused(_call(who, _frames([(32, 16)], stride=32 * 16 - 4), sj.SRC_RGBA_F32, flatten=WHITE), who, "frame 0", "alpha")


@pytest.mark.parametrize("who", ENTRIES)
def test_light_0_answers_with_the_older_entrys_name(who):
    fr = _frames([(32, 16), (20, 10)])
    plain, flat = OLDER[who]
    _refused(_call(who, fr, light=li.CODED, orientations=[1, 9]), plain, "orientation 9 is not one of 1..8")
    _refused(_call(who, fr, sj.SRC_RGBA, light=li.CODED, orientations=[1, 9], flatten=WHITE), flat, "orientation 9 is not one of 1..8")
    _refused(_call(who, fr, light=li.CODED, flatten=WHITE), flat, "flatten: SJPEG_HIP_SRC_RGB has no alpha channel")
    # ... and is not asked about the format: the coded-light calls take what they took
    if who in (SHEET, SHEET_ENCODE, SHEET_PACKED):
        _refused(_call(who, _frames([(32, 16)], 3), sj.SRC_YUV444, light=li.CODED, mode=sj.YUV_444, orientations=[9]), plain, "orientation 9")


# ---- sjpeg_amd.light

def test_module_names_and_signatures():
    import inspect
    assert li.LINEAR_SRGB == 1 and li.CODED == 0
    assert str(inspect.signature(li.linear_resize_images)) == \
        "(images, sizes=None, box=None, orientations=None, flatten=None, layout='hwc', engine=None)"
    for fn in (li.encode_linear_images, li.encode_linear_sheets):
        names = list(inspect.signature(fn).parameters)
        for kw in ("quality", "yuv_mode", "method", "use_trellis", "target_size", "target_psnr", "packed", "metadata", "flatten", "engine"):
            assert kw in names, (fn.__name__, kw)
    for name in ("light_table", "make_linear_sheets"):
        assert callable(getattr(li, name))
    # nothing public was added to the package itself
    assert not hasattr(sj, "LINEAR_SRGB") and not hasattr(sj, "linear_resize_images") and not hasattr(sj.Engine, "linear_ragged")


def test_module_refusals():
    for bad in (2, -1, True, 1.0, "linear"):
        with pytest.raises(sj.SjpegError, match="light .* is not CODED"):
            li.light_table(bad)
    with pytest.raises(sj.SjpegError, match="linear_resize_images: flatten is not a Flatten"):
        li.linear_resize_images([], flatten=(255, 255, 255))
    with pytest.raises(sj.SjpegError, match="linear_resize_images: no images"):
        li.linear_resize_images([])
    with pytest.raises(sj.SjpegError, match="encode_linear_images: layout 'xyz' is not"):
        li.encode_linear_images([], layout="xyz")
    with pytest.raises(sj.SjpegError, match="make_linear_sheets: layout='chw' has no alpha format"):
        li.make_linear_sheets([], SHEET22, flatten=sj.Flatten(), layout="chw")
    with pytest.raises(sj.SjpegError, match="Reduced, Resized, Oriented and Flattened pictures are not taken"):
        li.encode_linear_sheets(sj.Resized([np.zeros((2, 2, 3), np.uint8)], (1, 1)), SHEET22)
    with pytest.raises(sj.SjpegError, match="give sizes or box, not both"):
        li._sizes("linear_resize_images", [(4, 4)], [(2, 2)], (2, 2), None)
    with pytest.raises(sj.SjpegError, match="one size per picture"):
        li._sizes("linear_resize_images", [(4, 4)], [(2, 2), (1, 1), (1, 1)], None, None)
    with pytest.raises(sj.SjpegError, match="box 5 is not a pair"):
        li._sizes("linear_resize_images", [(4, 4)], None, 5, None)
    with pytest.raises(sj.SjpegError, match="method 9 is not one of 0..8"):
        li._method("encode_linear_images", 9, False)
    assert li._sizes("x", [(40, 20), (20, 40)], None, (10, 10), [1, 6]) == [(10, 5), (5, 10)]
    assert li._sizes("x", [(40, 20), (20, 40)], (4, 2), None, None) == [(4, 2), (4, 2)]
    assert li._method("x", 4, True) == 7 and li._method("x", 6, True) == 8 and li._method("x", 3, True) == 3


def test_abi_version_and_symbols():
    assert L.sjpeg_hip_abi_version() == 18           # (entries were added, none changed)
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    assert re.search(r"#define\s+SJPEG_HIP_ABI_VERSION\s+18\b", text)
    assert re.search(r"#define\s+SJPEG_HIP_LIGHT_CODED\s+0\b", text) and re.search(r"#define\s+SJPEG_HIP_LIGHT_LINEAR_SRGB\s+1\b", text)
    for name in ENTRIES + ("sjpeg_hip_light_table", "sjpeg_hip_light_round"):
        assert hasattr(L, name) and name in sj.EXPORTED_C_SYMBOLS, name
        assert re.search(r"\bint\s+%s\(" % name, text), name
    assert SHA in text and "5217863" in text
