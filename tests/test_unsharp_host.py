"""The unsharp mask (sjpeg_hip_unsharp_ragged_src and the other _unsharp entries, sjpeg_amd.unsharp) without a GPU: the
formula on single neighbourhoods against the definition in numpy integers, every refusal before any device work with
its message, the pass-through of no unsharp and of amount 0 under the older entry's name, the module's own refusals, and
the exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sjpeg_amd as sj
import sjpeg_amd.light as li
import sjpeg_amd.unsharp as un
import sjpeg_amd.video as sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = C.c_void_p(1 << 20)          # (the checks come before the engine is touched: any non-NULL value stands in for one)
SHAPE = "sjpeg_hip_unsharp_ragged_src"
ENCODE = "sjpeg_hip_encode_ragged_unsharp_src"
PACKED = "sjpeg_hip_encode_ragged_unsharp_packed_src"
YSHAPE = "sjpeg_hip_unsharp_ragged_yuv_src"
YENCODE = "sjpeg_hip_encode_ragged_yuv_unsharp_src"
YPACKED = "sjpeg_hip_encode_ragged_yuv_unsharp_packed_src"
RGB_ENTRIES, YUV_ENTRIES = (SHAPE, ENCODE, PACKED), (YSHAPE, YENCODE, YPACKED)
ENTRIES = RGB_ENTRIES + YUV_ENTRIES
# what no unsharp, or amount 0 for every frame, answers as.  The RGB entries: (light 0 without a flatten, light 0 with one,
# linear light); the YUV entries: (no depth and no colour to convert, no depth with a colour, a depth)
OLDER = {SHAPE: ("sjpeg_hip_orient_ragged_src", "sjpeg_hip_flatten_ragged_src", "sjpeg_hip_linear_ragged_src"),
         ENCODE: ("sjpeg_hip_encode_ragged_oriented_src", "sjpeg_hip_encode_ragged_flattened_src", "sjpeg_hip_encode_ragged_linear_src"),
         PACKED: ("sjpeg_hip_encode_ragged_oriented_packed_src", "sjpeg_hip_encode_ragged_flattened_packed_src",
                  "sjpeg_hip_encode_ragged_linear_packed_src"),
         YSHAPE: ("sjpeg_hip_resize_ragged_yuv_src", "sjpeg_hip_convert_ragged_yuv_src", "sjpeg_hip_convert_ragged_yuv16_src"),
         YENCODE: ("sjpeg_hip_encode_ragged_yuv_resized_src", "sjpeg_hip_encode_ragged_yuv_converted_src", "sjpeg_hip_encode_ragged_yuv16_src"),
         YPACKED: ("sjpeg_hip_encode_ragged_yuv_resized_packed_src", "sjpeg_hip_encode_ragged_yuv_converted_packed_src",
                   "sjpeg_hip_encode_ragged_yuv16_packed_src")}
YUV_FORMATS = [(sj.SRC_YUV444, "SJPEG_HIP_SRC_YUV444", 3), (sj.SRC_YUV420, "SJPEG_HIP_SRC_YUV420", 3),
               (sj.SRC_NV12, "SJPEG_HIP_SRC_NV12", 2), (sj.SRC_NV21, "SJPEG_HIP_SRC_NV21", 2)]
RGB_FORMATS = [(sj.SRC_RGB, "SJPEG_HIP_SRC_RGB"), (sj.SRC_BGRA, "SJPEG_HIP_SRC_BGRA"), (sj.SRC_GRAY, "SJPEG_HIP_SRC_GRAY"),
               (sj.SRC_RGB_PLANAR_F16, "SJPEG_HIP_SRC_RGB_PLANAR_F16")]
WHITE = ((255, 255, 255), 0, 255.0, 0.0)
BT709 = (1, 1)
P010 = (2, 8, 0)
L = un._lib()


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


def _call(who, frames, fmt=None, unsharp=((32, 0, 0, 0),), per_frame=0, light=li.CODED, sizes=None, orientations=None, flatten=None,
          colour=None, depth=None, mode=None, engine=FAKE, out_bytes=1 << 30, d_out=1 << 28, nframes=None, params=True, made=True):
    """one of the six entries on a stand-in engine.  unsharp: rows (amount, threshold, reserved 0, reserved 1) or None;
    flatten: (background, premultiplied, alpha_scale, alpha_bias); colour: (matrix, range); depth: (bytes, shift, reserved)"""
    yuv = who in YUV_ENTRIES
    if fmt is None:
        fmt = sj.SRC_YUV420 if yuv else sj.SRC_RGB
    if mode is None:
        mode = sj.YUV_444 if fmt == sj.SRC_YUV444 else sj.YUV_420
    n = len(frames) if nframes is None else nframes
    k1, sp = _ptr(sizes, np.int32, (-1, 2))
    k2, op = _ptr(orientations, np.uint8, (-1,))
    k3, up = _ptr(unsharp, np.uint8, (-1, 4))
    fst = None if flatten is None else sj._FlattenStruct((C.c_uint8 * 3)(*flatten[0]), flatten[1], flatten[2], flatten[3])
    fp = None if fst is None else C.addressof(fst)
    cst = None if colour is None else sv._ColourStruct(*colour)
    cp = None if cst is None else C.addressof(cst)
    dst = None if depth is None else sv._DepthStruct(depth[0], depth[1], (C.c_uint8 * 2)(depth[2], 0))
    dp = None if dst is None else C.addressof(dst)
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, 4, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    pp = C.byref(p) if params else None
    out = (sj.RaggedFrame * 8)() if made else None
    rfmt = C.c_int(-7)
    if who == SHAPE:
        rc = L.sjpeg_hip_unsharp_ragged_src(engine, fmt, n, frames, fp, light, sp, op, up, per_frame, d_out, out_bytes, out, C.byref(rfmt), None)
    elif who == ENCODE:
        rc = L.sjpeg_hip_encode_ragged_unsharp_src(engine, fmt, n, frames, pp, fp, light, sp, op, up, per_frame, None, 0, 1 << 16, 1 << 12,
                                                   None, None, None, None)
    elif who == PACKED:
        rc = L.sjpeg_hip_encode_ragged_unsharp_packed_src(engine, fmt, n, frames, pp, fp, light, sp, op, up, per_frame, None, 0, 1 << 16,
                                                          1 << 20, 1 << 12, 1 << 13, None, None, None, None)
    elif who == YSHAPE:
        rc = L.sjpeg_hip_unsharp_ragged_yuv_src(engine, fmt, n, frames, sp, op, cp, 0, dp, up, per_frame, d_out, out_bytes, out,
                                                C.byref(rfmt), None)
    elif who == YENCODE:
        rc = L.sjpeg_hip_encode_ragged_yuv_unsharp_src(engine, fmt, n, frames, pp, sp, op, cp, 0, dp, up, per_frame, None, 0, 1 << 16,
                                                       1 << 12, None, None, None, None)
    else:
        assert who == YPACKED
        rc = L.sjpeg_hip_encode_ragged_yuv_unsharp_packed_src(engine, fmt, n, frames, pp, sp, op, cp, 0, dp, up, per_frame, None, 0,
                                                              1 << 16, 1 << 20, 1 << 12, 1 << 13, None, None, None, None)
    assert rfmt.value == -7             # refused: nothing was reported
    return rc


def _own(who, dims):
    """frames the entry's family takes"""
    return _frames(dims, 3 if who in YUV_ENTRIES else 1)


# ---- the formula on single neighbourhoods

def _define(n, amount, threshold):
    """sjpeg_hip.h's definition on neighbourhoods [..., 3, 3], in Python integers"""
    n = np.asarray(n, np.int64)
    w = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.int64)
    S = (n * w).sum(axis=(-1, -2))
    p = n[..., 1, 1]
    D = 16 * p - S
    v = np.clip((512 * p + amount * D + 256) // 512, 0, 255)         # (// is the floor)
    return np.where(np.abs(D) < 16 * threshold, p, v).astype(np.uint8)


def test_unsharp_sample_is_the_definition():
    rs = np.random.RandomState(11)
    for amount, threshold in ((32, 0), (64, 0), (255, 0), (0, 0), (1, 0), (32, 25), (200, 3), (255, 255), (97, 1)):
        n = rs.randint(0, 256, (400, 3, 3)).astype(np.uint8)
        n[:50] = rs.randint(0, 2, (50, 3, 3)) * 255                     # (the extremes: both clamps)
        n[50:100] = np.clip(rs.randint(120, 126, (50, 1, 1)) + rs.randint(-2, 3, (50, 3, 3)), 0, 255)   # (near flat: the threshold's edge)
        assert np.array_equal(un.unsharp_sample(n, amount, threshold), _define(n, amount, threshold)), (amount, threshold)
    assert un.unsharp_sample(n.reshape(400, 9), 97, 1).shape == (400,) and un.unsharp_sample(n[0]).shape == ()


def _windows(im):
    """the neighbourhoods [H, W, 3, 3] of a picture [H, W], the edge replicated"""
    e = np.pad(im, 1, mode="edge")
    H, W = im.shape
    return np.stack([np.stack([e[i:i + H, j:j + W] for j in range(3)], axis=-1) for i in range(3)], axis=-2)


def test_known_answers():
    rows = np.array([[100] * 4 + [200] * 4] * 3, np.uint8)
    assert (un.unsharp_sample(_windows(rows), 32, 0) == [100, 100, 100, 75, 225, 200, 200, 200]).all()
    assert (un.unsharp_sample(_windows(rows), 64, 0) == [100, 100, 100, 50, 250, 200, 200, 200]).all()
    assert np.array_equal(un.unsharp_sample(_windows(rows), 32, 26), rows)
    assert np.array_equal(un.unsharp_sample(_windows(rows), 32, 25), un.unsharp_sample(_windows(rows), 32, 0))
    assert un.unsharp_sample(_windows(np.array([[10, 12]], np.uint8)), 32, 0).tolist() == [[10, 13]]
    board = np.where((np.arange(4)[:, None] + np.arange(4)[None, :]) & 1, 200, 100).astype(np.uint8)
    assert un.unsharp_sample(_windows(board), 32, 0)[0].tolist() == [63, 250, 50, 238]
    # the clamp at both ends; a constant and a 1 x 1 picture
    assert un.unsharp_sample([255] * 4 + [0] + [255] * 4, 255, 0) == 0 and un.unsharp_sample([0] * 4 + [255] + [0] * 4, 255, 0) == 255
    assert (un.unsharp_sample(_windows(np.full((3, 4), 91, np.uint8)), 255, 0) == 91).all()
    assert un.unsharp_sample(_windows(np.array([[201]], np.uint8)), 255, 0)[0, 0] == 201


def test_sample_refuses():
    n = np.arange(9, dtype=np.uint8)
    out = C.c_uint32(7)
    who = "sjpeg_hip_unsharp_sample"
    _refused(L.sjpeg_hip_unsharp_sample(32, 0, None, C.byref(out)), who, "n or byte == NULL")
    _refused(L.sjpeg_hip_unsharp_sample(32, 0, n.ctypes.data, None), who, "n or byte == NULL")
    _refused(L.sjpeg_hip_unsharp_sample(256, 0, n.ctypes.data, C.byref(out)), who, "amount 256 is not one of 0..255")
    _refused(L.sjpeg_hip_unsharp_sample(-1, 0, n.ctypes.data, C.byref(out)), who, "amount -1 is not one of 0..255")
    _refused(L.sjpeg_hip_unsharp_sample(0, 256, n.ctypes.data, C.byref(out)), who, "threshold 256 is not one of 0..255")
    assert out.value == 7


# ---- the entries' refusals, each before the engine is touched; the messages are pinned here

@pytest.mark.parametrize("who", ENTRIES)
def test_a_reserved_byte_names_the_frame(who):
    fr = _own(who, [(32, 16), (20, 10), (8, 8)])
    _refused(_call(who, fr, unsharp=[(32, 0, 0, 0), (0, 0, 0, 0), (32, 0, 0, 1)], per_frame=1), who, "frame 2: unsharp: reserved must be 0")
    _refused(_call(who, fr, unsharp=[(0, 0, 0, 0), (0, 0, 9, 0), (0, 0, 0, 0)], per_frame=1), who, "frame 1: unsharp: reserved must be 0")
    assert _err() == who + ": frame 1: unsharp: reserved must be 0"
    _refused(_call(who, fr, unsharp=[(32, 0, 1, 0)]), who, "unsharp: reserved must be 0")
    assert _err() == who + ": unsharp: reserved must be 0"


@pytest.mark.parametrize("who", RGB_ENTRIES)
@pytest.mark.parametrize("fmt,name,planes", YUV_FORMATS)
def test_yuv_plane_formats_are_pointed_at_the_yuv_entries(who, fmt, name, planes):
    _refused(_call(who, _frames([(32, 16)], planes), fmt), who, name + " is a YUV-plane format",
             "sjpeg_hip_unsharp_ragged_yuv_src and sjpeg_hip_encode_ragged_yuv_unsharp_src")


@pytest.mark.parametrize("who", YUV_ENTRIES)
@pytest.mark.parametrize("fmt,name", RGB_FORMATS)
def test_other_formats_are_pointed_at_the_rgb_entries(who, fmt, name):
    _refused(_call(who, _frames([(32, 16)], 3), fmt, mode=sj.YUV_400 if fmt == sj.SRC_GRAY else sj.YUV_420), who,
             name + " is not a YUV-plane format", "sjpeg_hip_unsharp_ragged_src and sjpeg_hip_encode_ragged_unsharp_src")


@pytest.mark.parametrize("who", ENTRIES)
def test_null_arguments(who):
    fr = _own(who, [(32, 16)])
    _refused(_call(who, fr, engine=None), who, "engine == NULL")
    _refused(_call(who, None, nframes=1), who, "frames", "== NULL")
    if who in (SHAPE, YSHAPE):
        _refused(_call(who, fr, d_out=None), who, "d_out", "== NULL")
        _refused(_call(who, fr, made=False), who, "== NULL")
        _refused(_call(who, fr, d_out=(1 << 28) + 4), who, "d_out must be a multiple of 16")
        _refused(_call(who, fr, out_bytes=16), who, "bytes 16 is below the")
    else:
        _refused(_call(who, fr, params=False), who, "params == NULL")
    _refused(_call(who, fr, nframes=0), who, "nframes must be 1..65535")
    _refused(_call(who, fr, 99), who, "unknown source format")


@pytest.mark.parametrize("who", ENTRIES)
def test_the_older_entries_checks_are_reached(who):
    fr = _own(who, [(32, 16), (20, 10)])
    _refused(_call(who, fr, sizes=[(8, 4), (21, 10)]), who, "frame 1: size 21x10 is above the source's 20x10")
    _refused(_call(who, fr, sizes=[(0, 4), (20, 10)]), who, "frame 0: size 0x4 is below 1x1")
    _refused(_call(who, fr, orientations=[1, 9]), who, "frame 1: orientation 9 is not one of 1..8")
    if who in RGB_ENTRIES:
        _refused(_call(who, fr, light=2), who, "light 2 is not SJPEG_HIP_LIGHT_CODED (0) or SJPEG_HIP_LIGHT_LINEAR_SRGB (1)")
        _refused(_call(who, fr, flatten=WHITE), who, "flatten: SJPEG_HIP_SRC_RGB has no alpha channel")
        _refused(_call(who, fr, sj.SRC_RGBA, flatten=((1, 2, 3), 2, 255.0, 0.0)), who, "flatten: premultiplied 2 is not 0")
        if who != SHAPE:
            _refused(_call(who, fr, sj.SRC_GRAY, mode=sj.YUV_420), who, "yuv_mode does not match the source format",
                     "gray pictures are coded 4:0:0 only")
    else:
        _refused(_call(who, fr, colour=(2, 0)), who, "colour: matrix 2 is not one of 0..1")
        _refused(_call(who, fr, depth=(1, 0, 0)), who, "depth: bytes 1 is not 2")
        _refused(_call(who, fr, depth=(2, 9, 0)), who, "depth: shift 9")
        _refused(_call(who, fr, depth=(2, 8, 1)), who, "depth: reserved must be 0")
        # (16-bit samples: planes and strides are multiples of 2)
        odd = _frames([(32, 16)], 3, stride=(1 << 19) + 1)
        _refused(_call(who, odd, depth=P010), who, "frame 0")
        if who != YSHAPE:
            _refused(_call(who, fr, mode=sj.YUV_444), who, "yuv_mode does not match the source format")
    # the order: the family, then (RGB) the light or (YUV) the depth, then the reserved byte, then the orientations and the plan
    bad = [(32, 0, 0, 7)]
    if who in RGB_ENTRIES:
        _refused(_call(who, _frames([(32, 16)], 3), sj.SRC_YUV420, light=2, unsharp=bad, orientations=[9]), who, "is a YUV-plane format")
        if who != SHAPE:
            _refused(_call(who, fr, light=2, unsharp=bad, orientations=[9, 1]), who, "light 2 is not")
            _refused(_call(who, fr, unsharp=bad, orientations=[9, 1]), who, "unsharp: reserved must be 0")
    elif who != YSHAPE:
        _refused(_call(who, fr, depth=(1, 0, 0), unsharp=bad, orientations=[9, 1]), who, "depth: bytes 1 is not 2")
        _refused(_call(who, fr, unsharp=bad, orientations=[9, 1]), who, "unsharp: reserved must be 0")


# ---- the route rules: nothing to sharpen is the older entry, under its name

@pytest.mark.parametrize("who", RGB_ENTRIES)
@pytest.mark.parametrize("unsharp,per_frame", [(None, 0), (None, 1), ([(0, 9, 0, 0)], 0), ([(0, 0, 0, 0), (0, 255, 0, 0)], 1)])
def test_nothing_to_sharpen_answers_with_the_older_rgb_entrys_name(who, unsharp, per_frame):
    fr = _frames([(32, 16), (20, 10)])
    plain, flat, linear = OLDER[who]
    _refused(_call(who, fr, unsharp=unsharp, per_frame=per_frame, orientations=[1, 9]), plain, "orientation 9 is not one of 1..8")
    _refused(_call(who, fr, sj.SRC_RGBA, unsharp=unsharp, per_frame=per_frame, orientations=[1, 9], flatten=WHITE), flat, "orientation 9 is not")
    _refused(_call(who, fr, unsharp=unsharp, per_frame=per_frame, orientations=[1, 9], light=li.LINEAR_SRGB), linear, "orientation 9 is not")
    _refused(_call(who, fr, unsharp=unsharp, per_frame=per_frame, light=3), linear, "light 3 is not SJPEG_HIP_LIGHT_CODED (0)")


@pytest.mark.parametrize("who", YUV_ENTRIES)
@pytest.mark.parametrize("unsharp,per_frame", [(None, 0), ([(0, 9, 0, 0)], 0), ([(0, 0, 0, 0), (0, 255, 0, 0)], 1)])
def test_nothing_to_sharpen_answers_with_the_older_yuv_entrys_name(who, unsharp, per_frame):
    fr = _frames([(32, 16), (20, 10)], 3)
    resized, converted, deep = OLDER[who]
    _refused(_call(who, fr, unsharp=unsharp, per_frame=per_frame, orientations=[1, 9]), resized, "orientation 9 is not one of 1..8")
    _refused(_call(who, fr, unsharp=unsharp, per_frame=per_frame, orientations=[1, 9], colour=BT709), converted, "orientation 9 is not")
    _refused(_call(who, fr, unsharp=unsharp, per_frame=per_frame, orientations=[1, 9], depth=P010), deep, "orientation 9 is not")
    # (the encodes' format check is the converted entry's own prologue's, in front of its hand-over to the resized one)
    _refused(_call(who, fr, sj.SRC_RGB, unsharp=unsharp, per_frame=per_frame), resized if who == YSHAPE else converted,
             "SJPEG_HIP_SRC_RGB is not a YUV-plane format")


@pytest.mark.parametrize("who", ENTRIES)
def test_one_sharpened_frame_is_enough_for_the_new_name(who):
    fr = _own(who, [(32, 16), (20, 10)])
    _refused(_call(who, fr, unsharp=[(0, 0, 0, 0), (1, 0, 0, 0)], per_frame=1, orientations=[1, 9]), who, "frame 1: orientation 9")
    # (per_frame == 0: unsharp[0] alone is read)
    older = OLDER[who][0]
    _refused(_call(who, fr, unsharp=[(0, 0, 0, 0), (1, 0, 0, 0)], per_frame=0, orientations=[1, 9]), older, "frame 1: orientation 9")


# ---- sjpeg_amd.unsharp

def test_module_names_and_signatures():
    import inspect
    assert un.Unsharp().amount == 32 and un.Unsharp().threshold == 0 and un.Unsharp(7, 9) == un.Unsharp(7, 9) and repr(un.Unsharp(7, 9)) == "Unsharp(7, 9)"
    assert C.sizeof(un._UnsharpStruct) == 4
    for fn, kws in ((un.unsharp_images, ("images", "sizes", "box", "orientations", "unsharp", "light", "flatten", "layout", "engine")),
                    (un.encode_unsharp_images, ("box", "unsharp", "light", "flatten", "quality", "yuv_mode", "method", "use_trellis", "target_size",
                                                "target_psnr", "packed", "metadata", "engine")),
                    (un.encode_unsharp_video_frames, ("frames", "fmt", "colour", "box", "unsharp", "depth", "quality", "packed", "metadata", "engine")),
                    (un.unsharp_ragged, ("engine", "fmt", "planes_per_frame", "dims", "sizes", "orientations", "flatten", "light", "unsharp", "out")),
                    (un.encode_ragged_unsharp, ("unsharp", "search", "metadata", "packed"))):
        names = list(inspect.signature(fn).parameters)
        for kw in kws:
            assert kw in names, (fn.__name__, kw)
    assert inspect.signature(un.encode_unsharp_video_frames).parameters["depth"].default is None
    assert callable(un.unsharp_sample) and callable(un.unsharp_video_frames)
    # nothing public was added to the package itself
    assert not hasattr(sj, "Unsharp") and not hasattr(sj, "unsharp_images") and not hasattr(sj.Engine, "unsharp_ragged")


def test_module_refusals():
    for bad in (-1, 256, True, 1.5, "32", None):
        with pytest.raises(sj.SjpegError, match="Unsharp: amount .* is not one of 0..255"):
            un.Unsharp(bad)
        with pytest.raises(sj.SjpegError, match="Unsharp: threshold .* is not one of 0..255"):
            un.Unsharp(32, bad)
    with pytest.raises(sj.SjpegError, match="unsharp_sample: n is uint8"):
        un.unsharp_sample(np.zeros((4, 8), np.uint8))
    with pytest.raises(sj.SjpegError, match="x: unsharp 5 is not an Unsharp or a sequence"):
        un._unsharp_args("x", 2, 5)
    with pytest.raises(sj.SjpegError, match=r"x: unsharp is one Unsharp or a sequence of one per frame \(2\)"):
        un._unsharp_args("x", 2, [un.Unsharp()])
    with pytest.raises(sj.SjpegError, match="x: unsharp is one Unsharp or a sequence"):
        un._unsharp_args("x", 2, [un.Unsharp(), (32, 0)])
    assert un._unsharp_args("x", 2, None) == (None, None, 0)
    arr, addr, per = un._unsharp_args("x", 2, [un.Unsharp(1, 2), un.Unsharp(3, 4)])
    assert per == 1 and bytes(arr) == bytes([1, 2, 0, 0, 3, 4, 0, 0]) and addr == C.addressof(arr)
    assert un._unsharp_args("x", 2, un.Unsharp(5, 6))[2] == 0
    with pytest.raises(sj.SjpegError, match="unsharp_images: no images"):
        un.unsharp_images([])
    with pytest.raises(sj.SjpegError, match="unsharp_images: flatten is not a Flatten"):
        un.unsharp_images([], flatten=(255, 255, 255))
    with pytest.raises(sj.SjpegError, match="light .* is not CODED"):
        un.unsharp_images([], light=2)
    with pytest.raises(sj.SjpegError, match="encode_unsharp_images: layout 'xyz' is not"):
        un.encode_unsharp_images([], layout="xyz")
    with pytest.raises(sj.SjpegError, match="encode_unsharp_video_frames: no frames"):
        un.encode_unsharp_video_frames([])
    with pytest.raises(sj.SjpegError, match="unsharp_video_frames: depth 10 is not a VideoDepth"):
        un.unsharp_video_frames([], depth=10)
    assert un._light_of("x", None) == li.CODED and un._light_of("x", True) == li.LINEAR_SRGB and un._light_of("x", li.LINEAR_SRGB) == 1


def test_abi_version_and_symbols():
    assert L.sjpeg_hip_abi_version() == 18           # (entries were added, none changed)
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    assert re.search(r"#define\s+SJPEG_HIP_ABI_VERSION\s+18\b", text)
    for name in ENTRIES + ("sjpeg_hip_unsharp_sample",):
        assert hasattr(L, name) and name in sj.EXPORTED_C_SYMBOLS, name
        assert re.search(r"\bint\s+%s\(" % name, text), name
    assert re.search(r"typedef struct sjpeg_hip_unsharp \{\s*uint8_t amount;[^}]*uint8_t threshold;[^}]*uint8_t reserved\[2\];", text)
    # the kernel, the host and the stand-alone tests share one statement of the formula
    csrc = os.path.join(ROOT, "sjpeg_amd", "csrc")
    for f in ("unsharp.hip", "unsharp_plan.cc"):
        assert '#include "unsharp_math.h"' in open(os.path.join(csrc, f)).read()
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"HOST_SRCS :=.*\bunsharp_plan\b", mk) and re.search(r"HIP_SRCS :=.*\bunsharp\b", mk)
