"""The search with any sampling and with the trellis (sjpeg_hip_encode_ragged_full_src, _full_packed_src,
sjpeg_hip_engine_search_stats) without a GPU: the entry points are declared, exported and in the library, their argument
checks come before any device work and name the argument or the frame, encode_images_full checks its arguments, and the
older entry points keep their refusals."""
import ctypes as C
import re
import os

import numpy as np
import pytest

import sjpeg_amd as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = "sjpeg_hip_encode_ragged_full_src"
PACKED = "sjpeg_hip_encode_ragged_full_packed_src"
STATS = "sjpeg_hip_engine_search_stats"
EINVAL = -1
FAKE = C.c_void_p(1 << 20)          # (the checks come before the engine is touched: any non-NULL value stands in for one)


def test_declared_exported_and_in_the_library():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    for name in (FULL, PACKED, STATS):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in sj.EXPORTED_C_SYMBOLS
        assert hasattr(sj.lib(), name)
    assert sj.lib().sjpeg_hip_abi_version() == 18
    assert re.search(r"#define\s+SJPEG_HIP_ABI_VERSION\s+18\b", text)


def test_argument_types():
    L = sj.lib()
    assert list(getattr(L, FULL).argtypes) == [C.c_void_p, C.c_int, C.c_int, C.POINTER(sj.RaggedFrame),
                                               C.POINTER(sj.RaggedParams), C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                               C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p]
    assert list(getattr(L, PACKED).argtypes) == list(L.sjpeg_hip_encode_ragged_packed_src.argtypes)
    assert getattr(L, STATS).restype is C.c_int


def _frame(w=16, h=16, plane=1 << 24):
    f = (sj.RaggedFrame * 2)()
    for k in range(2):
        f[k].width, f[k].height = w, h
        f[k].plane[0] = plane
        f[k].row_stride[0] = 3 * w
        f[k].out_offset = 4096 * k
        f[k].out_capacity = 4096
    return f


def _params(mode=sj.YUV_AUTO, method=7, search=None, per_frame=0):
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, method, q.ctypes.data, 0, None, 0x78, 12, 1, search, per_frame)
    p._keep = (q, search)
    return p


def _search(mode=1, value=1000.0, passes=5):
    return (sj.SearchParams * 2)(sj.SearchParams(1, 1000.0, passes, 1.0, 0.0, 100.0),
                                 sj.SearchParams(mode, value, passes, 1.0, 0.0, 100.0))


def _full(engine, params, frames=True, d_out=1 << 16, d_sizes=1 << 12, fmt=sj.SRC_RGB, nframes=2):
    fr = _frame() if frames is True else frames
    return getattr(sj.lib(), FULL)(engine, fmt, nframes, fr, params, d_out, d_sizes, None, None, None, None)


def _packed(engine, params, frames=True, d_packed=1 << 16, d_offsets=1 << 14, d_sizes=1 << 12, fmt=sj.SRC_RGB):
    fr = _frame() if frames is True else frames
    return getattr(sj.lib(), PACKED)(engine, fmt, 2, fr, params, d_packed, 1 << 20, d_offsets, d_sizes, None, None, None,
                                     None)


def _refused(rc, who, *words):
    assert rc == EINVAL
    msg = sj.lib().sjpeg_hip_last_error().decode()
    assert who in msg
    for w in words:
        assert w in msg, (w, msg)


def test_null_arguments_are_named():
    p = _params()
    _refused(_full(None, C.byref(p)), FULL, "engine")
    _refused(_full(FAKE, None), FULL, "params")
    _refused(_full(FAKE, C.byref(p), frames=None), FULL, "frames")
    _refused(_full(FAKE, C.byref(p), d_out=None), FULL, "d_out")
    _refused(_full(FAKE, C.byref(p), d_sizes=None), FULL, "d_sizes")
    _refused(_packed(None, C.byref(p)), PACKED, "engine")
    _refused(_packed(FAKE, None), PACKED, "params")
    _refused(_packed(FAKE, C.byref(p), frames=None), PACKED, "frames")
    _refused(_packed(FAKE, C.byref(p), d_packed=None), PACKED, "d_packed")
    _refused(_packed(FAKE, C.byref(p), d_offsets=None), PACKED, "d_offsets")
    _refused(_packed(FAKE, C.byref(p), d_packed=(1 << 16) + 8), PACKED, "multiple of 16")
    stats = (C.c_uint64 * 6)()
    assert getattr(sj.lib(), STATS)(None, stats) == EINVAL
    assert getattr(sj.lib(), STATS)(FAKE, None) == EINVAL


@pytest.mark.parametrize("call,who", [(_full, FULL), (_packed, PACKED)])
def test_bad_parameters_are_refused_before_device_work(call, who):
    _refused(call(FAKE, C.byref(_params(mode=5))), who, "yuv_mode")
    _refused(call(FAKE, C.byref(_params(mode=-1))), who, "yuv_mode")
    _refused(call(FAKE, C.byref(_params(method=9))), who, "method")
    _refused(call(FAKE, C.byref(_params(method=-1))), who, "method")
    _refused(call(FAKE, C.byref(_params(mode=sj.YUV_AUTO)), fmt=sj.SRC_GRAY), who, "SJPEG_YUV_AUTO", "RGB")
    _refused(call(FAKE, C.byref(_params(mode=sj.YUV_SHARP)), fmt=sj.SRC_YUV420), who, "SJPEG_YUV_SHARP", "RGB")
    _refused(call(FAKE, C.byref(_params(search=_search(mode=3), per_frame=1))), who, "search[1]", "frame 1", "target_mode")
    _refused(call(FAKE, C.byref(_params(search=_search(value=float("nan")), per_frame=1))), who, "frame 1", "not finite")
    _refused(call(FAKE, C.byref(_params(search=_search(value=float("inf")), per_frame=1))), who, "frame 1", "not finite")
    # the frames' own checks name the frame
    _refused(call(FAKE, C.byref(_params()), frames=_frame(plane=None)), who, "frame 0", "null plane")
    _refused(call(FAKE, C.byref(_params()), frames=_frame(w=0)), who, "frame 0", "dimensions")


def test_engine_methods_and_keywords_exist():
    import inspect
    for name in ("encode_ragged_full", "encode_ragged_full_packed", "search_stats"):
        assert callable(getattr(sj.Engine, name))
    sig = inspect.signature(sj.encode_images_full).parameters
    want = dict(quality=75.0, yuv_mode=sj.YUV_AUTO, method=4, use_trellis=False, target_size=None, target_psnr=None,
                passes=10, tolerance=1.0, qmin=0.0, qmax=100.0, min_quant=None, q_bias=0x78, dmax_luma=12, dmax_chroma=1,
                engine=None, packed=False)
    assert list(sig)[0] == "images" and list(sig)[1:] == list(want)
    for k, v in want.items():
        assert sig[k].default == v or sig[k].default is v, k


def test_encode_images_full_checks_its_arguments():
    img = [np.zeros((8, 8, 3), np.uint8)]
    before = sj.packed_stats()
    for packed in (False, True):
        with pytest.raises(sj.SjpegError, match="not a CUDA tensor"):
            sj.encode_images_full(img, packed=packed)
        with pytest.raises(sj.SjpegError, match="not a CUDA tensor"):
            sj.encode_images_full(img, method=4, use_trellis=True, target_size=1000, packed=packed)
        with pytest.raises(sj.SjpegError, match="not both"):
            sj.encode_images_full(img, target_size=1000, target_psnr=40.0, packed=packed)
        with pytest.raises(sj.SjpegError, match="no images"):
            sj.encode_images_full([], packed=packed)
        with pytest.raises(sj.SjpegError, match="method"):
            sj.encode_images_full(img, method=9, packed=packed)
    assert sj.packed_stats() == before


def test_the_old_refusals_are_still_in_force():
    img = [np.zeros((8, 8, 3), np.uint8)]
    with pytest.raises(sj.SjpegError, match="trellis"):
        sj.encode_images(img, method=7, target_size=1000)
    with pytest.raises(sj.SjpegError, match="trellis"):
        sj.encode_images(img, method=4, use_trellis=True, target_size=1000)
    with pytest.raises(sj.SjpegError, match="YUV_AUTO"):
        sj.encode_images(img, yuv_mode=sj.YUV_AUTO, target_size=1000)
    # the C entry points too: sjpeg_hip_encode_ragged_search_src keeps methods 0..6
    q = np.ones((1, 2, 64), np.uint8)
    sp = sj.SearchParams(1, 1000.0, 5, 1.0, 0.0, 100.0)
    rc = sj.lib().sjpeg_hip_encode_ragged_search_src(FAKE, sj.SRC_RGB, sj.YUV_420, 1, _frame(), q.ctypes.data, 0, None, 0x78,
                                                     7, 12, 1, C.byref(sp), 0, None, None, 1 << 16, 1 << 12, None)
    _refused(rc, "sjpeg_hip_encode_ragged_search_src", "methods 0..6")
