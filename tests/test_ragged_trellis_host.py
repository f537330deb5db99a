"""Ragged batches with trellis quantization (sjpeg_hip_encode_ragged_trellis_src, methods 7 and 8) without a GPU: the
entry point is declared, exported and refuses a NULL engine, and encode_images / compress_images check use_trellis
before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sjpeg_amd as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sjpeg_hip_encode_ragged_trellis_src"


def test_declared_exported_and_in_the_library():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert NAME in sj.EXPORTED_C_SYMBOLS
    assert hasattr(sj.lib(), NAME)


def test_argument_types():
    fn = getattr(sj.lib(), NAME)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(sj.RaggedFrame),
                                 C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def test_abi_version_unchanged():
    assert sj.lib().sjpeg_hip_abi_version() == 18
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    assert re.search(r"#define\s+SJPEG_HIP_ABI_VERSION\s+18\b", text)


def _frame(w=16, h=16):
    f = (sj.RaggedFrame * 1)()
    f[0].width, f[0].height = w, h
    f[0].row_stride[0] = 3 * w
    f[0].out_capacity = 4096
    return f


@pytest.mark.parametrize("mode", [sj.YUV_AUTO, sj.YUV_420, sj.YUV_SHARP, sj.YUV_444, sj.YUV_400])
@pytest.mark.parametrize("method", [7, 8])
def test_null_engine_is_refused(mode, method):
    buf = (C.c_uint64 * 64)()
    q = np.ones((1, 2, 64), np.uint8)
    modes = (C.c_int * 1)()
    rc = getattr(sj.lib(), NAME)(None, sj.SRC_RGB, mode, 1, _frame(), q.ctypes.data, 0, None, 0x78, method, 12, 1,
                                 C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), modes, None)
    assert rc != 0
    assert "engine" in sj.lib().sjpeg_hip_last_error().decode()


def test_engine_method_exists():
    assert callable(getattr(sj.Engine, "encode_ragged_trellis"))


def test_trellis_with_a_target_is_refused_before_device_work():
    img = [np.zeros((8, 8, 3), np.uint8)]
    with pytest.raises(sj.SjpegError, match="trellis"):
        sj.encode_images(img, method=4, use_trellis=True, target_size=1000)
    with pytest.raises(sj.SjpegError, match="trellis"):
        sj.encode_images(img, method=6, use_trellis=True, target_psnr=40.0)
    with pytest.raises(sj.SjpegError, match="trellis"):
        sj.encode_images(img, method=1, use_trellis=True, target_size=1000)


def test_trellis_auto_refuses_non_rgb_layout_before_device_work():
    with pytest.raises(sj.SjpegError, match="RGB pictures"):
        sj.encode_images([np.zeros((8, 8, 4), np.uint8)], yuv_mode=sj.YUV_AUTO, method=4, use_trellis=True)
    with pytest.raises(sj.SjpegError, match="RGB pictures"):
        sj.compress_images([np.zeros((8, 8, 4), np.uint8)], use_trellis=True)


@pytest.mark.parametrize("method", [7, 8])
def test_method_without_the_keyword_is_refused_as_before(method):
    with pytest.raises(sj.SjpegError, match="host API"):
        sj.encode_images([np.zeros((8, 8, 3), np.uint8)], method=method)


def test_pictures_are_checked_before_device_work():
    with pytest.raises(sj.SjpegError, match="not a CUDA tensor"):
        sj.encode_images([np.zeros((8, 8, 3), np.uint8)], method=4, use_trellis=True)
