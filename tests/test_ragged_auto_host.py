"""Ragged batches with SJPEG_YUV_AUTO and the sharp conversion, without a GPU: the new entry points are declared and
exported and refuse a NULL engine, sjpeg_hip_riskiness_verdict is SjpegRiskiness' arithmetic, and encode_images /
compress_images check their arguments before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sjpeg_amd as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sjpeg_hip_riskiness_ragged_src", "sjpeg_hip_riskiness_verdict", "sjpeg_hip_sharp_ragged_workspace",
         "sjpeg_hip_sharp_yuv_ragged", "sjpeg_hip_encode_ragged_auto_src"]


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_in_the_library(name):
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    assert re.search(r"\b%s\s*\(" % name, text)
    assert name in sj.EXPORTED_C_SYMBOLS
    assert hasattr(sj.lib(), name)


def test_abi_version_unchanged():
    assert sj.lib().sjpeg_hip_abi_version() == 18


def _frame(w=16, h=16):
    f = (sj.RaggedFrame * 1)()
    f[0].width, f[0].height = w, h
    f[0].row_stride[0] = 3 * w
    f[0].out_capacity = 4096
    return f


def _refused(rc):
    assert rc != 0
    assert "engine" in sj.lib().sjpeg_hip_last_error().decode()


def test_null_engine_is_refused():
    L = sj.lib()
    buf = (C.c_uint64 * 64)()
    _refused(L.sjpeg_hip_riskiness_ragged_src(None, sj.SRC_RGB, 1, _frame(), C.cast(buf, C.c_void_p),
                                              C.cast(buf, C.c_void_p), None))
    ptrs = (C.c_void_p * 1)(C.addressof(buf))
    _refused(L.sjpeg_hip_sharp_yuv_ragged(None, sj.SRC_RGB, 1, _frame(), ptrs, ptrs, ptrs, C.cast(buf, C.c_void_p),
                                          1 << 20, None))
    q = np.ones((1, 2, 64), np.uint8)
    modes = (C.c_int * 1)()
    for mode in (sj.YUV_AUTO, sj.YUV_SHARP, sj.YUV_420):
        _refused(L.sjpeg_hip_encode_ragged_auto_src(None, sj.SRC_RGB, mode, 1, _frame(), q.ctypes.data, 0, None, 0x78,
                                                    4, 12, 1, C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p),
                                                    modes, None))


def test_sharp_ragged_workspace():
    L = sj.lib()
    frames = (sj.RaggedFrame * 3)()
    for k, (w, h) in enumerate([(3, 9), (640, 480), (1921, 7)]):
        frames[k].width, frames[k].height = w, h
    big = L.sjpeg_hip_sharp_ragged_workspace(3, frames)
    # at least what the uniform call asks for each of the frames that are converted iteratively
    assert big >= sj.lib().sjpeg_hip_sharp_workspace(640, 480, 1) + sj.lib().sjpeg_hip_sharp_workspace(1921, 7, 1) - 8192
    assert L.sjpeg_hip_sharp_ragged_workspace(1, frames) > 0            # (3x9: tables and a descriptor only)
    frames[0].width = 0
    assert L.sjpeg_hip_sharp_ragged_workspace(3, frames) == 0
    assert L.sjpeg_hip_sharp_ragged_workspace(0, frames) == 0


def _verdict_py(s, w, h):
    """src/jpeg_tools.cc:212-236 in Python (double arithmetic, as RiskVerdict)."""
    count, gray = float(s[1]), float(s[2])
    total = s[0] / count if count > 0 else 0.0
    num = (w - 1.0) * (h - 1.0)
    if num > 0:
        gray /= num
    frac = 100.0 * count / (float(w) * h)
    if frac < 1.0:
        total = 0.0
    total = 100.0 if total > 25.0 else total * 100.0 / 25.0
    mode = sj.YUV_400 if gray > 0.995 else sj.YUV_420 if total < 40.0 else sj.YUV_SHARP if total < 70.0 else sj.YUV_444
    return mode, float(np.float32(total))


@pytest.mark.parametrize("sums,w,h", [
    ((0, 0, 0), 1, 1), ((500, 10, 0), 1, 300), ((500, 10, 0), 300, 1),     # W or H = 1: no positions
    ((99 * 20, 99, 0), 100, 100),                 # frac 0.99 % < 1 %: score 0 -> 4:2:0
    ((100 * 20, 100, 0), 100, 100),               # frac exactly 1 %: score 20 * 4 = 80 -> 4:4:4
    ((100 * 26, 100, 0), 100, 100),               # above 25: clamped to 100
    ((100 * 25, 100, 0), 100, 100),               # exactly 25: 100, not clamped
    ((1000 * 10, 1000, 0), 100, 100),             # 40 exactly -> sharp
    ((1000 * 9, 1000, 0), 100, 100),              # 36 -> 4:2:0
    ((10000 * 175, 10000 * 10, 0), 100, 100),     # 17.5 -> 70 exactly -> 4:4:4
    ((10000 * 174, 10000 * 10, 0), 100, 100),     # 69.6 -> sharp
    ((0, 0, 9752), 100, 100),                     # gray 9752 / 9801 = 0.995 -> not gray
    ((0, 0, 9753), 100, 100),                     # 0.99510 > 0.995 -> 4:0:0
    ((100 * 26, 100, 9801), 100, 100),            # gray wins over the score
])
def test_verdict_follows_risk_verdict(sums, w, h):
    got = sj.riskiness_verdict(sums, w, h)
    want = _verdict_py(sums, w, h)
    assert got[0] == want[0], (sums, w, h, got, want)
    assert got[1] == pytest.approx(want[1], abs=1e-4)


def test_verdict_refuses_bad_dimensions():
    assert sj.riskiness_verdict((1, 1, 1), 0, 5) == (sj.YUV_AUTO, -1.0)


@pytest.mark.parametrize("method", [7, 8])
def test_trellis_refused_before_device_work(method):
    with pytest.raises(sj.SjpegError, match="host API"):
        sj.encode_images([np.zeros((8, 8, 3), np.uint8)], yuv_mode=sj.YUV_AUTO, method=method)
    with pytest.raises(sj.SjpegError, match="host API"):
        sj.encode_images([np.zeros((8, 8, 3), np.uint8)], yuv_mode=sj.YUV_SHARP, method=method)


@pytest.mark.parametrize("mode", [sj.YUV_AUTO, sj.YUV_SHARP])
def test_auto_refuses_non_rgb_layout_before_device_work(mode):
    with pytest.raises(sj.SjpegError, match="RGB pictures"):
        sj.encode_images([np.zeros((8, 8, 4), np.uint8)], yuv_mode=mode, method=4)
    with pytest.raises(sj.SjpegError, match="RGB pictures"):
        sj.encode_images([np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.uint8)], yuv_mode=mode)
    with pytest.raises(sj.SjpegError, match="RGB pictures"):
        sj.compress_images([np.zeros((8, 8, 4), np.uint8)])


def test_yuv_mode_range():
    with pytest.raises(sj.SjpegError, match="0..4"):
        sj.encode_images([np.zeros((8, 8, 3), np.uint8)], yuv_mode=5, method=4)
