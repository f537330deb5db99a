"""Ragged batches with the reference's analysis (methods 0..6) without a GPU: the three entry points are declared and
exported, refuse a NULL engine, and encode_images checks `method` and its qualities before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sjpeg_amd as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sjpeg_hip_scan_histogram_ragged_src", "sjpeg_hip_scan_symbol_stats_ragged_src",
         "sjpeg_hip_encode_ragged_batch_src"]


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_in_the_library(name):
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    assert re.search(r"\b%s\s*\(" % name, text)
    assert name in sj.EXPORTED_C_SYMBOLS
    assert hasattr(sj.lib(), name)


def test_abi_version_unchanged():
    assert sj.lib().sjpeg_hip_abi_version() == 18


def _frame():
    f = (sj.RaggedFrame * 1)()
    f[0].width = f[0].height = 16
    f[0].row_stride[0] = 48
    f[0].out_capacity = 4096
    return f


def _refused(rc):
    assert rc != 0
    assert "engine" in sj.lib().sjpeg_hip_last_error().decode()


def test_null_engine_is_refused():
    L = sj.lib()
    buf = (C.c_uint32 * (2 * 64 * 128))()
    _refused(L.sjpeg_hip_scan_histogram_ragged_src(None, sj.SRC_RGB, sj.YUV_420, 1, _frame(), C.cast(buf, C.c_void_p),
                                                   None))
    t = sj.make_tables(quality=75.0)[0]
    _refused(L.sjpeg_hip_scan_symbol_stats_ragged_src(None, sj.SRC_RGB, sj.YUV_420, 1, _frame(),
                                                      C.cast(C.pointer(t), C.c_void_p), 0, C.cast(buf, C.c_void_p),
                                                      None))
    q = np.ones((1, 2, 64), np.uint8)
    sizes = (C.c_uint64 * 1)()
    _refused(L.sjpeg_hip_encode_ragged_batch_src(None, sj.SRC_RGB, sj.YUV_420, 1, _frame(), q.ctypes.data, 0, None,
                                                 0x78, 4, 12, 1, C.cast(buf, C.c_void_p), C.cast(sizes, C.c_void_p),
                                                 None))


@pytest.mark.parametrize("method", [7, 8])
def test_encode_images_refuses_trellis_before_device_work(method):
    # (numpy pictures: any device work would fail on them with another message)
    with pytest.raises(sj.SjpegError, match="host API"):
        sj.encode_images([np.zeros((8, 8, 3), np.uint8)], method=method)


def test_encode_images_quality_list_length():
    with pytest.raises(sj.SjpegError, match="one quality per image"):
        sj.encode_images([np.zeros((8, 8, 3), np.uint8)] * 3, quality=[50.0, 75.0], method=4)
    with pytest.raises(sj.SjpegError, match="one quality per image"):
        sj.encode_images([np.zeros((8, 8, 3), np.uint8)] * 2, quality=[50.0, 75.0, 90.0])
