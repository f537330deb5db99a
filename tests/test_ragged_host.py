"""Ragged batches without a GPU: the entry point is declared and exported, refuses a NULL engine, and encode_images
checks its arguments before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sjpeg_amd as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ragged_symbol_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    assert re.search(r"\bsjpeg_hip_encode_ragged_src\s*\(", text)
    assert "sjpeg_hip_ragged_frame" in text
    assert "sjpeg_hip_encode_ragged_src" in sj.EXPORTED_C_SYMBOLS
    assert hasattr(sj.lib(), "sjpeg_hip_encode_ragged_src")
    assert sj.lib().sjpeg_hip_abi_version() == 18


def test_ragged_frame_layout():
    # the ctypes mirror of sjpeg_hip_ragged_frame: 3 pointers, 3 row strides, width, height, offset, capacity
    assert C.sizeof(sj.RaggedFrame) == 3 * 8 + 3 * 8 + 4 + 4 + 8 + 8
    assert sj.RaggedFrame.out_offset.offset == 56


def test_null_engine_is_refused():
    f = (sj.RaggedFrame * 1)()
    f[0].width = f[0].height = 16
    t = sj.make_tables(quality=75.0)[0]
    sizes = (C.c_uint64 * 1)()
    out = (C.c_uint8 * 16)()
    rc = sj.lib().sjpeg_hip_encode_ragged_src(None, sj.SRC_RGB, sj.YUV_420, 1, f, C.cast(C.pointer(t), C.c_void_p), 0,
                                              None, None, 1, C.cast(out, C.c_void_p), C.cast(sizes, C.c_void_p), None)
    assert rc != 0
    assert "engine" in sj.lib().sjpeg_hip_last_error().decode()


def test_encode_images_checks_before_device_work():
    torch = pytest.importorskip("torch")
    with pytest.raises(sj.SjpegError, match="no images"):
        sj.encode_images([])
    with pytest.raises(sj.SjpegError, match="not a CUDA tensor"):
        sj.encode_images([torch.zeros((8, 8, 3), dtype=torch.uint8)])
    with pytest.raises(sj.SjpegError, match="not a CUDA tensor"):
        sj.encode_images([np.zeros((8, 8, 3), np.uint8)])
    with pytest.raises(sj.SjpegError, match="not a CUDA tensor"):
        sj.encode_images([torch.zeros((8, 8, 3), dtype=torch.float32), torch.zeros((8, 8, 3), dtype=torch.uint8)])
