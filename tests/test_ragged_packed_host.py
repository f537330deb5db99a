"""Ragged batches into one packed buffer (sjpeg_hip_encode_ragged_packed_src) without a GPU: the entry point is declared,
exported and in the library, its argument checks come before any device work, the Python params structure has the C
layout, and encode_images / compress_images check their arguments before the packed path starts."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sjpeg_amd as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sjpeg_hip_encode_ragged_packed_src"
EINVAL = -1


def _header():
    return open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()


def test_declared_exported_and_in_the_library():
    text = _header()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert re.search(r"\}\s*sjpeg_hip_ragged_params\s*;", text)
    assert NAME in sj.EXPORTED_C_SYMBOLS
    assert hasattr(sj.lib(), NAME)


def test_argument_types():
    fn = getattr(sj.lib(), NAME)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_int, C.c_int, C.POINTER(sj.RaggedFrame), C.POINTER(sj.RaggedParams),
                                 C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                 C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p]


def test_abi_version_unchanged():
    assert sj.lib().sjpeg_hip_abi_version() == 18
    assert re.search(r"#define\s+SJPEG_HIP_ABI_VERSION\s+18\b", _header())


def test_einval_is_minus_one():
    assert re.search(r"SJPEG_HIP_EINVAL\s*=?\s*\(?-1\)?", _header())


def test_params_structure_has_the_c_layout(tmp_path):
    exe = str(tmp_path / "ragged_params_size")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "ragged_params_size.cc"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    P = sj.RaggedParams
    assert got == [C.sizeof(P), P.quant.offset, P.quant_per_frame.offset, P.min_quant.offset, P.q_bias.offset,
                   P.search.offset, P.search_per_frame.offset]


def _frame(w=16, h=16):
    f = (sj.RaggedFrame * 1)()
    f[0].width, f[0].height = w, h
    f[0].row_stride[0] = 3 * w
    f[0].out_capacity = 4096
    return f


def _call(engine, params, d_packed, d_offsets, d_sizes=1 << 12, nframes=1):
    modes, q, v = (C.c_int * 1)(), (C.c_float * 1)(), (C.c_float * 1)()
    return getattr(sj.lib(), NAME)(engine, sj.SRC_RGB, nframes, _frame(), params, d_packed, 1 << 20, d_offsets, d_sizes,
                                   modes, q, v, None)


def _params(mode=sj.YUV_420, method=4):
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, method, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    p._keep = q
    return p


def _refused(rc, *words):
    assert rc == EINVAL
    msg = sj.lib().sjpeg_hip_last_error().decode()
    assert NAME in msg
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("mode,method", [(sj.YUV_AUTO, 4), (sj.YUV_420, 0), (sj.YUV_SHARP, 6), (sj.YUV_444, 7)])
def test_null_engine_is_refused(mode, method):
    _refused(_call(None, C.byref(_params(mode, method)), 1 << 16, 1 << 14), "engine")


def test_null_params_offsets_and_misaligned_pool_are_refused():
    # (the checks come before the engine is touched: any non-NULL value stands in for one)
    fake = C.c_void_p(1 << 20)
    _refused(_call(fake, None, 1 << 16, 1 << 14), "params")
    _refused(_call(fake, C.byref(_params()), 1 << 16, None), "d_offsets")
    _refused(_call(fake, C.byref(_params()), None, 1 << 14), "d_packed")
    _refused(_call(fake, C.byref(_params()), (1 << 16) + 8, 1 << 14), "multiple of 16")
    _refused(_call(fake, C.byref(_params()), 1 << 16, 1 << 14, nframes=0), "nframes")
    _refused(_call(fake, C.byref(_params()), 1 << 16, 1 << 14, nframes=65536), "nframes")


def test_engine_method_and_keywords_exist():
    import inspect
    assert callable(getattr(sj.Engine, "encode_ragged_packed"))
    sig = inspect.signature(sj.Engine.encode_ragged_packed)
    for name in ("search", "capacities", "packed_capacity", "out"):
        assert name in sig.parameters
    assert inspect.signature(sj.encode_images).parameters["packed"].default is False
    assert inspect.signature(sj.compress_images).parameters["packed"].default is False
    assert set(sj.packed_stats()) == {"calls", "retries"}


def test_packed_checks_its_arguments_before_device_work():
    img = [np.zeros((8, 8, 3), np.uint8)]
    before = sj.packed_stats()
    with pytest.raises(sj.SjpegError, match="not a CUDA tensor"):
        sj.encode_images(img, packed=True)
    with pytest.raises(sj.SjpegError, match="not a CUDA tensor"):
        sj.compress_images(img, packed=True)
    with pytest.raises(sj.SjpegError, match="not both"):
        sj.encode_images(img, target_size=1000, target_psnr=40.0, packed=True)
    with pytest.raises(sj.SjpegError, match="trellis"):
        sj.encode_images(img, method=4, use_trellis=True, target_size=1000, packed=True)
    with pytest.raises(sj.SjpegError, match="YUV_AUTO"):
        sj.encode_images(img, yuv_mode=sj.YUV_AUTO, target_size=1000, packed=True)
    with pytest.raises(sj.SjpegError, match="host API"):
        sj.encode_images(img, method=7, packed=True)
    with pytest.raises(sj.SjpegError, match="RGB pictures"):
        sj.compress_images([np.zeros((8, 8, 4), np.uint8)], packed=True)
    with pytest.raises(sj.SjpegError, match="no images"):
        sj.encode_images([], packed=True)
    assert sj.packed_stats() == before


def test_first_pool():
    # per picture 2048 bytes of header allowance plus half a byte per sample, rounded up to 16; 64 KiB at least
    assert sj._first_pool([(8, 8)], sj.YUV_420) == 65536
    assert sj._first_pool([(1000, 1000)] * 2, sj.YUV_444) == 2 * (2048 + 1500000)
    assert sj._first_pool([(1000, 1000)], sj.YUV_420) == 2048 + 750000
    assert sj._first_pool([(1000, 1000)], sj.YUV_400) == 2048 + 500000
    assert sj._first_pool([(1001, 999)], sj.YUV_AUTO) == (2048 + (3 * 1001 * 999) // 2 + 15) & ~15
