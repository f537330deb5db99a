"""The ragged search (sjpeg_hip_encode_ragged_search_src and its two measurement passes) without a GPU: the entry points
are declared, exported and bound, sjpeg_hip_search has its C layout, and bad arguments are refused with EINVAL before
any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sjpeg_amd as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sjpeg_hip_scan_quant_error_ragged_src", "sjpeg_hip_scan_counted_bits_ragged_src",
         "sjpeg_hip_encode_ragged_search_src"]
EINVAL = -1


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound(name):
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    assert re.search(r"\b%s\s*\(" % name, text)
    assert name in sj.EXPORTED_C_SYMBOLS
    fn = getattr(sj.lib(), name)
    assert fn.restype is C.c_int and fn.argtypes is not None


def test_search_struct_layout():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    assert "typedef struct sjpeg_hip_search" in text
    assert C.sizeof(sj.SearchParams) == 24
    offsets = [getattr(sj.SearchParams, f).offset for f in ("target_mode", "target_value", "passes", "tolerance",
                                                             "qmin", "qmax")]
    assert offsets == [0, 4, 8, 12, 16, 20]


def test_abi_version_unchanged():
    assert sj.lib().sjpeg_hip_abi_version() == 18


def _frame():
    f = (sj.RaggedFrame * 1)()
    f[0].plane[0] = 4096                 # (never read: every refusal comes before device work)
    f[0].width = f[0].height = 16
    f[0].row_stride[0] = 48
    f[0].out_capacity = 4096
    return f


class _Call:
    """One sjpeg_hip_encode_ragged_search_src call with good arguments unless told otherwise.  The engine handle is a
    dummy address: the checks must refuse before they touch it."""

    def __init__(self):
        self.q = np.ones((1, 2, 64), np.uint8)
        self.sizes = (C.c_uint64 * 1)()
        self.out = (C.c_uint8 * 16)()

    def __call__(self, engine=C.c_void_p(8), search=(1, 2000.0, 10, 1.0, 0.0, 100.0), method=4, yuv_mode=sj.YUV_420):
        sp = None if search is None else C.pointer(sj.SearchParams(*search))
        return sj.lib().sjpeg_hip_encode_ragged_search_src(engine, sj.SRC_RGB, yuv_mode, 1, _frame(), self.q.ctypes.data,
                                                           0, None, 0x78, method, 12, 1, sp, 0, None, None,
                                                           C.cast(self.out, C.c_void_p), C.cast(self.sizes, C.c_void_p),
                                                           None)


def _einval(rc, word):
    assert rc == EINVAL
    assert word in sj.lib().sjpeg_hip_last_error().decode()


def test_search_refusals():
    call = _Call()
    _einval(call(engine=None), "engine")
    _einval(call(search=None), "search")
    _einval(call(search=(0, 2000.0, 10, 1.0, 0.0, 100.0)), "target_mode")
    _einval(call(search=(3, 2000.0, 10, 1.0, 0.0, 100.0)), "target_mode")
    _einval(call(search=(1, float("inf"), 10, 1.0, 0.0, 100.0)), "finite")
    _einval(call(search=(2, float("nan"), 10, 1.0, 0.0, 100.0)), "finite")
    _einval(call(method=7), "method")
    _einval(call(yuv_mode=sj.YUV_AUTO), "yuv_mode")


def test_measurement_refusals():
    L = sj.lib()
    buf = (C.c_uint64 * 1)()
    t = sj.make_tables(quality=75.0)[0]
    for fn in (L.sjpeg_hip_scan_quant_error_ragged_src, L.sjpeg_hip_scan_counted_bits_ragged_src):
        _einval(fn(None, sj.SRC_RGB, sj.YUV_420, 1, _frame(), C.cast(C.pointer(t), C.c_void_p), 0,
                   C.cast(buf, C.c_void_p), None), "engine")
        _einval(fn(C.c_void_p(8), sj.SRC_RGB, sj.YUV_420, 1, _frame(), None, 0, C.cast(buf, C.c_void_p), None),
                "tables")
        t.flags = 1                      # SJPEG_HIP_QUANT_TRELLIS
        _einval(fn(C.c_void_p(8), sj.SRC_RGB, sj.YUV_420, 1, _frame(), C.cast(C.pointer(t), C.c_void_p), 0,
                   C.cast(buf, C.c_void_p), None), "trellis")
        t.flags = 0


def test_encode_images_target_checks_before_device_work():
    img = [np.zeros((8, 8, 3), np.uint8)]
    with pytest.raises(sj.SjpegError, match="not both"):
        sj.encode_images(img, target_size=1000, target_psnr=40.0)
    with pytest.raises(sj.SjpegError, match="trellis"):
        sj.encode_images(img, method=7, target_size=1000)
    with pytest.raises(sj.SjpegError, match="YUV_AUTO"):
        sj.encode_images(img, yuv_mode=sj.YUV_AUTO, method=4, target_psnr=40.0)
    with pytest.raises(sj.SjpegError, match="YUV_AUTO"):
        sj.encode_images(img, yuv_mode=sj.YUV_SHARP, method=4, target_size=1000)


def test_search_hook_program_compiles_and_links(tmp_path):
    """CPU: the program the GPU test compares q / value with builds against the public header and the library."""
    import subprocess
    exe = str(tmp_path / "search_hook_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "search_hook_test.cc"), "-o", exe, "-L", sj.CSRC,
                           "-lsjpeg_amd", "-lpthread", "-Wl,-rpath," + sj.CSRC, "-Wl,-rpath-link,/opt/rocm/lib"])
