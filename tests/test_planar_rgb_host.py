"""Planar RGB (SJPEG_HIP_SRC_RGB_PLANAR) without a GPU: the enum value is in the header and in Python, the ABI version
stays 18, the one-pitch rule and the null-plane check of the ragged entry points come before any device work and name
the frame, and the layout keyword checks its arguments."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import sjpeg_amd as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = "sjpeg_hip_encode_ragged_full_src"
RAGGED = "sjpeg_hip_encode_ragged_src"
EINVAL = -1
FAKE = C.c_void_p(1 << 20)          # (the checks come before the engine is touched: any non-NULL value stands in for one)


def test_enum_value_and_abi_version():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    assert re.search(r"\bSJPEG_HIP_SRC_RGB_PLANAR\s*=\s*8\b", text)
    assert sj.SRC_RGB_PLANAR == 8
    assert "row_stride[1]" in text and "frame_stride[1]" in text        # the rule stands next to the enum
    assert sj.lib().sjpeg_hip_abi_version() == 18
    assert re.search(r"#define\s+SJPEG_HIP_ABI_VERSION\s+18\b", text)


def _frames(w=16, h=16, strides=(24, 24, 24), planes=(1 << 24, 2 << 24, 3 << 24), bad=1):
    """Two frames; frame `bad` gets the strides and planes given, the other one is in order."""
    f = (sj.RaggedFrame * 2)()
    for k in range(2):
        f[k].width, f[k].height = w, h
        for i in range(3):
            f[k].plane[i] = planes[i] if k == bad else (i + 1) << 24
            f[k].row_stride[i] = strides[i] if k == bad else 24
        f[k].out_offset = 4096 * k
        f[k].out_capacity = 4096
    return f


def _params(mode=sj.YUV_420, method=4):
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, method, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    p._keep = q
    return p


def _full(frames, mode=sj.YUV_420):
    p = _params(mode)
    return getattr(sj.lib(), FULL)(FAKE, sj.SRC_RGB_PLANAR, 2, frames, C.byref(p), 1 << 16, 1 << 12, None, None, None, None)


def _ragged(frames, mode=sj.YUV_420):
    tables, _ = sj.make_tables(quality=75.0)
    tarr = (sj.ScanTables * 1)(tables)
    return getattr(sj.lib(), RAGGED)(FAKE, sj.SRC_RGB_PLANAR, mode, 2, frames, C.cast(tarr, C.c_void_p), 0, None, None, 1,
                                     C.c_void_p(1 << 16), C.c_void_p(1 << 12), None)


def _refused(rc, who, *words):
    assert rc == EINVAL
    msg = sj.lib().sjpeg_hip_last_error().decode()
    assert who in msg
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("call,who", [(_full, FULL), (_ragged, RAGGED)])
def test_the_one_pitch_rule_comes_before_device_work(call, who):
    _refused(call(_frames(strides=(24, 32, 24))), who, "frame 1", "row_stride[1]", "row_stride[0]")
    _refused(call(_frames(strides=(24, 24, -24))), who, "frame 1", "row_stride[2]", "row_stride[0]")
    _refused(call(_frames(strides=(24, 32, 24), bad=0)), who, "frame 0", "row_stride[1]")
    _refused(call(_frames(planes=(1 << 24, None, 3 << 24))), who, "frame 1", "null plane")
    _refused(call(_frames(planes=(1 << 24, 2 << 24, None), bad=0)), who, "frame 0", "null plane")
    _refused(call(_frames(strides=(15, 15, 15))), who, "frame 1", "row_stride")
    _refused(call(_frames(strides=(-15, -15, -15))), who, "frame 1", "row_stride")
    # every sampling takes the layout: the same refusal, not "yuv_mode does not match"
    for mode in (sj.YUV_444, sj.YUV_400):
        _refused(call(_frames(strides=(24, 32, 24)), mode), who, "frame 1", "row_stride[1]")


def test_auto_and_sharp_admit_the_layout():
    # (SJPEG_YUV_AUTO / SHARP refuse anything but RGB sources by name; planar RGB gets as far as its frames' checks)
    for mode in (sj.YUV_AUTO, sj.YUV_SHARP):
        _refused(_full(_frames(strides=(24, 24, 40)), mode), FULL, "frame 1", "row_stride[2]")


def test_layout_keyword():
    for fn in (sj.encode_images, sj.compress_images, sj.riskiness_images):
        sig = inspect.signature(fn).parameters
        assert list(sig)[-1] == "layout" and sig["layout"].default == "hwc", fn.__name__
    # (encode_images_full's parameter list is pinned by tests/test_ragged_full_host.py: its channel-first twin)
    assert list(inspect.signature(sj.encode_images_full_chw).parameters) == list(inspect.signature(sj.encode_images_full).parameters)
    assert "layout" not in inspect.signature(sj.Engine.encode_frames).parameters
    chw = [np.zeros((3, 8, 8), np.uint8)]
    hwc = [np.zeros((8, 8, 3), np.uint8)]
    before = sj.packed_stats()
    with pytest.raises(sj.SjpegError, match="image 0 is not a CUDA tensor"):
        sj.encode_images_full_chw(chw)
    with pytest.raises(sj.SjpegError, match="not both"):
        sj.encode_images_full_chw(chw, target_size=1000, target_psnr=40.0)
    for fn in (sj.encode_images, sj.compress_images, sj.riskiness_images):
        with pytest.raises(sj.SjpegError, match="nchw"):
            fn(chw, layout="nchw")
        with pytest.raises(sj.SjpegError, match="layout"):
            fn(chw, layout=None)
        with pytest.raises(sj.SjpegError, match="image 0 is not a CUDA tensor"):
            fn(chw, layout="chw")
    for packed in (False, True):
        with pytest.raises(sj.SjpegError, match="not a CUDA tensor"):
            sj.encode_images(chw, yuv_mode=sj.YUV_AUTO, packed=packed, layout="chw")
        with pytest.raises(sj.SjpegError, match="no images"):
            sj.encode_images([], packed=packed, layout="chw")
    # the default layout keeps its checks and messages
    with pytest.raises(sj.SjpegError, match="image 0 is not a CUDA tensor"):
        sj.encode_images(hwc)
    with pytest.raises(sj.SjpegError, match=r"\[H, W, 3\]"):
        sj.encode_images(chw, yuv_mode=sj.YUV_AUTO)
    assert sj.packed_stats() == before
