"""Float channel-first pictures (SJPEG_HIP_SRC_RGB_PLANAR_F32 / _F16 / _BF16) without a GPU: the enum values are in
the header and in Python, the ABI version stays 18, the element-size rules of the ragged entry points come before any
device work and name the frame, the pixel transform refuses non-finite values, the two calls without an engine refuse
the formats by name, FloatPixels checks its arguments, and the pinned signatures are what they were."""
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
F32, F16, BF16 = 9, 10, 11


def test_enum_values_and_abi_version():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    for name, value in (("F32", 9), ("F16", 10), ("BF16", 11)):
        assert re.search(r"\bSJPEG_HIP_SRC_RGB_PLANAR_%s\s*=\s*%d\b" % (name, value), text)
        assert getattr(sj, "SRC_RGB_PLANAR_" + name) == value
    assert "fmaf" in text and "sjpeg_hip_engine_set_pixel_transform" in text
    assert sj.lib().sjpeg_hip_abi_version() == 18
    assert re.search(r"#define\s+SJPEG_HIP_ABI_VERSION\s+18\b", text)
    for name in ("sjpeg_hip_engine_set_pixel_transform", "sjpeg_hip_engine_get_pixel_transform"):
        assert name in sj.EXPORTED_C_SYMBOLS
        getattr(sj.lib(), name)


def _frames(w=16, h=16, strides=(64, 64, 64), planes=(1 << 24, 2 << 24, 3 << 24), bad=1):
    """Two frames; frame `bad` gets the strides and planes given, the other one is in order (for any element size)."""
    f = (sj.RaggedFrame * 2)()
    for k in range(2):
        f[k].width, f[k].height = w, h
        for i in range(3):
            f[k].plane[i] = planes[i] if k == bad else (i + 1) << 24
            f[k].row_stride[i] = strides[i] if k == bad else 64
        f[k].out_offset = 4096 * k
        f[k].out_capacity = 4096
    return f


def _params(mode=sj.YUV_420, method=4):
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, method, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    p._keep = q
    return p


def _full(frames, fmt, mode=sj.YUV_420):
    p = _params(mode)
    return getattr(sj.lib(), FULL)(FAKE, fmt, 2, frames, C.byref(p), 1 << 16, 1 << 12, None, None, None, None)


def _ragged(frames, fmt, mode=sj.YUV_420):
    tables, _ = sj.make_tables(quality=75.0)
    tarr = (sj.ScanTables * 1)(tables)
    return getattr(sj.lib(), RAGGED)(FAKE, fmt, mode, 2, frames, C.cast(tarr, C.c_void_p), 0, None, None, 1,
                                     C.c_void_p(1 << 16), C.c_void_p(1 << 12), None)


def _refused(rc, who, *words):
    assert rc == EINVAL
    msg = sj.lib().sjpeg_hip_last_error().decode()
    assert who in msg
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("call,who", [(_full, FULL), (_ragged, RAGGED)])
def test_the_element_size_rules_come_before_device_work(call, who):
    w = 16
    # an odd byte stride for half elements
    _refused(call(_frames(strides=(33, 33, 33)), F16), who, "frame 1", "row_stride[0]", "element size")
    _refused(call(_frames(strides=(-33, -33, -33), bad=0), BF16), who, "frame 0", "row_stride[0]", "element size")
    _refused(call(_frames(strides=(66, 66, 66)), F32), who, "frame 1", "row_stride[0]", "element size")
    # a stride of 2 * width - 2: one element short of a row
    _refused(call(_frames(strides=(2 * w - 2,) * 3), F16), who, "frame 1", "row_stride")
    _refused(call(_frames(strides=(-(2 * w - 2),) * 3), BF16), who, "frame 1", "row_stride")
    _refused(call(_frames(strides=(4 * w - 4,) * 3), F32), who, "frame 1", "row_stride")
    _refused(call(_frames(strides=(2 * w,) * 3), F32), who, "frame 1", "row_stride")          # (enough for 2 bytes, not for 4)
    # a plane at an odd address
    _refused(call(_frames(planes=(1 << 24, (2 << 24) + 1, 3 << 24)), F16), who, "frame 1", "plane[1]", "element size")
    _refused(call(_frames(planes=((1 << 24) + 2, 2 << 24, 3 << 24), bad=0), F32), who, "frame 0", "plane[0]", "element size")
    # the planar rules hold as they are
    _refused(call(_frames(strides=(48, 64, 48)), F16), who, "frame 1", "row_stride[1]", "row_stride[0]")
    _refused(call(_frames(planes=(1 << 24, None, 3 << 24)), F32), who, "frame 1", "null plane")
    # every sampling takes the formats: the same refusal, not "yuv_mode does not match"
    for mode in (sj.YUV_444, sj.YUV_400):
        _refused(call(_frames(strides=(33, 33, 33)), F16, mode), who, "frame 1", "row_stride[0]")


def test_auto_and_sharp_admit_the_formats():
    for fmt in (F32, F16, BF16):
        for mode in (sj.YUV_AUTO, sj.YUV_SHARP):
            _refused(_full(_frames(strides=(67, 67, 67)), fmt, mode), FULL, "frame 1", "row_stride[0]", "element size")


def test_non_finite_transform_refused():
    L = sj.lib()
    for scale, bias in ((float("nan"), 0.0), (float("inf"), 0.0), (255.0, float("-inf")), (255.0, float("nan"))):
        # (the arguments are checked before the engine is touched)
        assert L.sjpeg_hip_engine_set_pixel_transform(FAKE, scale, bias) == EINVAL
        assert "finite" in L.sjpeg_hip_last_error().decode()
        with pytest.raises(sj.SjpegError, match="finite"):
            sj.FloatPixels([], scale, bias)
    assert L.sjpeg_hip_engine_set_pixel_transform(None, 255.0, 0.0) == EINVAL


def test_engineless_calls_refuse_the_formats_by_name():
    L = sj.lib()
    for fmt in (F32, F16, BF16):
        src = sj.Source()
        src.format = fmt
        for i in range(3):
            src.plane[i] = (i + 1) << 24
            src.row_stride[i] = 64
            src.frame_stride[i] = 64 * 16
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
        fn = C.cast(L.sjpeg_hip_riskiness_sums, proto)
        assert fn(C.addressof(src), 16, 16, 1, 1 << 20, 1 << 21, None) == EINVAL
        msg = L.sjpeg_hip_last_error().decode()
        assert "sjpeg_hip_riskiness_sums" in msg and "sjpeg_hip_riskiness_ragged_src" in msg, msg
        L.sjpeg_hip_sharp_workspace.restype = C.c_size_t
        L.sjpeg_hip_sharp_workspace.argtypes = [C.c_int, C.c_int, C.c_int]
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                            C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p)
        fn = C.cast(L.sjpeg_hip_sharp_yuv, proto)
        assert fn(C.addressof(src), 16, 16, 1, 1 << 20, 1 << 21, 1 << 22, 256, 64, 1 << 23,
                  L.sjpeg_hip_sharp_workspace(16, 16, 1), None) == EINVAL
        msg = L.sjpeg_hip_last_error().decode()
        assert "sjpeg_hip_sharp_yuv" in msg and "sjpeg_hip_sharp_yuv_ragged" in msg, msg


def test_float_pixels_argument_checks():
    import torch
    cpu = [torch.zeros((3, 8, 8), dtype=torch.float32)]
    before = sj.packed_stats()
    for fn in (sj.encode_images, sj.compress_images, sj.riskiness_images):
        with pytest.raises(sj.SjpegError, match="image 0 is not a CUDA tensor"):
            fn(sj.FloatPixels(cpu), layout="chw")
        with pytest.raises(sj.SjpegError, match="layout='chw'"):
            fn(sj.FloatPixels(cpu), layout="hwc")
        with pytest.raises(sj.SjpegError, match="layout='chw'"):
            fn(sj.FloatPixels(cpu))
    with pytest.raises(sj.SjpegError, match="image 0 is not a CUDA tensor"):
        sj.encode_images_full_chw(sj.FloatPixels(cpu))
    with pytest.raises(sj.SjpegError, match="layout='chw'"):
        sj.encode_images_full(sj.FloatPixels(cpu))
    # the dtype checks of the wrapper's pictures (meta tensors: "CUDA" enough for the argument checks, no device needed)
    class _Cuda(torch.Tensor):
        is_cuda = True
    def fake(dtype):
        return torch.zeros((3, 8, 8), dtype=dtype).as_subclass(_Cuda)
    with pytest.raises(sj.SjpegError, match=r"image 1 is torch\.float16, image 0 torch\.float32"):
        sj.encode_images(sj.FloatPixels([fake(torch.float32), fake(torch.float16)]), layout="chw")
    with pytest.raises(sj.SjpegError, match=r"image 1 is torch\.float64"):
        sj.encode_images(sj.FloatPixels([fake(torch.float32), fake(torch.float64)]), layout="chw")
    with pytest.raises(sj.SjpegError, match=r"image 0 is torch\.float64"):
        sj.riskiness_images(sj.FloatPixels([fake(torch.float64)]), layout="chw")
    with pytest.raises(sj.SjpegError, match=r"image 0 is torch\.uint8"):
        sj.encode_images_full_chw(sj.FloatPixels([fake(torch.uint8)]))
    # a bare float tensor keeps the refusal it always had
    with pytest.raises(sj.SjpegError, match=r"is torch\.float32, not torch\.uint8"):
        sj.encode_images([fake(torch.float32)], layout="chw")
    assert sj.packed_stats() == before


def test_pinned_signatures_are_unchanged():
    for fn in (sj.encode_images, sj.compress_images, sj.riskiness_images):
        sig = inspect.signature(fn).parameters
        assert list(sig)[-1] == "layout" and sig["layout"].default == "hwc", fn.__name__
        assert "scale" not in sig and "bias" not in sig
    assert list(inspect.signature(sj.encode_images_full_chw).parameters) == list(inspect.signature(sj.encode_images_full).parameters)
    assert list(inspect.signature(sj.encode_images_full).parameters)[-1] == "packed"
    assert list(inspect.signature(sj.FloatPixels).parameters) == ["images", "scale", "bias"]
    assert list(inspect.signature(sj.Engine.set_pixel_transform).parameters) == ["self", "scale", "bias"]
