"""Channels-last, RGBA and gray float pictures (SJPEG_HIP_SRC_RGB_F* / _RGBA_F* / _GRAY_F*) and the per-channel pixel
transform without a GPU: the enum values, the argument checks of the ragged and full entry points before any device
work (the frame and the field named), the refusals of the gray formats and of the calls without an engine, the
transform's setters and getters, how Python reads a picture's strides, FloatPixels.normalized, the premise of the gray
route on the CPU oracle, and the pinned signatures."""
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
# format -> (step, channels, element size)
FORMATS = {12: (3, 3, 4), 13: (3, 3, 2), 14: (3, 3, 2), 15: (4, 3, 4), 16: (4, 3, 2), 17: (4, 3, 2),
           18: (1, 1, 4), 19: (1, 1, 2), 20: (1, 1, 2)}
NAMES = {12: "RGB_F32", 13: "RGB_F16", 14: "RGB_BF16", 15: "RGBA_F32", 16: "RGBA_F16", 17: "RGBA_BF16",
         18: "GRAY_F32", 19: "GRAY_F16", 20: "GRAY_BF16"}
GRAY = (18, 19, 20)


def _mode(fmt):
    return sj.YUV_400 if fmt in GRAY else sj.YUV_420


def test_enum_values_and_exports():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    for value, name in NAMES.items():
        assert re.search(r"\bSJPEG_HIP_SRC_%s\s*=\s*%d\b" % (name, value), text), name
        assert getattr(sj, "SRC_" + name) == value
    assert sj.lib().sjpeg_hip_abi_version() == 18
    assert re.search(r"#define\s+SJPEG_HIP_ABI_VERSION\s+18\b", text)
    for name in ("sjpeg_hip_engine_set_pixel_transform3", "sjpeg_hip_engine_get_pixel_transform3"):
        assert name in text and name in sj.EXPORTED_C_SYMBOLS
        getattr(sj.lib(), name)


def _frames(w=16, h=16, stride=1024, plane=1 << 24, bad=1):
    """Two frames of ONE plane (plane[1], plane[2] stay NULL: they are ignored); frame `bad` gets the stride and plane
    given, the other one is in order for any of the formats."""
    f = (sj.RaggedFrame * 2)()
    for k in range(2):
        f[k].width, f[k].height = w, h
        f[k].plane[0] = plane if k == bad else 1 << 24
        f[k].row_stride[0] = stride if k == bad else 1024
        f[k].out_offset = 4096 * k
        f[k].out_capacity = 4096
    return f


def _params(mode, method=4):
    q = np.ones((1, 2, 64), np.uint8)
    p = sj.RaggedParams(mode, method, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    p._keep = q
    return p


def _full(frames, fmt, mode=None):
    p = _params(_mode(fmt) if mode is None else mode)
    return getattr(sj.lib(), FULL)(FAKE, fmt, 2, frames, C.byref(p), 1 << 16, 1 << 12, None, None, None, None)


def _ragged(frames, fmt, mode=None):
    tables, _ = sj.make_tables(quality=75.0)
    tarr = (sj.ScanTables * 1)(tables)
    return getattr(sj.lib(), RAGGED)(FAKE, fmt, _mode(fmt) if mode is None else mode, 2, frames,
                                     C.cast(tarr, C.c_void_p), 0, None, None, 1, C.c_void_p(1 << 16), C.c_void_p(1 << 12), None)


def _refused(rc, who, *words):
    assert rc == EINVAL
    msg = sj.lib().sjpeg_hip_last_error().decode()
    assert who in msg
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("call,who", [(_full, FULL), (_ragged, RAGGED)])
@pytest.mark.parametrize("fmt", sorted(FORMATS), ids=lambda f: NAMES[f])
def test_the_rules_come_before_device_work(call, who, fmt):
    w = 16
    step, channels, esz = FORMATS[fmt]
    need = ((w - 1) * step + channels) * esz
    # a stride or a plane off the element size
    _refused(call(_frames(stride=1024 + esz // 2), fmt), who, "frame 1", "row_stride[0]", "element size")
    _refused(call(_frames(stride=-(1024 + esz // 2), bad=0), fmt), who, "frame 0", "row_stride[0]", "element size")
    _refused(call(_frames(plane=(1 << 24) + esz // 2), fmt), who, "frame 1", "plane[0]", "element size")
    # one element short of the last sample that is read, both directions
    _refused(call(_frames(stride=need - esz), fmt), who, "frame 1", "row_stride")
    _refused(call(_frames(stride=-(need - esz), bad=0), fmt), who, "frame 0", "row_stride")
    # exactly that length passes: the frame is then refused for what the loop checks AFTER its strides
    for sign in (1, -1):
        f = _frames(stride=sign * need)
        f[1].out_offset, f[1].out_capacity = 2 ** 64 - 1, 2
        _refused(call(f, fmt), who, "frame 1", "out_offset + out_capacity")
        f = _frames(stride=sign * (need - esz))
        f[1].out_offset, f[1].out_capacity = 2 ** 64 - 1, 2
        _refused(call(f, fmt), who, "frame 1", "row_stride")


@pytest.mark.parametrize("fmt", GRAY, ids=lambda f: NAMES[f])
def test_gray_is_400_only(fmt):
    for mode in (sj.YUV_420, sj.YUV_444):
        _refused(_ragged(_frames(), fmt, mode), RAGGED, "yuv_mode does not match the source format")
        _refused(_full(_frames(), fmt, mode), FULL, "yuv_mode")
    # AUTO and SHARP refuse them with the message the byte gray format gets
    for mode in (sj.YUV_AUTO, sj.YUV_SHARP):
        rc = _full(_frames(), sj.SRC_GRAY, mode)
        assert rc == EINVAL
        byte_msg = sj.lib().sjpeg_hip_last_error().decode()
        assert _full(_frames(), fmt, mode) == EINVAL
        assert sj.lib().sjpeg_hip_last_error().decode() == byte_msg


def test_auto_and_sharp_admit_rgb_and_rgba():
    for fmt in range(12, 18):
        esz = FORMATS[fmt][2]
        for mode in (sj.YUV_AUTO, sj.YUV_SHARP):
            _refused(_full(_frames(stride=1024 + esz // 2), fmt, mode), FULL, "frame 1", "row_stride[0]", "element size")


def test_riskiness_and_sharp_ragged_refuse_gray_as_the_byte_format():
    L = sj.lib()
    fr = _frames()
    ptrs = (C.c_void_p * 2)(1 << 25, 1 << 26)

    def risk(fmt):
        assert L.sjpeg_hip_riskiness_ragged_src(FAKE, fmt, 2, fr, None, 1 << 22, None) == EINVAL
        return L.sjpeg_hip_last_error().decode()

    def sharp(fmt):
        assert L.sjpeg_hip_sharp_yuv_ragged(FAKE, fmt, 2, fr, ptrs, ptrs, ptrs, 1 << 27, 1 << 20, None) == EINVAL
        return L.sjpeg_hip_last_error().decode()

    for fmt in GRAY:
        assert risk(fmt) == risk(sj.SRC_GRAY)
        assert sharp(fmt) == sharp(sj.SRC_GRAY)


def test_engineless_calls_refuse_the_nine_formats():
    L = sj.lib()
    for fmt in FORMATS:
        src = sj.Source()
        src.format = fmt
        src.plane[0] = 1 << 24
        src.row_stride[0] = 1024
        src.frame_stride[0] = 1024 * 16
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


# ---- the per-channel transform

def test_transform3_argument_checks():
    L = sj.lib()
    three = C.c_float * 3
    ok = three(1.0, 2.0, 4.0)
    for bad in (float("nan"), float("inf"), float("-inf")):
        for c in range(3):
            v = [255.0, 255.0, 255.0]
            v[c] = bad
            # (the arguments are checked before the engine is touched)
            assert L.sjpeg_hip_engine_set_pixel_transform3(FAKE, three(*v), ok) == EINVAL
            assert "finite" in L.sjpeg_hip_last_error().decode() and "[%d]" % c in L.sjpeg_hip_last_error().decode()
            assert L.sjpeg_hip_engine_set_pixel_transform3(FAKE, ok, three(*v)) == EINVAL
            assert "finite" in L.sjpeg_hip_last_error().decode()
    assert L.sjpeg_hip_engine_set_pixel_transform3(None, ok, ok) == EINVAL
    assert L.sjpeg_hip_engine_set_pixel_transform3(FAKE, None, ok) == EINVAL
    assert L.sjpeg_hip_engine_get_pixel_transform3(None, ok, ok) == EINVAL
    with pytest.raises(sj.SjpegError, match="finite"):
        sj.FloatPixels([], (255.0, float("nan"), 255.0), 0.0)
    with pytest.raises(sj.SjpegError, match="finite"):
        sj.FloatPixels([], 255.0, [0.0, 0.0, float("inf")])


def test_transform3_round_trips_on_engine_state():
    """Set then get round-trips and the one-value setter fills three: on a real engine where a device exists (the
    library makes engines on a device only); the Python side of the contract -- one value or three -- everywhere."""
    L = sj.lib()
    three = C.c_float * 3
    if sj.device_count() > 0:
        eng = sj.Engine(0)
        assert eng.pixel_transform3() == ((255.0,) * 3, (0.0,) * 3)
        eng.set_pixel_transform((1.0, 2.0, 4.0), (0.0, 1.0, 2.0))
        assert eng.pixel_transform3() == ((1.0, 2.0, 4.0), (0.0, 1.0, 2.0))
        assert eng.pixel_transform() == (1.0, 0.0)
        eng.set_pixel_transform(127.5, 127.5)
        assert eng.pixel_transform3() == ((127.5,) * 3, (127.5,) * 3)
        s, b = three(), three()
        assert L.sjpeg_hip_engine_set_pixel_transform3(eng._h, three(3.0, 5.0, 7.0), three(-1.0, 0.5, 9.0)) == 0
        assert L.sjpeg_hip_engine_get_pixel_transform3(eng._h, s, b) == 0
        assert (tuple(s), tuple(b)) == ((3.0, 5.0, 7.0), (-1.0, 0.5, 9.0))
        eng.close()
    # the Python side of the contract: one value or three
    fp = sj.FloatPixels([], 2.0, 1.0)
    assert (fp.scale, fp.bias, fp.scale3, fp.bias3) == (2.0, 1.0, (2.0,) * 3, (1.0,) * 3)
    fp = sj.FloatPixels([], (1, 2, 4), np.array([0.0, 1.0, 2.0]))
    assert (fp.scale3, fp.bias3) == ((1.0, 2.0, 4.0), (0.0, 1.0, 2.0))
    for bad in ((1.0, 2.0), (1.0, 2.0, 3.0, 4.0), ()):
        with pytest.raises(sj.SjpegError, match="sequence of three"):
            sj.FloatPixels([], bad, 0.0)
        with pytest.raises(sj.SjpegError, match="sequence of three"):
            sj.FloatPixels([], 255.0, bad)
        with pytest.raises(sj.SjpegError, match="sequence of three"):
            sj.FloatPixels.normalized([], bad, 1.0)
        with pytest.raises(sj.SjpegError, match="sequence of three"):
            sj.FloatPixels.normalized([], 0.5, bad)


def test_normalized_values():
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    fp = sj.FloatPixels.normalized([], mean, std)
    assert fp.scale3 == tuple(float(np.float32(255.0 * np.float64(s))) for s in std)
    assert fp.bias3 == tuple(float(np.float32(255.0 * np.float64(m))) for m in mean)
    fp = sj.FloatPixels.normalized([], 0.5, 0.5)
    assert (fp.scale, fp.bias) == (127.5, 127.5)
    fp = sj.FloatPixels.normalized([], 0.0, (1.0, 0.5, 0.25))
    assert fp.scale3 == (255.0, 127.5, 63.75) and fp.bias3 == (0.0, 0.0, 0.0)


# ---- how Python reads a picture's strides (fake "CUDA" tensors: enough for the argument checks, no device needed)

def _fake_cuda():
    import torch

    class _Cuda(torch.Tensor):
        is_cuda = True
    return lambda t: t.as_subclass(_Cuda)


def test_python_classification():
    import torch
    fake = _fake_cuda()
    h, w = 5, 7
    for dt, (planar, rgb, rgba, gray) in ((torch.float32, (9, 12, 15, 18)), (torch.float16, (10, 13, 16, 19)),
                                          (torch.bfloat16, (11, 14, 17, 20))):
        esz = torch.zeros((), dtype=dt).element_size()
        fp = sj.FloatPixels([])
        # planar, as today
        x = fake(torch.zeros((3, h, w), dtype=dt))
        planes, dims, _, fmt = sj._chw_planes("t", [x], fp)
        assert fmt == planar and dims == [(w, h)] and len(planes[0]) == 3
        # a slice of a channels_last batch: strides (1, 3W, 3)
        nchw = torch.zeros((2, 3, h, w), dtype=dt).to(memory_format=torch.channels_last)
        assert nchw[1].stride() == (1, 3 * w, 3)
        planes, dims, _, fmt = sj._chw_planes("t", [fake(nchw[0]), fake(nchw[1])], fp)
        assert fmt == rgb and dims == [(w, h)] * 2
        assert planes[1] == [(nchw[1].data_ptr(), 3 * w * esz)]
        # hwc.permute(2, 0, 1)
        planes, dims, _, fmt = sj._chw_planes("t", [fake(torch.zeros((h, w, 3), dtype=dt).permute(2, 0, 1))], fp)
        assert fmt == rgb and planes[0][0][1] == 3 * w * esz
        # rgba.permute(2, 0, 1)[:3], and x[..., 1:4] of ARGB
        a = torch.zeros((h, w, 4), dtype=dt)
        planes, dims, _, fmt = sj._chw_planes("t", [fake(a.permute(2, 0, 1)[:3])], fp)
        assert fmt == rgba and planes[0] == [(a.data_ptr(), 4 * w * esz)] and dims == [(w, h)]
        planes, dims, _, fmt = sj._chw_planes("t", [fake(a[..., 1:4].permute(2, 0, 1))], fp)
        assert fmt == rgba and planes[0] == [(a.data_ptr() + esz, 4 * w * esz)]
        # gray: [1, H, W] and [H, W], a crop too
        for g in (torch.zeros((1, h, w), dtype=dt), torch.zeros((h, w), dtype=dt), torch.zeros((h, w + 3), dtype=dt)[:, 2:2 + w]):
            planes, dims, _, fmt = sj._chw_planes("t", [fake(g)], fp)
            assert fmt == gray and dims == [(w, h)] and planes[0] == [(g.data_ptr(), g.stride(-2) * esz)]
        # size-1 dimensions as the planar code treats them: a one-pixel-wide picture is planar whatever stride(2) says
        one = torch.zeros((2, 3, h, 1), dtype=dt).to(memory_format=torch.channels_last)[0]
        assert sj._chw_planes("t", [fake(one)], fp)[3] == planar
        # ... and takes the call's layout where the others say which it is
        assert sj._chw_planes("t", [fake(nchw[0]), fake(one)], fp)[3] == rgb
        assert sj._chw_planes("t", [fake(one), fake(a.permute(2, 0, 1)[:3])], fp)[3] == rgba
        # a mixed call names the odd image, with its shape and strides
        with pytest.raises(sj.SjpegError) as e:
            sj._chw_planes("t", [x, fake(nchw[0])], fp)
        assert "image 1" in str(e.value) and str(tuple(nchw[0].shape)) in str(e.value) and str(tuple(nchw[0].stride())) in str(e.value)
        with pytest.raises(sj.SjpegError, match="image 1"):
            sj._chw_planes("t", [fake(nchw[0]), fake(a.permute(2, 0, 1)[:3])], fp)
        with pytest.raises(sj.SjpegError, match="image 2"):
            sj._chw_planes("t", [x, x, fake(torch.zeros((h, w), dtype=dt))], fp)
        # every other stride pattern keeps the refusal it has
        with pytest.raises(sj.SjpegError, match="image 0 must be"):
            sj._chw_planes("t", [fake(torch.zeros((3, h, 2 * w), dtype=dt)[:, :, ::2])], fp)
        with pytest.raises(sj.SjpegError, match="image 0 must be"):
            sj._chw_planes("t", [fake(torch.zeros((h, w, 5), dtype=dt).permute(2, 0, 1)[:3])], fp)
    # bytes: channels-last goes in as SRC_RGB / SRC_RGBA, gray stays refused
    u = torch.zeros((2, 3, h, w), dtype=torch.uint8).to(memory_format=torch.channels_last)
    planes, dims, _, fmt = sj._chw_planes("t", [fake(u[0]), fake(u[1])])
    assert fmt == sj.SRC_RGB and planes[1] == [(u[1].data_ptr(), 3 * w)]
    a = torch.zeros((h, w, 4), dtype=torch.uint8)
    assert sj._chw_planes("t", [fake(a.permute(2, 0, 1)[:3])])[3] == sj.SRC_RGBA
    assert sj._chw_planes("t", [fake(torch.zeros((3, h, w), dtype=torch.uint8))])[3] == sj.SRC_RGB_PLANAR
    with pytest.raises(sj.SjpegError, match="image 0 must be"):
        sj._chw_planes("t", [fake(torch.zeros((1, h, w), dtype=torch.uint8))])
    with pytest.raises(sj.SjpegError, match="image 1"):
        sj._chw_planes("t", [fake(u[0]), fake(torch.zeros((3, h, 2 * w), dtype=torch.uint8)[:, :, ::2])])


def test_gray_float_pixels_take_yuv_400_only():
    import torch
    fake = _fake_cuda()
    g = [fake(torch.zeros((1, 8, 8), dtype=torch.float16))]
    for mode in (sj.YUV_AUTO, sj.YUV_SHARP, sj.YUV_420, sj.YUV_444):
        with pytest.raises(sj.SjpegError, match="YUV_400 only"):
            sj.encode_images(sj.FloatPixels(g), 75.0, mode, layout="chw")
        with pytest.raises(sj.SjpegError, match="YUV_400 only"):
            sj.encode_images_full_chw(sj.FloatPixels(g), 75.0, mode)
    with pytest.raises(sj.SjpegError, match="YUV_400 only"):
        sj.compress_images(sj.FloatPixels(g), layout="chw")
    with pytest.raises(sj.SjpegError, match="YUV_400 only"):
        sj.riskiness_images(sj.FloatPixels(g), layout="chw")


# ---- the premise of the gray route

def test_gray_equals_rgb_400_on_the_oracle(oracle):
    """A gray float picture is handed to the colour path as R = G = B and coded in 4:0:0; that is the byte gray
    picture's JPEG only if the reference's luma of (v, v, v) is v for every v.  All 256 values, on the CPU oracle."""
    w, h = 32, 24
    img = np.random.RandomState(5).randint(0, 256, (h, w)).astype(np.uint8)
    img.reshape(-1)[:256] = np.arange(256)
    quant = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(75.0, quant.ctypes.data)
    gray = oracle.encode_src(sj.SRC_GRAY, [img], w, h, quant, yuv_mode=4)
    rgb = np.repeat(img[..., None], 3, 2).copy()
    assert gray == oracle.encode_src(sj.SRC_RGB, [rgb.reshape(h, -1)], w, h, quant, yuv_mode=4)
    assert gray == oracle.encode(rgb, 75.0, sj.YUV_400)


def test_pinned_signatures_still_hold():
    for fn in (sj.encode_images, sj.compress_images, sj.riskiness_images):
        sig = inspect.signature(fn).parameters
        assert list(sig)[-1] == "layout" and sig["layout"].default == "hwc", fn.__name__
    assert list(inspect.signature(sj.FloatPixels).parameters) == ["images", "scale", "bias"]
    assert list(inspect.signature(sj.FloatPixels.normalized).parameters) == ["images", "mean", "std"]
    assert list(inspect.signature(sj.Engine.set_pixel_transform).parameters) == ["self", "scale", "bias"]
    assert list(inspect.signature(sj.Engine.pixel_transform3).parameters) == ["self"]
