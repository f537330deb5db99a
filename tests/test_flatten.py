"""Alpha flattened inside the ragged call on the GPU (sjpeg_hip_flatten_ragged_src, sjpeg_hip_encode_ragged_flattened_src,
the flat sheet entries, Flattened, flatten_images).  The contract is sjpeg_hip.h's: the flattened picture F of a frame
is b = (a s + (255 - a) bg + 127) // 255 (premultiplied: min(255, s + ((255 - a) bg + 127) // 255)) in integers, and a
flattened call makes byte for byte what the corresponding existing call makes of F handed over as SJPEG_HIP_SRC_RGB.
The expectation is _flatten() below, the two formulas in numpy integers, fed to the existing models -- _area of
test_resize.py, _upright of test_orient.py, sheet_model.py -- and to the existing entry points for the JPEG bytes.
Every comparison is byte equality."""
import numpy as np
import pytest
import torch

import sheet_model as sm
import sjpeg_amd as sj
from oracle import synth
from test_orient import _upright
from test_reduce import BF16, DMAX, F16, F32, XFORM3, _check_pictures, _quant, _rgb_planes, _seen, _streams
from test_resize import _area

pytestmark = pytest.mark.gpu

# source -> size: one pixel; identities (the flatten-copy) at widths that are no multiple of 4; a plain resize; two
# tiles across and two down at ratio 1; 64 lanes a column; a segment staged in chunks (6000 pixels: above the 4096
# four-byte pixels and the 5461 pixels of three byte runs that fit the stage)
SHAPES = [((1, 1), (1, 1)), ((3, 2), (3, 2)), ((5, 7), (5, 7)), ((7, 5), (3, 2)), ((257, 17), (257, 17)), ((300, 40), (7, 3)),
          ((6000, 2), (1, 1))]
BACKGROUNDS = [(255, 255, 255), (0, 0, 0), (17, 128, 250)]
# format -> (memory layout, dtype or None for bytes)
ALPHA_FORMATS = {"BGRA": (sj.SRC_BGRA, "bgra", None), "RGBA": (sj.SRC_RGBA, "rgba", None), "RGBA_F32": (sj.SRC_RGBA_F32, "rgba", F32),
                 "RGBA_F16": (sj.SRC_RGBA_F16, "rgba", F16), "RGBA_BF16": (sj.SRC_RGBA_BF16, "rgba", BF16)}
# the alpha sample's transform, none of them (255, 0): alpha in -1..1 for fp32 and half, exact halves for bfloat16
AXFORM = {F32: (127.5, 127.5), F16: (127.5, 127.5), BF16: (2.0, 1.0)}


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.fixture(scope="module")
def risk_table():
    import os
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        tab = f.read()
    sj.set_riskiness_table(tab)
    return tab


# ---- the expectation, in numpy integers

def _flatten(s, a, bg, premultiplied):
    """F of colour bytes s [H, W, 3] and alpha bytes a [H, W] over bg: sjpeg_hip.h's two formulas"""
    s, a, bg = s.astype(np.int64), a.astype(np.int64)[..., None], np.asarray(bg, np.int64)
    if premultiplied:
        return np.minimum(255, s + ((255 - a) * bg + 127) // 255).astype(np.uint8)
    return ((a * s + (255 - a) * bg + 127) // 255).astype(np.uint8)


def _alpha_seen(host, dtype):
    """the alpha byte of what lies on the device: the stored byte, or rint(clamp(fma(x, scale, bias), 0, 255)), NaN -> 0,
    restated in float64 and asserted far enough from a tie that the fp32 fma's one rounding cannot change it"""
    x = host[..., 3]
    if dtype is None:
        return x
    scale, bias = AXFORM[dtype]
    with np.errstate(invalid="ignore"):
        v = x.astype(np.float64) * scale + bias
        fin = np.isfinite(v)
        assert (np.abs(v[fin] - np.rint(v[fin])) <= 0.47).all()
        return np.where(np.isnan(v), 0.0, np.rint(np.clip(v, 0, 255))).astype(np.uint8)


def _rgba_on_device(u8, alpha, layout, dtype, seed=1, off=0, pad=0, specials=False, shift=0):
    """A device tensor [H, off + W + pad, 4] holding colours u8 [H, W, 3] and alpha [H, W] in `layout` / `dtype`, as
    test_reduce._on_device lays colours out (floats: fp32((k + d - bias) / scale) cast to dtype, d within DMAX); what
    lies beside the picture is 77 / NaN.  specials: the first alpha samples are NaN, +inf and -inf.  shift: the wider
    tensor starts that many elements into its allocation.  Returns (planes entry, the wider tensor [H, off + W + pad, 4],
    the host copy of the view as uint8 or float32)."""
    h, w = u8.shape[:2]
    if dtype is None:
        src = np.concatenate([u8[..., [2, 1, 0]] if layout == "bgra" else u8, alpha[..., None]], axis=2)
    else:
        s = np.asarray(XFORM3[dtype][0] + (AXFORM[dtype][0],), np.float64)
        b = np.asarray(XFORM3[dtype][1] + (AXFORM[dtype][1],), np.float64)
        k = np.concatenate([u8, alpha[..., None]], axis=2).astype(np.float64)
        d = np.random.RandomState(seed).uniform(-DMAX[dtype], DMAX[dtype], k.shape) if DMAX[dtype] > 0 else 0.0
        src = ((k + d - b) / s).astype(np.float32)
        if specials:
            flat = src.reshape(-1, 4)
            for i, v in enumerate((np.nan, np.inf, -np.inf)):
                if i < len(flat):
                    flat[i, 3] = v
    tdt = torch.uint8 if dtype is None else dtype
    flat = torch.full((shift + h * (off + w + pad) * 4,), 77 if dtype is None else float("nan"), dtype=tdt)
    flat[shift:].view(h, off + w + pad, 4)[:, off:off + w] = torch.from_numpy(np.ascontiguousarray(src)).to(tdt)
    dev = flat.cuda()[shift:].view(h, off + w + pad, 4)
    view = dev[:, off:off + w]
    host = view.cpu().numpy() if dtype is None else view.cpu().to(torch.float32).numpy()
    return [(view.data_ptr(), dev.stride(0) * dev.element_size())], dev, host


def _seen_rgba(host, layout, dtype):
    """(the colour bytes [H, W, 3] in R, G, B order, the alpha bytes [H, W]) the kernel sees of a host copy"""
    return _seen(host, layout, dtype), _alpha_seen(host, dtype)


def _alphas(w, h, seed):
    """the four alpha contents: noise, all 0, all 255, and the pair 1 / 254 in a checkerboard"""
    rs = np.random.RandomState(seed)
    pair = np.where((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1, 254, 1).astype(np.uint8)
    return [rs.randint(0, 256, (h, w)).astype(np.uint8), np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8), pair]


def test_the_expectation_itself():
    """_flatten() against the formulas sample by sample in Python integers, and its end values"""
    rs = np.random.RandomState(7)
    s, a = rs.randint(0, 256, (4, 5, 3)).astype(np.uint8), rs.randint(0, 256, (4, 5)).astype(np.uint8)
    a[0, 0], a[0, 1] = 0, 255
    bg = (17, 128, 250)
    F, P = _flatten(s, a, bg, False), _flatten(s, a, bg, True)
    for y in range(4):
        for x in range(5):
            for c in range(3):
                av, sv = int(a[y, x]), int(s[y, x, c])
                assert F[y, x, c] == (av * sv + (255 - av) * bg[c] + 127) // 255
                assert P[y, x, c] == min(255, sv + ((255 - av) * bg[c] + 127) // 255)
    assert tuple(F[0, 0]) == bg and np.array_equal(F[0, 1], s[0, 1]) and np.array_equal(P[0, 1], s[0, 1])
    x = np.array([[[0.0, 0, 0, np.nan], [0, 0, 0, np.inf], [0, 0, 0, -np.inf], [0, 0, 0, 1.0], [0, 0, 0, -1.0]]], np.float32)
    assert _alpha_seen(x, F32).tolist() == [[0, 255, 0, 255, 0]]


# ---- 1. the kernel alone: per alpha format the same frames under every background and both modes

@pytest.fixture(scope="module")
def sources():
    """(colours u8 [H, W, 3], alpha u8 [H, W], (w, h)): noise and all-255 colours under the four alpha contents, for
    every shape.  Never written to."""
    out = []
    for k, ((w, h), size) in enumerate(SHAPES):
        for ci, colour in enumerate((synth.g_noise(w, h, 8100 + k), np.full((h, w, 3), 255, np.uint8))):
            for alpha in _alphas(w, h, 8200 + 2 * k + ci):
                out.append((colour, alpha, size))
    return out


@pytest.mark.parametrize("name", list(ALPHA_FORMATS))
def test_flatten_ragged_against_numpy(engine, sources, name):
    fmt, layout, dtype = ALPHA_FORMATS[name]
    ascale, abias = AXFORM[dtype] if dtype is not None else (255.0, 0.0)
    if dtype is not None:
        engine.set_pixel_transform(*XFORM3[dtype])
    planes, keep, seen, dims, sizes = [], [], [], [], []
    for k, (u8, alpha, size) in enumerate(sources):
        p, dev, host = _rgba_on_device(u8, alpha, layout, dtype, seed=k, off=k % 3, pad=(k // 3) % 2, specials=k % 4 == 0)
        keep.append(dev)
        s, a = _seen_rgba(host, layout, dtype)
        if dtype is None:
            assert np.array_equal(s, u8) and np.array_equal(a, alpha)
        elif k % 4 == 0:
            assert a.reshape(-1)[:3].tolist() == [0, 255, 0][:a.size]          # NaN, +inf, -inf
        planes.append(p); seen.append((s, a)); dims.append((u8.shape[1], u8.shape[0])); sizes.append(size)
    for premultiplied in (False, True):
        for bg in BACKGROUNDS:
            flatten = sj.Flatten(bg, premultiplied, ascale, abias)
            rfmt, pics, buf = engine.flatten_ragged(fmt, planes, dims, flatten, sizes)
            assert rfmt == sj.SRC_RGB
            for p, size in zip(pics, sizes):
                assert (p.shape[1], p.shape[0]) == size and p.data_ptr() % 16 == 0 and p.stride(0) == (size[0] * 3 + 3) // 4 * 4
            _check_pictures(pics, [_area(_flatten(s, a, bg, premultiplied), *size) for (s, a), size in zip(seen, sizes)])
    # sizes None and orientations None: the flatten alone, F itself
    _, pics, _ = engine.flatten_ragged(fmt, planes[:24], dims[:24], flatten)
    _check_pictures(pics, [_flatten(s, a, bg, premultiplied) for s, a in seen[:24]])
    engine.set_pixel_transform(255.0, 0.0)


def test_the_end_values(engine):
    """alpha 255 is the picture and alpha 0 the background, to the byte, in both modes (premultiplied over black)"""
    u8 = synth.g_noise(37, 11, 8300)
    for alpha, bg, pre, want in ((255, (17, 128, 250), False, u8), (255, (17, 128, 250), True, u8),
                                 (0, (17, 128, 250), False, np.broadcast_to(np.uint8([17, 128, 250]), u8.shape)),
                                 (0, (0, 0, 0), True, u8)):
        p, dev, host = _rgba_on_device(u8, np.full(u8.shape[:2], alpha, np.uint8), "rgba", None)
        _, pics, _ = engine.flatten_ragged(sj.SRC_RGBA, [p], [(37, 11)], sj.Flatten(bg, pre))
        _check_pictures(pics, [np.ascontiguousarray(want)])


# ---- 2. orientations: the store is test_orient.py's; this is the plumbing

@pytest.mark.parametrize("name", ["BGRA", "RGBA_F16"])
def test_orientations_1_6_7(engine, name):
    fmt, layout, dtype = ALPHA_FORMATS[name]
    if dtype is not None:
        engine.set_pixel_transform(*XFORM3[dtype])
    bg = (17, 128, 250)
    flatten = sj.Flatten(bg, False, *(AXFORM[dtype] if dtype is not None else (255.0, 0.0)))
    planes, keep, wants, dims, sizes, orients = [], [], [], [], [], []
    for k, ((w, h), size) in enumerate([SHAPES[2], SHAPES[3], SHAPES[5]]):
        p, dev, host = _rgba_on_device(synth.g_noise(w, h, 8400 + k), _alphas(w, h, 8410 + k)[0], layout, dtype, seed=k, off=k)
        keep.append(dev)
        R = _area(_flatten(*_seen_rgba(host, layout, dtype), bg, False), *size)
        for o in (1, 6, 7):
            planes.append(p); dims.append((w, h)); sizes.append(size); orients.append(o); wants.append(_upright(R, o))
    _, pics, _ = engine.flatten_ragged(fmt, planes, dims, flatten, sizes, orients)
    for p, size, o in zip(pics, sizes, orients):
        assert (p.shape[1], p.shape[0]) == sj.oriented_size(*size, o)
    _check_pictures(pics, wants)
    engine.set_pixel_transform(255.0, 0.0)


# ---- 3. strides and bounds

def test_negative_row_stride(engine):
    dims, sizes = [(17, 9), (63, 65), (300, 40)], [(16, 9), (5, 64), (300, 40)]
    bg = (0, 0, 0)
    planes, keep, wants = [], [], []
    for k, (w, h) in enumerate(dims):
        rgba = np.concatenate([synth.g_noise(w, h, 8500 + k), _alphas(w, h, 8510 + k)[0][..., None]], axis=2)
        d = torch.from_numpy(np.ascontiguousarray(rgba[::-1])).cuda()                       # stored bottom-up
        keep.append(d)
        planes.append([(d.data_ptr() + (h - 1) * d.stride(0), -d.stride(0))])
        wants.append(_area(_flatten(rgba[..., :3], rgba[..., 3], bg, True), *sizes[k]))
    _, pics, _ = engine.flatten_ragged(sj.SRC_RGBA, planes, dims, sj.Flatten(bg, True), sizes)
    _check_pictures(pics, wants)


def test_odd_column_crop_of_a_wider_float_tensor(engine):
    """element-only alignment: the crop starts at column 1 of a wider tensor that itself starts one element into its
    allocation, so every row of halfs starts 2 bytes off a dword"""
    bg = (17, 128, 250)
    u8, alpha = synth.g_noise(31, 33, 8600), _alphas(31, 33, 8610)[0]
    sizes = [(31, 33), (30, 17), (4, 5)]
    for fmt, dtype in ((sj.SRC_RGBA_F16, F16), (sj.SRC_RGBA_BF16, BF16), (sj.SRC_RGBA_F32, F32)):
        engine.set_pixel_transform(*XFORM3[dtype])
        p, dev, host = _rgba_on_device(u8, alpha, "rgba", dtype, seed=3, off=1, pad=2, specials=True, shift=1)
        assert p[0][0] % 4 == (0 if dtype is F32 else 2) and p[0][0] % 16 != 0
        F = _flatten(*_seen_rgba(host, "rgba", dtype), bg, False)
        _, pics, _ = engine.flatten_ragged(fmt, [p] * 3, [(31, 33)] * 3, sj.Flatten(bg, False, *AXFORM[dtype]), sizes)
        _check_pictures(pics, [_area(F, *s) for s in sizes])
    engine.set_pixel_transform(255.0, 0.0)


def test_guard_bytes_around_the_output_buffer(engine, sources):
    picked = sources[::3]
    planes, keep, wants, dims, sizes, orients = [], [], [], [], [], []
    bg = (255, 255, 255)
    for k, (u8, alpha, size) in enumerate(picked):
        p, dev, host = _rgba_on_device(u8, alpha, "bgra", None, off=k % 2)
        keep.append(dev)
        o = (1, 6, 3, 8)[k % 4]
        planes.append(p); dims.append((u8.shape[1], u8.shape[0])); sizes.append(size); orients.append(o)
        wants.append(_upright(_area(_flatten(u8, alpha, bg, False), *size), o))
    frames, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
    arr = np.ascontiguousarray(np.asarray(sizes, np.int32))
    oarr = np.ascontiguousarray(np.asarray(orients, np.uint8))
    need = sj.lib().sjpeg_hip_orient_ragged_bytes(sj.SRC_BGRA, len(dims), frames, arr.ctypes.data, oarr.ctypes.data)
    assert need > 0 and need % 16 == 0
    guard = 256
    whole = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    assert (whole.data_ptr() + guard) % 16 == 0
    _, pics, _ = engine.flatten_ragged(sj.SRC_BGRA, planes, dims, sj.Flatten(bg), sizes, orients, out=whole[guard:guard + need])
    _check_pictures(pics, wants)
    host = whole.cpu().numpy()
    assert (host[:guard] == 0xA5).all() and (host[guard + need:] == 0xA5).all()
    # one byte short is refused before anything runs
    with pytest.raises(sj.SjpegError, match="bytes"):
        engine.flatten_ragged(sj.SRC_BGRA, planes, dims, sj.Flatten(bg), sizes, orients, out=whole[guard:guard + need - 16][:need - 1])


# ---- 4. encodes of one small batch: each against the same call on the flattened uint8 pictures

ENC_DIMS = [(64, 48), (31, 33), (17, 9)]
ENC_SIZES = [(40, 30), (31, 33), (16, 9)]
ENC_ORIENTS = [6, 1, 3]
ENC_BG = (17, 128, 250)


@pytest.fixture(scope="module")
def batch():
    """(device RGBA pictures [H, W, 4], the flattened, resized, upright pictures on the device and the host)"""
    rgba = [np.concatenate([synth.g_struct(w, h, 8700 + k) if k % 2 else synth.g_noise(w, h, 8700 + k),
                            _alphas(w, h, 8710 + k)[0][..., None]], axis=2) for k, (w, h) in enumerate(ENC_DIMS)]
    up = [np.ascontiguousarray(_upright(_area(_flatten(x[..., :3], x[..., 3], ENC_BG, False), *s), o))
          for x, s, o in zip(rgba, ENC_SIZES, ENC_ORIENTS)]
    return [torch.from_numpy(x).cuda() for x in rgba], [torch.from_numpy(x).cuda() for x in up], up


def _rgba_planes(devs):
    return [[d.as_strided((d.shape[0], d.shape[1] * 4), (d.stride(0), 1))] for d in devs], [(d.shape[1], d.shape[0]) for d in devs]


def _wrapped(devs):
    return sj.Flattened(devs, ENC_BG, orientations=ENC_ORIENTS, sizes=ENC_SIZES)


@pytest.mark.parametrize("method", [0, 4])
def test_engine_entries_against_the_full_call(engine, batch, method):
    devs, up_dev, up = batch
    planes, dims = _rgba_planes(devs)
    uplanes, udims = _rgb_planes(up_dev)
    flatten = sj.Flatten(ENC_BG)
    out, szs, offs, modes, q, v = engine.encode_ragged_flattened(sj.SRC_RGBA, planes, dims, flatten, ENC_SIZES, ENC_ORIENTS, sj.YUV_420,
                                                                 _quant(), method)
    out2, szs2, offs2, modes2, q2, v2 = engine.encode_ragged_full(sj.SRC_RGB, uplanes, udims, sj.YUV_420, _quant(), method)
    want = _streams(out2, szs2, offs2)
    assert _streams(out, szs, offs) == want
    assert modes == modes2 and q == q2 and v == v2 and offs == offs2
    assert sj.encode_images(_wrapped(devs), 75.0, sj.YUV_420, engine=engine, method=method) == want
    assert sj.encode_images(up_dev, 75.0, sj.YUV_420, engine=engine, method=method) == want
    _check_pictures(sj.flatten_images(_wrapped(devs), engine=engine), up)


def test_compress_images_decides_on_the_flattened_picture(engine, risk_table, batch):
    devs, up_dev, up = batch
    assert sj.compress_images(_wrapped(devs), 75.0, engine=engine) == sj.compress_images(up_dev, 75.0, engine=engine)
    planes, dims = _rgba_planes(devs)
    uplanes, udims = _rgb_planes(up_dev)
    out, szs, offs, modes, _, _ = engine.encode_ragged_flattened(sj.SRC_RGBA, planes, dims, sj.Flatten(ENC_BG), ENC_SIZES, ENC_ORIENTS,
                                                                 sj.YUV_AUTO, _quant(), 4)
    out2, szs2, offs2, modes2, _, _ = engine.encode_ragged_full(sj.SRC_RGB, uplanes, udims, sj.YUV_AUTO, _quant(), 4)
    assert modes == modes2 and _streams(out, szs, offs) == _streams(out2, szs2, offs2)


def test_target_size_search(engine, batch):
    devs, up_dev, up = batch
    targets = [max(400, x.size // 6) for x in up]
    planes, dims = _rgba_planes(devs)
    uplanes, udims = _rgb_planes(up_dev)
    search = [dict(target_mode=sj.TARGET_SIZE, target_value=t) for t in targets]
    out, szs, offs, _, q, v = engine.encode_ragged_flattened(sj.SRC_RGBA, planes, dims, sj.Flatten(ENC_BG), ENC_SIZES, ENC_ORIENTS,
                                                             sj.YUV_420, _quant(), 4, search=search)
    out2, szs2, offs2, _, q2, v2 = engine.encode_ragged_full(sj.SRC_RGB, uplanes, udims, sj.YUV_420, _quant(), 4, search=search)
    want = _streams(out2, szs2, offs2)
    assert _streams(out, szs, offs) == want and q == q2 and v == v2
    assert sj.encode_images(_wrapped(devs), 75.0, sj.YUV_420, engine=engine, method=4, target_size=targets) == want


def test_packed(engine, batch):
    devs, up_dev, up = batch
    want = sj.encode_images(up_dev, 75.0, sj.YUV_444, engine=engine, method=4)
    assert sj.encode_images(_wrapped(devs), 75.0, sj.YUV_444, engine=engine, method=4, packed=True) == want
    planes, dims = _rgba_planes(devs)
    uplanes, udims = _rgb_planes(up_dev)
    out, szs, offs, modes, q, v = engine.encode_ragged_flattened_packed(sj.SRC_RGBA, planes, dims, sj.Flatten(ENC_BG), ENC_SIZES,
                                                                        ENC_ORIENTS, sj.YUV_444, _quant(), 4)
    out2, szs2, offs2, modes2, q2, v2 = engine.encode_ragged_full_packed(sj.SRC_RGB, uplanes, udims, sj.YUV_444, _quant(), 4)
    torch.cuda.synchronize()
    assert _streams(out, szs, offs.cpu().numpy()) == want == _streams(out2, szs2, offs2.cpu().numpy())
    assert offs.cpu().tolist() == offs2.cpu().tolist() and szs.cpu().tolist() == szs2.cpu().tolist()
    assert modes == modes2 and q == q2 and v == v2


def test_metadata(engine, batch):
    devs, up_dev, up = batch
    metas = [sj.PictureMetadata(exif=b"Exif\0\0" + bytes(range(40))), None,
             sj.PictureMetadata(xmp=b"<x:xmpmeta>flattened</x:xmpmeta>", app_markers=b"\xff\xe5\x00\x06abcd")]
    want = sj.encode_images_full_meta(up_dev, metas, yuv_mode=sj.YUV_420, engine=engine)
    assert sj.encode_images_full_meta(_wrapped(devs), metas, yuv_mode=sj.YUV_420, engine=engine) == want
    planes, dims = _rgba_planes(devs)
    out, szs, offs, _, _, _ = engine.encode_ragged_flattened(sj.SRC_RGBA, planes, dims, sj.Flatten(ENC_BG), ENC_SIZES, ENC_ORIENTS,
                                                             sj.YUV_420, _quant(), 4, metadata=metas)
    assert _streams(out, szs, offs) == want
    out, szs, offs, _, _, _ = engine.encode_ragged_flattened_packed(sj.SRC_RGBA, planes, dims, sj.Flatten(ENC_BG), ENC_SIZES, ENC_ORIENTS,
                                                                    sj.YUV_420, _quant(), 4, metadata=metas)
    assert _streams(out, szs, offs.cpu().numpy()) == want


def test_float_pixels_through_the_wrapper(engine, risk_table, batch):
    """Flattened around a FloatPixels of [H, W, 4] half tensors, premultiplied, with an alpha transform of its own"""
    devs, up_dev, up = batch
    made, wants = [], []
    for k, d in enumerate(devs):
        x = d.cpu().numpy()
        p, dev, host = _rgba_on_device(x[..., :3], x[..., 3], "rgba", F16, seed=60 + k, off=k)
        made.append(dev[:, k:])
        s, a = _seen_rgba(host, "rgba", F16)
        wants.append(torch.from_numpy(np.ascontiguousarray(_upright(_area(_flatten(s, a, (0, 0, 0), True), *ENC_SIZES[k]), ENC_ORIENTS[k]))).cuda())
    fp = sj.FloatPixels(made, *XFORM3[F16])
    flat = sj.Flattened(fp, (0, 0, 0), True, *AXFORM[F16], orientations=ENC_ORIENTS, sizes=ENC_SIZES)
    assert sj.encode_images(flat, 75.0, sj.YUV_420, engine=engine, method=4) == sj.encode_images(wants, 75.0, sj.YUV_420, engine=engine, method=4)
    _check_pictures(sj.flatten_images(flat, engine=engine), [w.cpu().numpy() for w in wants])
    assert sj.encode_images_full(flat, engine=engine) == sj.encode_images_full(wants, engine=engine)
    engine.set_pixel_transform(255.0, 0.0)


def test_flatten_none_is_the_oriented_call(engine, batch):
    """flatten None: byte for byte the oriented entry on the same RGBA frames -- the alpha dropped, as today"""
    devs, up_dev, up = batch
    planes, dims = _rgba_planes(devs)
    want = _streams(*engine.encode_ragged_oriented(sj.SRC_RGBA, planes, dims, ENC_SIZES, ENC_ORIENTS, sj.YUV_420, _quant(), 4)[:3])
    assert _streams(*engine.encode_ragged_flattened(sj.SRC_RGBA, planes, dims, None, ENC_SIZES, ENC_ORIENTS, sj.YUV_420, _quant(), 4)[:3]) == want
    out, szs, offs, _, _, _ = engine.encode_ragged_flattened_packed(sj.SRC_RGBA, planes, dims, None, ENC_SIZES, ENC_ORIENTS, sj.YUV_420, _quant(), 4)
    assert _streams(out, szs, offs.cpu().numpy()) == want
    # ... and under flatten there is no pass-through: own sizes, orientation 1 still make F
    rgba = [d.cpu().numpy() for d in devs]
    F = [torch.from_numpy(_flatten(x[..., :3], x[..., 3], ENC_BG, False)).cuda() for x in rgba]
    fplanes, fdims = _rgb_planes(F)
    want = _streams(*engine.encode_ragged_full(sj.SRC_RGB, fplanes, fdims, sj.YUV_420, _quant(), 4)[:3])
    for sizes, orients in ((None, None), (dims, [1] * 3)):
        got = engine.encode_ragged_flattened(sj.SRC_RGBA, planes, dims, sj.Flatten(ENC_BG), sizes, orients, sj.YUV_420, _quant(), 4)
        assert _streams(*got[:3]) == want


def test_two_calls_back_to_back(batch):
    """The second call writes the engine's flattened pictures while the first call's encode may still read them: the
    stream orders the two.  No wait in between; both outputs checked afterwards."""
    devs, up_dev, up = batch
    eng = sj.Engine(0)
    planes, dims = _rgba_planes(devs)
    other = [torch.from_numpy(np.concatenate([synth.g_noise(w, h, 8800 + k), _alphas(w, h, 8810 + k)[3][..., None]], axis=2)).cuda()
             for k, (w, h) in enumerate(ENC_DIMS)]
    oplanes, odims = _rgba_planes(other)
    first = eng.encode_ragged_flattened(sj.SRC_RGBA, planes, dims, sj.Flatten(ENC_BG), ENC_SIZES, ENC_ORIENTS, sj.YUV_420, _quant(), 0)
    second = eng.encode_ragged_flattened(sj.SRC_RGBA, oplanes, odims, sj.Flatten((0, 0, 0), True), ENC_SIZES, ENC_ORIENTS, sj.YUV_420, _quant(), 0)
    got1, got2 = _streams(*first[:3]), _streams(*second[:3])
    assert got1 == sj.encode_images(up_dev, 75.0, sj.YUV_420, engine=eng)
    oup = []
    for o, s, t in zip(other, ENC_SIZES, ENC_ORIENTS):
        x = o.cpu().numpy()
        oup.append(torch.from_numpy(np.ascontiguousarray(_upright(_area(_flatten(x[..., :3], x[..., 3], (0, 0, 0), True), *s), t))).cuda())
    assert got2 == sj.encode_images(oup, 75.0, sj.YUV_420, engine=eng)
    eng.close()


def test_scratch_bytes_and_trim(batch):
    devs, up_dev, up = batch
    eng = sj.Engine(0)
    planes, dims = _rgba_planes(devs)
    uplanes, udims = _rgb_planes(up_dev)
    eng.encode_ragged_full(sj.SRC_RGB, uplanes, udims, sj.YUV_420, _quant(), 4)       # (what the inner call takes is there already)
    torch.cuda.synchronize()
    before = eng.scratch_bytes()
    frames, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
    arr = np.ascontiguousarray(np.asarray(ENC_SIZES, np.int32))
    oarr = np.ascontiguousarray(np.asarray(ENC_ORIENTS, np.uint8))
    need = sj.lib().sjpeg_hip_orient_ragged_bytes(sj.SRC_RGBA, len(dims), frames, arr.ctypes.data, oarr.ctypes.data)
    assert need > 0
    out, szs, offs, _, _, _ = eng.encode_ragged_flattened(sj.SRC_RGBA, planes, dims, sj.Flatten(ENC_BG), ENC_SIZES, ENC_ORIENTS, sj.YUV_420,
                                                          _quant(), 4)
    _streams(out, szs, offs)
    after = eng.scratch_bytes()
    assert after >= before + need
    eng.trim()
    assert eng.scratch_bytes() <= after - need
    eng.close()


# ---- 5. sheets: a 2 x 2 sheet of three RGBA pictures, one smaller than its cell; gutter and margin odd, so spans meet
# inside dwords; the sheet's background is not the flatten's

SHEET_BG, FLAT_BG = (9, 200, 33), (250, 128, 17)


@pytest.fixture(scope="module")
def sheet_batch():
    sheet = sj.Sheet(2, 2, (21, 17), gutter=3, margin=5, background=SHEET_BG)
    dims, orientations = [(37, 23), (9, 7), (40, 64)], [1, 6, 3]
    rgba = [np.concatenate([synth.g_noise(w, h, 8900 + k), _alphas(w, h, 8910 + k)[0 if k != 1 else 3][..., None]], axis=2)
            for k, (w, h) in enumerate(dims)]
    return sheet, dims, orientations, rgba, [torch.from_numpy(x).cuda() for x in rgba]


def _grid(sheet):
    return sheet.cols, sheet.rows, sheet.cell, sheet.gutter, sheet.margin, sheet.background


def test_sheets_against_the_model(engine, risk_table, sheet_batch):
    sheet, dims, orientations, rgba, devs = sheet_batch
    given = sm.fitted_sizes(dims, sheet.cell, orientations)
    assert given[1] == (9, 7)                                            # smaller than its cell: it stays as it is
    planes, _ = _rgba_planes(devs)
    for flatten, bg, pre in ((FLAT_BG, FLAT_BG, False), (sj.Flatten(FLAT_BG, True), FLAT_BG, True), (True, SHEET_BG, False)):
        F = [_flatten(x[..., :3], x[..., 3], bg, pre) for x in rgba]
        wants, where = sm.rgb_sheets(F, *_grid(sheet), given, orientations)
        made = sj.make_sheets(devs, sheet, orientations=orientations, engine=engine, flatten=flatten)
        _check_pictures(made, [np.ascontiguousarray(w) for w in wants])
        assert sj.sheet_places(sheet, dims, sj.SRC_RGBA, None, orientations) == where
        want_dev = [torch.from_numpy(np.ascontiguousarray(w)).cuda() for w in wants]
        want = sj.encode_images_full(want_dev, 75.0, sj.YUV_AUTO, 4, engine=engine)
        for packed in (False, True):
            got, places = sj.encode_sheets(devs, sheet, orientations=orientations, engine=engine, packed=packed, flatten=flatten)
            assert got == want and places == where
    # the engine's entry, on BGRA: the flatten's background beside the sheet's
    bgra = [torch.from_numpy(np.ascontiguousarray(x[..., [2, 1, 0, 3]])).cuda() for x in rgba]
    bplanes, _ = _rgba_planes(bgra)
    F = [_flatten(x[..., :3], x[..., 3], FLAT_BG, False) for x in rgba]
    wants, _ = sm.rgb_sheets(F, *_grid(sheet), given, orientations)
    rfmt, sheets, _ = engine.sheet_ragged(sj.SRC_BGRA, bplanes, dims, sheet, None, orientations, flatten=sj.Flatten(FLAT_BG))
    assert rfmt == sj.SRC_RGB
    _check_pictures(sheets, [np.ascontiguousarray(w) for w in wants])
    # flatten None is today's call: the alpha dropped
    plain, _ = sm.rgb_sheets([x[..., :3] for x in rgba], *_grid(sheet), given, orientations)
    _, sheets, _ = engine.sheet_ragged(sj.SRC_RGBA, planes, dims, sheet, None, orientations)
    _check_pictures(sheets, [np.ascontiguousarray(w) for w in plain])
