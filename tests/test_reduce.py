"""Pictures reduced inside the ragged call on the GPU (sjpeg_hip_reduce_ragged_src, sjpeg_hip_encode_ragged_reduced_src,
Reduced).  The contract is sjpeg_hip.h's: sample (x', y', c) of frame f is (sum + s*s/2) / (s*s) over the s x s box of the
bytes the encoder sees today, the last column and row replicated, and the JPEG is that of the uint8 picture so defined.
Every comparison is exact.  The expected pictures come from _box() and _seen() below (numpy, from what lies on the
device); the expected JPEGs from the existing entry points on those pictures."""
import os

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import synth

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
SIZES = [(1, 1), (2, 3), (7, 5), (8, 8), (9, 16), (17, 9), (31, 33), (63, 65), (130, 70)]
FACTORS = list(range(1, 9))
# per channel, away from ties: fp32 values around -1..1, half values in 0..1 and -1..1, bfloat16 exact small multiples
XFORM3 = {F32: ((127.5, 255.0, 63.75), (127.5, 0.0, 10.0)), F16: ((255.0, 127.5, 255.0), (0.0, 127.5, 0.0)),
          BF16: ((1.0, 2.0, 4.0), (0.0, 1.0, 2.0))}
DMAX = {F32: 0.4, F16: 0.25, BF16: 0.0}
# format -> (memory layout, dtype or None for bytes)
FORMATS = {"RGB": (sj.SRC_RGB, "rgb", None), "BGRA": (sj.SRC_BGRA, "bgra", None), "RGBA": (sj.SRC_RGBA, "rgba", None),
           "RGB_PLANAR": (sj.SRC_RGB_PLANAR, "planar", None), "RGB_PLANAR_F16": (sj.SRC_RGB_PLANAR_F16, "planar", F16),
           "RGB_F32": (sj.SRC_RGB_F32, "rgb", F32), "RGBA_BF16": (sj.SRC_RGBA_BF16, "rgba", BF16),
           "GRAY": (sj.SRC_GRAY, "gray", None), "GRAY_F16": (sj.SRC_GRAY_F16, "gray", F16)}


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.fixture(scope="module")
def risk_table():
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        tab = f.read()
    sj.set_riskiness_table(tab)
    return tab


# ---- the expectation, in numpy

def _box(b, s):
    """The formula of sjpeg_hip.h on a uint8 picture [H, W] or [H, W, C]: edge replication is the min() of the formula."""
    h, w = b.shape[:2]
    h2, w2 = -(-h // s), -(-w // s)
    p = np.pad(b, ((0, h2 * s - h), (0, w2 * s - w)) + ((0, 0),) * (b.ndim - 2), mode="edge").astype(np.int64)
    p = p.reshape((h2, s, w2, s) + b.shape[2:]).sum(axis=(1, 3))
    return ((p + (s * s) // 2) // (s * s)).astype(np.uint8)


def _seen(host, layout, dtype):
    """b(): the bytes the encoder sees of what lies on the device -- `host` is the host copy of the device tensor, laid
    out as `layout` says -- as [H, W, 3] (gray: [H, W]).  Bytes: the R, G and B of each pixel, alpha not part of it.
    Floats: rint(clamp(fma(x, scale[c], bias[c]), 0, 255)) restated in float64 (np.float32 samples: the product is exact
    there), asserted to lie far enough from a tie that the one rounding of the fp32 fma cannot change the byte."""
    if dtype is None:
        if layout == "planar":
            return np.ascontiguousarray(host.transpose(1, 2, 0))
        if layout == "gray":
            return host
        return np.ascontiguousarray(host[..., {"rgb": [0, 1, 2], "rgba": [0, 1, 2], "bgra": [2, 1, 0]}[layout]])
    scale, bias = XFORM3[dtype]
    x = host.astype(np.float32).astype(np.float64)
    if layout == "planar":
        x = x.transpose(1, 2, 0)
    elif layout == "gray":
        x = x[..., None]
    else:
        x = x[..., :3]
    c = x.shape[-1]
    v = x * np.asarray(scale, np.float64)[:c] + np.asarray(bias, np.float64)[:c]
    assert (np.abs(v - np.rint(v)) <= 0.47).all()
    out = np.rint(np.clip(v, 0, 255)).astype(np.uint8)
    return out[..., 0] if layout == "gray" else out


def _on_device(u8, layout, dtype, seed=1, off=0, pad=0):
    """A device tensor holding the uint8 picture u8 [H, W, 3] in `layout` / `dtype` (gray: its G channel), cut out of rows
    `off` + W + `pad` pixels wide; floats are fp32((k + d - bias) / scale) cast to dtype, d uniform within DMAX.  Returns
    (planes entry of the ragged calls, the tensor that owns the memory, the host copy _seen() reads)."""
    h, w = u8.shape[:2]
    k = u8[..., 1] if layout == "gray" else u8
    if dtype is None:
        src = k
    else:
        scale, bias = XFORM3[dtype]
        c = 1 if layout == "gray" else 3
        s, b = np.asarray(scale, np.float64)[:c], np.asarray(bias, np.float64)[:c]
        d = np.random.RandomState(seed).uniform(-DMAX[dtype], DMAX[dtype], k.shape) if DMAX[dtype] > 0 else 0.0
        src = (((k.astype(np.float64) + d).reshape(h, w, c) - b) / s).astype(np.float32).reshape(k.shape)
    tdt = torch.uint8 if dtype is None else dtype
    fill = 77 if dtype is None else float("nan")
    esz = torch.zeros((), dtype=tdt).element_size()
    t = torch.from_numpy(src).to(tdt)
    if layout == "gray":
        buf = torch.full((h, off + w + pad), fill, dtype=tdt)
        buf[:, off:off + w] = t
        dev = buf.cuda()
        view = dev[:, off:off + w]
        return [(view.data_ptr(), dev.stride(0) * esz)], dev, view.cpu().numpy() if dtype is None else view.cpu().to(torch.float32).numpy()
    if layout == "planar":
        buf = torch.full((3, h, off + w + pad), fill, dtype=tdt)
        buf[:, :, off:off + w] = t.permute(2, 0, 1)
        dev = buf.cuda()
        view = dev[:, :, off:off + w]
        planes = [(view[c].data_ptr(), dev.stride(1) * esz) for c in range(3)]
        return planes, dev, view.cpu().numpy() if dtype is None else view.cpu().to(torch.float32).numpy()
    step = 3 if layout == "rgb" else 4
    buf = torch.full((h, off + w + pad, step), fill, dtype=tdt)
    buf[:, off:off + w, :3] = t[..., [2, 1, 0]] if layout == "bgra" else t
    dev = buf.cuda()
    view = dev[:, off:off + w]
    return [(view.data_ptr(), dev.stride(0) * esz)], dev, view.cpu().numpy() if dtype is None else view.cpu().to(torch.float32).numpy()


def _ties(w, h, s, seed):
    """A picture whose s x s boxes sum exactly to a tie of the rounding -- sum + s*s/2 a multiple of s*s -- or to one
    below it, alternating: the two sides of every rounding step."""
    rs = np.random.RandomState(seed)
    n = s * s
    h2, w2 = -(-h // s), -(-w // s)
    m = rs.randint(1, 256, (h2, w2, 3))
    total = m * n - n // 2 - ((np.arange(h2)[:, None, None] + np.arange(w2)[None, :, None] + np.arange(3)) & 1)
    base, rem = total // n, total % n
    cell = np.arange(n).reshape(1, s, 1, s, 1)
    img = base[:, None, :, None, :] + (cell < rem[:, None, :, None, :])
    assert img.min() >= 0 and img.max() <= 255
    assert (img.sum(axis=(1, 3)) == total).all()
    return np.ascontiguousarray(img.reshape(h2 * s, w2 * s, 3)[:h, :w].astype(np.uint8))


@pytest.fixture(scope="module")
def sources():
    """The uint8 pictures of the kernel tests, one per content, size and factor: (u8 [H, W, 3], factor).  Never written to."""
    out = []
    for ci in range(3):
        for si, (w, h) in enumerate(SIZES):
            for s in FACTORS:
                if ci == 0:
                    im = synth.g_noise(w, h, 9000 + 16 * si + s)
                elif ci == 1:
                    im = np.full((h, w, 3), 255, np.uint8)
                else:
                    im = _ties(w, h, s, 9500 + 16 * si + s)
                out.append((im, s))
    return out


def _check_pictures(pics, wants):
    torch.cuda.synchronize()
    assert len(pics) == len(wants)
    for k, (p, want) in enumerate(zip(pics, wants)):
        got = p.cpu().numpy()
        assert got.shape == want.shape, (k, got.shape, want.shape)
        assert np.array_equal(got, want), (k, want.shape, np.argwhere(got != want)[:4])


# ---- 1. the kernel alone: ONE ragged call per format over every size, factor and content

@pytest.mark.parametrize("name", list(FORMATS))
def test_reduce_ragged_against_numpy(engine, sources, name):
    fmt, layout, dtype = FORMATS[name]
    if dtype is not None:
        engine.set_pixel_transform(*XFORM3[dtype])
    planes, keep, wants, dims, factors = [], [], [], [], []
    for k, (u8, s) in enumerate(sources):
        p, dev, host = _on_device(u8, layout, dtype, seed=k, off=k % 3, pad=(k // 3) % 2)
        seen = _seen(host, layout, dtype)
        assert np.array_equal(seen, u8[..., 1] if layout == "gray" else u8)     # (the construction and b() agree)
        planes.append(p); keep.append(dev)
        wants.append(_box(seen, s)); dims.append((u8.shape[1], u8.shape[0])); factors.append(s)
    rfmt, pics, buf = engine.reduce_ragged(fmt, planes, dims, factors)
    assert rfmt == (sj.SRC_GRAY if layout == "gray" else sj.SRC_RGB)
    for p, (w, h), s in zip(pics, dims, factors):
        assert (p.shape[1], p.shape[0]) == sj.reduced_size(w, h, s)
        assert p.data_ptr() % 16 == 0 and p.stride(0) % 4 == 0
    _check_pictures(pics, wants)
    engine.set_pixel_transform(255.0, 0.0)


# ---- 2. strides and bounds

def test_negative_row_stride(engine):
    ims = [synth.g_noise(w, h, 9700 + k) for k, (w, h) in enumerate([(17, 9), (63, 65), (130, 70)])]
    factors = [8, 3, 2]
    devs = [torch.from_numpy(np.ascontiguousarray(im[::-1])).cuda() for im in ims]         # stored bottom-up
    planes = [[(d.data_ptr() + (d.shape[0] - 1) * d.stride(0), -d.stride(0))] for d in devs]
    _, pics, _ = engine.reduce_ragged(sj.SRC_RGB, planes, [(im.shape[1], im.shape[0]) for im in ims], factors)
    _check_pictures(pics, [_box(im, s) for im, s in zip(ims, factors)])


def test_odd_column_crop_of_a_wider_float_tensor(engine):
    """element-only alignment: the crop starts 3 halfs (6 bytes) into the row, the gray one 1 half"""
    engine.set_pixel_transform(*XFORM3[F16])
    u8 = synth.g_noise(31, 33, 9710)
    for fmt, layout in ((sj.SRC_RGB_F16, "rgb"), (sj.SRC_GRAY_F16, "gray"), (sj.SRC_RGB_PLANAR_F16, "planar")):
        p, dev, host = _on_device(u8, layout, F16, seed=3, off=1, pad=2)
        assert p[0][0] % 4 == 2
        seen = _seen(host, layout, F16)
        _, pics, _ = engine.reduce_ragged(fmt, [p] * 3, [(31, 33)] * 3, [1, 2, 5])
        _check_pictures(pics, [_box(seen, s) for s in (1, 2, 5)])
    engine.set_pixel_transform(255.0, 0.0)


def test_rgb_of_an_argb_half_tensor(engine):
    """x[..., 1:4] of an ARGB tensor is an RGBA source whose last "alpha" lies outside the allocation: never read"""
    engine.set_pixel_transform(*XFORM3[F16])
    u8 = synth.g_noise(17, 9, 9720)
    _, _, host = _on_device(u8, "rgb", F16, seed=5)
    argb = torch.full((9, 17, 4), float("nan"), dtype=F16)
    argb[..., 1:4] = torch.from_numpy(host).to(F16)
    dev = argb.cuda()
    view = dev[..., 1:4]
    assert view.data_ptr() + ((9 * 17 - 1) * 4 + 4) * 2 > dev.data_ptr() + dev.numel() * 2
    seen = _seen(view.cpu().to(torch.float32).numpy(), "rgb", F16)
    assert np.array_equal(seen, u8)
    _, pics, _ = engine.reduce_ragged(sj.SRC_RGBA_F16, [[(view.data_ptr(), dev.stride(0) * 2)]] * 4, [(17, 9)] * 4, [1, 2, 8, 3])
    _check_pictures(pics, [_box(seen, s) for s in (1, 2, 8, 3)])
    engine.set_pixel_transform(255.0, 0.0)


@pytest.mark.parametrize("fmt,layout", [(sj.SRC_RGB, "rgb"), (sj.SRC_GRAY, "gray")])
def test_guard_bytes_around_the_reduced_buffer(engine, fmt, layout):
    dims, factors = [(17, 9), (1, 1), (130, 70), (9, 16), (63, 65)], [8, 1, 3, 2, 1]
    ims = [synth.g_noise(w, h, 9730 + k) for k, (w, h) in enumerate(dims)]
    made = [_on_device(im, layout, None) for im in ims]
    frames, _, _, _ = sj._ragged_frames([m[0] for m in made], dims, None, None, None, None)
    fac = (sj.C.c_uint8 * len(dims))(*factors)
    need = sj.lib().sjpeg_hip_reduce_ragged_bytes(fmt, len(dims), frames, sj.C.cast(fac, sj.C.c_void_p))
    assert need > 0 and need % 16 == 0
    guard = 256
    whole = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    _, pics, _ = engine.reduce_ragged(fmt, [m[0] for m in made], dims, factors, out=whole[guard:guard + need])
    _check_pictures(pics, [_box(_seen(m[2], layout, None), s) for m, s in zip(made, factors)])
    host = whole.cpu().numpy()
    assert (host[:guard] == 0xA5).all() and (host[guard + need:] == 0xA5).all()
    # one byte short is refused before anything runs
    with pytest.raises(sj.SjpegError):
        engine.reduce_ragged(fmt, [m[0] for m in made], dims, factors, out=whole[guard:guard + need - 16][:need - 1])


# ---- 3. encode: each against the existing entry on the numpy-reduced pictures

ENC_DIMS = [(17, 9), (31, 33), (63, 65), (130, 70), (8, 8)]
ENC_FACTORS = [2, 1, 3, 8, 4]


@pytest.fixture(scope="module")
def batch():
    """(device pictures [H, W, 3], their factors, the numpy-reduced pictures on the device and on the host)"""
    ims = [synth.g_struct(w, h, 9800 + k) if k % 2 else synth.g_noise(w, h, 9800 + k) for k, (w, h) in enumerate(ENC_DIMS)]
    small = [_box(im, s) for im, s in zip(ims, ENC_FACTORS)]
    return [torch.from_numpy(im).cuda() for im in ims], ENC_FACTORS, [torch.from_numpy(x).cuda() for x in small], small


def _quant(q=75.0):
    m = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(float(q), m.ctypes.data)
    return m


def _rgb_planes(devs):
    return [[d.as_strided((d.shape[0], d.shape[1] * 3), (d.stride(0), 1))] for d in devs], [(d.shape[1], d.shape[0]) for d in devs]


def _streams(out, sizes, offs):
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    assert (sz > 0).all()
    return [host[int(offs[k]):int(offs[k]) + int(sz[k])].tobytes() for k in range(len(sz))]


def test_method_0_and_the_oracle(engine, oracle, batch):
    devs, factors, small_dev, small = batch
    got = sj.encode_images(sj.Reduced(devs, factors), 80.0, sj.YUV_420, engine=engine)
    assert got == sj.encode_images(small_dev, 80.0, sj.YUV_420, engine=engine)
    assert got == [oracle.encode(x, 80.0, sj.YUV_420) for x in small]
    # per-picture quality and 4:4:4, one int factor
    qs = [60.0, 75.0, 90.0, 50.0, 85.0]
    half = [torch.from_numpy(_box(d.cpu().numpy(), 2)).cuda() for d in devs]
    assert sj.encode_images(sj.Reduced(devs, 2), qs, sj.YUV_444, engine=engine) == sj.encode_images(half, qs, sj.YUV_444, engine=engine)


def test_method_4_through_the_engine_entry(engine, batch):
    devs, factors, small_dev, small = batch
    planes, dims = _rgb_planes(devs)
    out, sizes, offs, modes, _, _ = engine.encode_ragged_reduced(sj.SRC_RGB, planes, dims, factors, sj.YUV_420, _quant(), 4)
    got = _streams(out, sizes, offs)
    assert got == sj.encode_images(small_dev, 75.0, sj.YUV_420, engine=engine, method=4)
    assert modes == [sj.YUV_420] * len(devs)
    assert got == sj.encode_images(sj.Reduced(devs, factors), 75.0, sj.YUV_420, engine=engine, method=4)


def test_compress_images_decides_on_the_reduced_picture(engine, risk_table, batch):
    devs, factors, small_dev, small = batch
    # a picture that is risky at full size and one more: the verdicts are those of the reduced pictures
    sharp = torch.from_numpy(synth.g_struct(130, 70, 9850)).cuda()
    ims, fs = devs + [sharp], factors + [2]
    red = small_dev + [torch.from_numpy(_box(sharp.cpu().numpy(), 2)).cuda()]
    assert sj.compress_images(sj.Reduced(ims, fs), 75.0, engine=engine) == sj.compress_images(red, 75.0, engine=engine)
    planes, dims = _rgb_planes(ims)
    out, sizes, offs, modes, _, _ = engine.encode_ragged_reduced(sj.SRC_RGB, planes, dims, fs, sj.YUV_AUTO, _quant(), 4)
    rplanes, rdims = _rgb_planes(red)
    out2, sizes2, offs2, modes2, _, _ = engine.encode_ragged_full(sj.SRC_RGB, rplanes, rdims, sj.YUV_AUTO, _quant(), 4)
    assert modes == modes2 == [sj.riskiness_verdict(s, w, h)[0] for s, (w, h) in
                               zip(engine.riskiness_ragged(sj.SRC_RGB, rplanes, rdims).cpu().numpy(), rdims)]
    assert _streams(out, sizes, offs) == _streams(out2, sizes2, offs2)


def test_target_size_search(engine, batch):
    devs, factors, small_dev, small = batch
    targets = [max(400, x.size // 6) for x in small]
    got = sj.encode_images(sj.Reduced(devs, factors), 75.0, sj.YUV_420, engine=engine, method=4, target_size=targets)
    assert got == sj.encode_images(small_dev, 75.0, sj.YUV_420, engine=engine, method=4, target_size=targets)
    planes, dims = _rgb_planes(devs)
    search = [dict(target_mode=sj.TARGET_SIZE, target_value=t) for t in targets]
    out, sizes, offs, _, q, v = engine.encode_ragged_reduced(sj.SRC_RGB, planes, dims, factors, sj.YUV_420, _quant(), 4, search=search)
    assert _streams(out, sizes, offs) == got
    rplanes, rdims = _rgb_planes(small_dev)
    _, _, _, _, q2, v2 = engine.encode_ragged_full(sj.SRC_RGB, rplanes, rdims, sj.YUV_420, _quant(), 4, search=search)
    torch.cuda.synchronize()
    assert q == q2 and v == v2


def test_method_7_on_two_tiny_pictures(engine, batch):
    devs, factors, small_dev, small = batch
    got = sj.encode_images(sj.Reduced(devs[:2], factors[:2]), 75.0, sj.YUV_420, engine=engine, method=4, use_trellis=True)
    assert got == sj.encode_images(small_dev[:2], 75.0, sj.YUV_420, engine=engine, method=4, use_trellis=True)


def test_packed(engine, batch):
    devs, factors, small_dev, small = batch
    want = sj.encode_images(small_dev, 75.0, sj.YUV_444, engine=engine, method=4)
    assert sj.encode_images(sj.Reduced(devs, factors), 75.0, sj.YUV_444, engine=engine, method=4, packed=True) == want
    planes, dims = _rgb_planes(devs)
    out, sizes, offs, modes, _, _ = engine.encode_ragged_reduced_packed(sj.SRC_RGB, planes, dims, factors, sj.YUV_444, _quant(), 4)
    torch.cuda.synchronize()
    o, sz, host = offs.cpu().numpy(), sizes.cpu().numpy(), out.cpu().numpy()
    assert (sz > 0).all() and (o[:-1] % 16 == 0).all()
    assert list(o[:-1]) == sorted(o[:-1]) and len(set(o[:-1])) == len(devs)        # ascending in the caller's order
    assert o[-1] == sum((int(s) + 15) & ~15 for s in sz)
    assert [host[int(o[k]):int(o[k]) + int(sz[k])].tobytes() for k in range(len(devs))] == want


def test_metadata_with_a_size_target(engine, batch):
    devs, factors, small_dev, small = batch
    metas = [sj.PictureMetadata(exif=b"Exif\0\0" + bytes(range(40)) * (k + 1)) if k % 2 == 0 else None for k in range(len(devs))]
    metas[3] = sj.PictureMetadata(xmp=b"<x:xmpmeta>reduced</x:xmpmeta>", app_markers=b"\xff\xe5\x00\x06abcd")
    targets = [max(600, x.size // 5) for x in small]
    want = sj.encode_images_full_meta(small_dev, metas, yuv_mode=sj.YUV_420, target_size=targets, engine=engine)
    assert sj.encode_images_full_meta(sj.Reduced(devs, factors), metas, yuv_mode=sj.YUV_420, target_size=targets, engine=engine) == want
    planes, dims = _rgb_planes(devs)
    search = [dict(target_mode=sj.TARGET_SIZE, target_value=t) for t in targets]
    out, sizes, offs, _, _, _ = engine.encode_ragged_reduced(sj.SRC_RGB, planes, dims, factors, sj.YUV_420, _quant(), 4, search=search,
                                                             metadata=metas)
    assert _streams(out, sizes, offs) == want
    out, sizes, offs, _, _, _ = engine.encode_ragged_reduced_packed(sj.SRC_RGB, planes, dims, factors, sj.YUV_420, _quant(), 4,
                                                                    search=search, metadata=metas)
    assert _streams(out, sizes, offs.cpu().numpy()) == want


def test_float_pixels_and_chw(engine, batch):
    """Reduced around a FloatPixels, layout="chw": the transform is read before the boxes are summed"""
    devs, factors, small_dev, small = batch
    made = [_on_device(d.cpu().numpy(), "planar", F16, seed=40 + k) for k, d in enumerate(devs)]
    fp = sj.FloatPixels([m[1] for m in made], *XFORM3[F16])
    got = sj.encode_images(sj.Reduced(fp, factors), 75.0, sj.YUV_420, engine=engine, method=4, layout="chw")
    assert got == sj.encode_images(small_dev, 75.0, sj.YUV_420, engine=engine, method=4)
    pics = sj.reduce_images(fp, factors, engine=engine, layout="chw")
    _check_pictures([p.permute(1, 2, 0) for p in pics], small)
    assert sj.encode_images_full_chw(pics, 75.0, sj.YUV_444, engine=engine) == sj.encode_images_full(small_dev, 75.0, sj.YUV_444, engine=engine)
    engine.set_pixel_transform(255.0, 0.0)


# ---- 4. all factors 1, a pyramid, two calls back to back, the engine's memory

def test_all_factors_1_is_the_plain_call(engine, batch):
    devs = batch[0]
    want = sj.encode_images(devs, 75.0, sj.YUV_420, engine=engine, method=4)
    assert sj.encode_images(sj.Reduced(devs, 1), 75.0, sj.YUV_420, engine=engine, method=4) == want
    planes, dims = _rgb_planes(devs)
    out, sizes, offs, _, _, _ = engine.encode_ragged_full(sj.SRC_RGB, planes, dims, sj.YUV_420, _quant(), 4)
    assert _streams(out, sizes, offs) == want
    before = engine.scratch_bytes()                  # (what the plain _full_ call holds)
    for factors in ([1] * len(devs), None):
        out, sizes, offs, _, _, _ = engine.encode_ragged_reduced(sj.SRC_RGB, planes, dims, factors, sj.YUV_420, _quant(), 4)
        assert _streams(out, sizes, offs) == want
    assert engine.scratch_bytes() == before          # no copy: nothing was allocated for reduced pictures
    # an NV12 batch passes with factors of 1
    rs = np.random.RandomState(9900)
    nv, nvdims = [], [(34, 18), (17, 9)]
    for (w, h) in nvdims:
        nv.append([torch.from_numpy(rs.randint(0, 256, (h, w)).astype(np.uint8)).cuda(),
                   torch.from_numpy(rs.randint(0, 256, ((h + 1) // 2, 2 * ((w + 1) // 2))).astype(np.uint8)).cuda()])
    out, sizes, offs, _, _, _ = engine.encode_ragged_reduced(sj.SRC_NV12, nv, nvdims, [1, 1], sj.YUV_420, _quant(), 4)
    out2, sizes2, offs2, _, _, _ = engine.encode_ragged_full(sj.SRC_NV12, nv, nvdims, sj.YUV_420, _quant(), 4)
    assert _streams(out, sizes, offs) == _streams(out2, sizes2, offs2)
    with pytest.raises(sj.SjpegError, match="SJPEG_HIP_SRC_NV12"):
        engine.encode_ragged_reduced(sj.SRC_NV12, nv, nvdims, [1, 2], sj.YUV_420, _quant(), 4)


def test_pyramid(engine):
    im = synth.g_struct(130, 70, 9910)
    dev = torch.from_numpy(im).cuda()
    levels = [1, 2, 4, 8]
    want = [_box(im, s) for s in levels]
    assert [w.shape[:2] for w in want] == [(70, 130), (35, 65), (18, 33), (9, 17)]
    _check_pictures(sj.reduce_images([dev] * 4, levels, engine=engine), want)
    got = sj.encode_images(sj.Reduced([dev] * 4, levels), 85.0, sj.YUV_444, engine=engine, method=4)
    for k, w in enumerate(want):
        assert got[k] == sj.encode_images([torch.from_numpy(w).cuda()], 85.0, sj.YUV_444, engine=engine, method=4)[0], levels[k]


def test_two_calls_back_to_back(batch):
    """The second call writes the engine's reduced pictures while the first call's encode may still read them: the
    stream orders the two.  No wait in between; both outputs checked afterwards."""
    devs, factors, small_dev, small = batch
    eng = sj.Engine(0)
    planes, dims = _rgb_planes(devs)
    other = [torch.from_numpy(synth.g_noise(w, h, 9920 + k)).cuda() for k, (w, h) in enumerate(ENC_DIMS)]
    oplanes, odims = _rgb_planes(other)
    first = eng.encode_ragged_reduced(sj.SRC_RGB, planes, dims, factors, sj.YUV_420, _quant(), 0)
    second = eng.encode_ragged_reduced(sj.SRC_RGB, oplanes, odims, factors, sj.YUV_420, _quant(), 0)
    got1, got2 = _streams(*first[:3]), _streams(*second[:3])
    assert got1 == sj.encode_images(small_dev, 75.0, sj.YUV_420, engine=eng)
    osmall = [torch.from_numpy(_box(o.cpu().numpy(), s)).cuda() for o, s in zip(other, factors)]
    assert got2 == sj.encode_images(osmall, 75.0, sj.YUV_420, engine=eng)
    eng.close()


def test_scratch_bytes_and_trim(batch):
    devs, factors, small_dev, small = batch
    eng = sj.Engine(0)
    planes, dims = _rgb_planes(devs)
    # the plain call on the reduced pictures first: what the inner call takes is there already
    rplanes, rdims = _rgb_planes(small_dev)
    eng.encode_ragged_full(sj.SRC_RGB, rplanes, rdims, sj.YUV_420, _quant(), 4)
    torch.cuda.synchronize()
    before = eng.scratch_bytes()
    frames, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
    fac = (sj.C.c_uint8 * len(dims))(*factors)
    need = sj.lib().sjpeg_hip_reduce_ragged_bytes(sj.SRC_RGB, len(dims), frames, sj.C.cast(fac, sj.C.c_void_p))
    out, sizes, offs, _, _, _ = eng.encode_ragged_reduced(sj.SRC_RGB, planes, dims, factors, sj.YUV_420, _quant(), 4)
    _streams(out, sizes, offs)
    after = eng.scratch_bytes()
    assert after >= before + need
    assert need <= sum(d.numel() for d in devs) + 19 * sum(-(-d.shape[0] // s) for d, s in zip(devs, factors))   # (the sources' size at most, plus padding)
    eng.trim()
    assert eng.scratch_bytes() <= after - need
    eng.close()
