"""Pictures resized inside the ragged call on the GPU (sjpeg_hip_resize_ragged_src, sjpeg_hip_encode_ragged_resized_src,
Resized).  The contract is sjpeg_hip.h's: a sample of the resized picture is the exact area average of the bytes the
encoder sees today -- (2 S + W H) / (2 W H) with S the sum weighted by the overlaps wy and wx --, and the JPEG is that of
the uint8 picture so defined.  Every comparison is exact.  The expected pictures come from _area() below (numpy int64:
Wy @ picture @ Wx^T, then the rounding) on what _seen() of tests/test_reduce.py reads on the device; the expected JPEGs
from the existing entry points on those pictures."""
import os

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import synth
from test_reduce import F16, FORMATS, XFORM3, _box, _check_pictures, _on_device, _quant, _rgb_planes, _seen, _streams

pytestmark = pytest.mark.gpu

# source -> target.  The issue's: 1 x 1, sides that halve unevenly, the identity, a support of 2 with weights that differ
# per column, one axis kept and one almost, a support of 44, a row wider than one workgroup's span and a segment longer
# than a small tile.  And two of ours, where the kernel takes its other path: a cell's row of source columns longer than
# the rows the kernel stages at once (5460 pixels of RGB, 16384 of gray), which it then stages in pieces.
SHAPES = [((1, 1), (1, 1)), ((2, 3), (1, 2)), ((7, 5), (3, 2)), ((8, 8), (8, 8)), ((17, 9), (16, 9)), ((63, 65), (5, 64)),
          ((130, 70), (129, 1)), ((300, 40), (7, 3)), ((1030, 9), (1029, 8)), ((1030, 9), (3, 2)),
          ((6000, 2), (1, 1)), ((17000, 3), (2, 2))]


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

def _weights(n_src, n_dst):
    """wx of sjpeg_hip.h as a matrix [n_dst, n_src]"""
    x, xo = np.arange(n_src, dtype=np.int64)[None, :], np.arange(n_dst, dtype=np.int64)[:, None]
    w = np.maximum(0, np.minimum((x + 1) * n_dst, (xo + 1) * n_src) - np.maximum(x * n_dst, xo * n_src))
    assert (w.sum(axis=1) == n_src).all()
    return w


def _area(b, w2, h2):
    """The formula of sjpeg_hip.h on a uint8 picture [H, W] or [H, W, C]"""
    H, W = b.shape[:2]
    wy, wx = _weights(H, h2), _weights(W, w2)
    p = b.astype(np.int64).reshape(H, W, -1)
    S = np.stack([(wy @ p[..., c]) @ wx.T for c in range(p.shape[2])], axis=-1)
    assert S.max() <= 255 * W * H
    out = (2 * S + W * H) // (2 * W * H)
    return out.astype(np.uint8).reshape((h2, w2) + b.shape[2:])


@pytest.fixture(scope="module")
def sources():
    """The uint8 pictures of the kernel tests: (u8 [H, W, 3], (w', h')), noise and all 255 for every shape.  Never
    written to."""
    out = []
    for k, ((w, h), size) in enumerate(SHAPES):
        out.append((synth.g_noise(w, h, 9100 + k), size))
        out.append((np.full((h, w, 3), 255, np.uint8), size))
    return out


def test_the_expectation_itself():
    """_area() on pictures whose answer is known: a constant stays, the identity stays, an even split is the mean"""
    rs = np.random.RandomState(1)
    im = rs.randint(0, 256, (9, 17, 3)).astype(np.uint8)
    assert np.array_equal(_area(im, 17, 9), im)
    assert (_area(np.full((40, 300), 201, np.uint8), 7, 3) == 201).all()
    assert _area(np.array([[1, 2], [3, 4]], np.uint8), 1, 1)[0, 0] == 3          # 2.5 rounds up
    # 3 -> 2: the middle sample is shared half and half: (2 a + b) / 3, (b + 2 c) / 3
    assert list(_area(np.array([[30, 60, 90]], np.uint8), 2, 1)[0]) == [40, 80]
    for s in (2, 3, 8):
        assert np.array_equal(_area(im[:8 // s * s, :16 // s * s], 16 // s, 8 // s), _box(im[:8 // s * s, :16 // s * s], s))


# ---- 1. the kernel alone: ONE ragged call per format over every shape and content

@pytest.mark.parametrize("name", list(FORMATS))
def test_resize_ragged_against_numpy(engine, sources, name):
    fmt, layout, dtype = FORMATS[name]
    if dtype is not None:
        engine.set_pixel_transform(*XFORM3[dtype])
    planes, keep, wants, dims, sizes = [], [], [], [], []
    for k, (u8, size) in enumerate(sources):
        p, dev, host = _on_device(u8, layout, dtype, seed=k, off=k % 3, pad=(k // 3) % 2)
        seen = _seen(host, layout, dtype)
        assert np.array_equal(seen, u8[..., 1] if layout == "gray" else u8)     # (the construction and b() agree)
        planes.append(p); keep.append(dev)
        wants.append(_area(seen, *size)); dims.append((u8.shape[1], u8.shape[0])); sizes.append(size)
    rfmt, pics, buf = engine.resize_ragged(fmt, planes, dims, sizes)
    assert rfmt == (sj.SRC_GRAY if layout == "gray" else sj.SRC_RGB)
    for p, size in zip(pics, sizes):
        assert (p.shape[1], p.shape[0]) == size
        assert p.data_ptr() % 16 == 0 and p.stride(0) % 4 == 0
    _check_pictures(pics, wants)
    engine.set_pixel_transform(255.0, 0.0)


def test_whole_factors_equal_the_reduction(engine):
    """W = s w' and H = s h': the existing reduction by s, byte for byte, for every s"""
    ims, factors = [], []
    for s in range(1, 9):
        for (w, h) in ((3 * s, 5 * s), (16 * s, 9 * s)):
            ims.append(torch.from_numpy(synth.g_noise(w, h, 9200 + 8 * s + w % 7)).cuda())
            factors.append(s)
    sizes = [(im.shape[1] // s, im.shape[0] // s) for im, s in zip(ims, factors)]
    got = sj.resize_images(ims, sizes, engine=engine)
    want = sj.reduce_images(ims, factors, engine=engine)
    _check_pictures(got, [w.cpu().numpy() for w in want])
    _check_pictures(got, [_box(im.cpu().numpy(), s) for im, s in zip(ims, factors)])


# ---- 2. strides and bounds

def test_negative_row_stride(engine):
    dims, sizes = [(17, 9), (63, 65), (300, 40)], [(16, 9), (5, 64), (7, 3)]
    ims = [synth.g_noise(w, h, 9300 + k) for k, (w, h) in enumerate(dims)]
    devs = [torch.from_numpy(np.ascontiguousarray(im[::-1])).cuda() for im in ims]         # stored bottom-up
    planes = [[(d.data_ptr() + (d.shape[0] - 1) * d.stride(0), -d.stride(0))] for d in devs]
    _, pics, _ = engine.resize_ragged(sj.SRC_RGB, planes, dims, sizes)
    _check_pictures(pics, [_area(im, *s) for im, s in zip(ims, sizes)])


def test_odd_column_crop_of_a_wider_float_tensor(engine):
    """element-only alignment: the crop starts 3 halfs (6 bytes) into the row, the gray one 1 half"""
    engine.set_pixel_transform(*XFORM3[F16])
    u8 = synth.g_noise(31, 33, 9310)
    sizes = [(31, 33), (30, 17), (4, 5)]
    for fmt, layout in ((sj.SRC_RGB_F16, "rgb"), (sj.SRC_GRAY_F16, "gray"), (sj.SRC_RGB_PLANAR_F16, "planar")):
        p, dev, host = _on_device(u8, layout, F16, seed=3, off=1, pad=2)
        assert p[0][0] % 4 == 2
        seen = _seen(host, layout, F16)
        _, pics, _ = engine.resize_ragged(fmt, [p] * 3, [(31, 33)] * 3, sizes)
        _check_pictures(pics, [_area(seen, *s) for s in sizes])
    engine.set_pixel_transform(255.0, 0.0)


def test_rgb_of_an_argb_half_tensor(engine):
    """x[..., 1:4] of an ARGB tensor is an RGBA source whose last "alpha" lies outside the allocation: never read"""
    engine.set_pixel_transform(*XFORM3[F16])
    u8 = synth.g_noise(17, 9, 9320)
    _, _, host = _on_device(u8, "rgb", F16, seed=5)
    argb = torch.full((9, 17, 4), float("nan"), dtype=F16)
    argb[..., 1:4] = torch.from_numpy(host).to(F16)
    dev = argb.cuda()
    view = dev[..., 1:4]
    assert view.data_ptr() + ((9 * 17 - 1) * 4 + 4) * 2 > dev.data_ptr() + dev.numel() * 2
    seen = _seen(view.cpu().to(torch.float32).numpy(), "rgb", F16)
    assert np.array_equal(seen, u8)
    sizes = [(17, 9), (16, 9), (1, 1), (5, 8)]
    _, pics, _ = engine.resize_ragged(sj.SRC_RGBA_F16, [[(view.data_ptr(), dev.stride(0) * 2)]] * 4, [(17, 9)] * 4, sizes)
    _check_pictures(pics, [_area(seen, *s) for s in sizes])
    engine.set_pixel_transform(255.0, 0.0)


@pytest.mark.parametrize("fmt,layout", [(sj.SRC_RGB, "rgb"), (sj.SRC_GRAY, "gray")])
def test_guard_bytes_around_the_resized_buffer(engine, fmt, layout):
    dims = [(17, 9), (1, 1), (130, 70), (300, 40), (1030, 9), (63, 65)]
    sizes = [(16, 9), (1, 1), (129, 1), (7, 3), (1029, 8), (5, 64)]
    ims = [synth.g_noise(w, h, 9330 + k) for k, (w, h) in enumerate(dims)]
    made = [_on_device(im, layout, None) for im in ims]
    frames, _, _, _ = sj._ragged_frames([m[0] for m in made], dims, None, None, None, None)
    arr = np.ascontiguousarray(np.asarray(sizes, np.int32))
    need = sj.lib().sjpeg_hip_resize_ragged_bytes(fmt, len(dims), frames, arr.ctypes.data)
    assert need > 0 and need % 16 == 0
    guard = 256
    whole = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    _, pics, _ = engine.resize_ragged(fmt, [m[0] for m in made], dims, sizes, out=whole[guard:guard + need])
    _check_pictures(pics, [_area(_seen(m[2], layout, None), *s) for m, s in zip(made, sizes)])
    host = whole.cpu().numpy()
    assert (host[:guard] == 0xA5).all() and (host[guard + need:] == 0xA5).all()
    # one byte short is refused before anything runs
    with pytest.raises(sj.SjpegError, match="resized_bytes"):
        engine.resize_ragged(fmt, [m[0] for m in made], dims, sizes, out=whole[guard:guard + need - 16][:need - 1])


def test_sums_past_32_bits(engine):
    """A gray 4099 x 4111 picture of bytes in 200..255 made 3 x 3 and 4098 x 2: the numerator 2 S + W H of the rounding
    passes 2^32 at every sample (S is about 228 W H = 3.8e9), and S itself does on the same shape filled with 255
    (255 * 4099 * 4111 = 2^32 + 2 034 899) -- which the 64-bit sums and the division have to hold"""
    im = np.random.RandomState(9400).randint(200, 256, (4111, 4099)).astype(np.uint8)
    assert 2 * 200 * 4099 * 4111 > 2 ** 32 and 255 * 4099 * 4111 > 2 ** 32
    dev, full = torch.from_numpy(im).cuda(), torch.full((4111, 4099), 255, dtype=torch.uint8, device="cuda")
    sizes = [(3, 3), (4098, 2), (3, 3)]
    _, pics, _ = engine.resize_ragged(sj.SRC_GRAY, [[dev], [dev], [full]], [(4099, 4111)] * 3, sizes)
    _check_pictures(pics, [_area(im, 3, 3), _area(im, 4098, 2), np.full((3, 3), 255, np.uint8)])


# ---- 3. encode: each against the existing entry on the numpy-resized pictures

ENC_DIMS = [(17, 9), (31, 33), (63, 65), (130, 70), (8, 8)]
ENC_SIZES = [(16, 9), (10, 33), (5, 64), (40, 21), (8, 8)]


@pytest.fixture(scope="module")
def batch():
    """(device pictures [H, W, 3], their sizes, the numpy-resized pictures on the device and on the host)"""
    ims = [synth.g_struct(w, h, 9500 + k) if k % 2 else synth.g_noise(w, h, 9500 + k) for k, (w, h) in enumerate(ENC_DIMS)]
    small = [_area(im, *s) for im, s in zip(ims, ENC_SIZES)]
    return [torch.from_numpy(im).cuda() for im in ims], ENC_SIZES, [torch.from_numpy(x).cuda() for x in small], small


def test_method_0_and_the_oracle(engine, oracle, batch):
    devs, sizes, small_dev, small = batch
    got = sj.encode_images(sj.Resized(devs, sizes), 80.0, sj.YUV_420, engine=engine)
    assert got == sj.encode_images(small_dev, 80.0, sj.YUV_420, engine=engine)
    assert got == [oracle.encode(x, 80.0, sj.YUV_420) for x in small]
    # per-picture quality and 4:4:4, one size for all
    qs = [60.0, 75.0, 90.0, 50.0, 85.0]
    tiny = [torch.from_numpy(_area(d.cpu().numpy(), 5, 7)).cuda() for d in devs]
    assert sj.encode_images(sj.Resized(devs, (5, 7)), qs, sj.YUV_444, engine=engine) == sj.encode_images(tiny, qs, sj.YUV_444, engine=engine)


def test_method_4_through_the_engine_entry(engine, batch):
    devs, sizes, small_dev, small = batch
    planes, dims = _rgb_planes(devs)
    out, szs, offs, modes, _, _ = engine.encode_ragged_resized(sj.SRC_RGB, planes, dims, sizes, sj.YUV_420, _quant(), 4)
    got = _streams(out, szs, offs)
    assert got == sj.encode_images(small_dev, 75.0, sj.YUV_420, engine=engine, method=4)
    assert modes == [sj.YUV_420] * len(devs)
    assert got == sj.encode_images(sj.Resized(devs, sizes), 75.0, sj.YUV_420, engine=engine, method=4)


def test_compress_images_decides_on_the_resized_picture(engine, risk_table, batch):
    devs, sizes, small_dev, small = batch
    sharp = torch.from_numpy(synth.g_struct(130, 70, 9550)).cuda()
    ims, ss = devs + [sharp], sizes + [(64, 35)]
    res = small_dev + [torch.from_numpy(_area(sharp.cpu().numpy(), 64, 35)).cuda()]
    assert sj.compress_images(sj.Resized(ims, ss), 75.0, engine=engine) == sj.compress_images(res, 75.0, engine=engine)
    planes, dims = _rgb_planes(ims)
    out, szs, offs, modes, _, _ = engine.encode_ragged_resized(sj.SRC_RGB, planes, dims, ss, sj.YUV_AUTO, _quant(), 4)
    rplanes, rdims = _rgb_planes(res)
    out2, szs2, offs2, modes2, _, _ = engine.encode_ragged_full(sj.SRC_RGB, rplanes, rdims, sj.YUV_AUTO, _quant(), 4)
    assert modes == modes2 == [sj.riskiness_verdict(s, w, h)[0] for s, (w, h) in
                               zip(engine.riskiness_ragged(sj.SRC_RGB, rplanes, rdims).cpu().numpy(), rdims)]
    assert _streams(out, szs, offs) == _streams(out2, szs2, offs2)


def test_target_size_search(engine, batch):
    devs, sizes, small_dev, small = batch
    targets = [max(400, x.size // 6) for x in small]
    got = sj.encode_images(sj.Resized(devs, sizes), 75.0, sj.YUV_420, engine=engine, method=4, target_size=targets)
    assert got == sj.encode_images(small_dev, 75.0, sj.YUV_420, engine=engine, method=4, target_size=targets)
    planes, dims = _rgb_planes(devs)
    search = [dict(target_mode=sj.TARGET_SIZE, target_value=t) for t in targets]
    out, szs, offs, _, q, v = engine.encode_ragged_resized(sj.SRC_RGB, planes, dims, sizes, sj.YUV_420, _quant(), 4, search=search)
    assert _streams(out, szs, offs) == got
    rplanes, rdims = _rgb_planes(small_dev)
    _, _, _, _, q2, v2 = engine.encode_ragged_full(sj.SRC_RGB, rplanes, rdims, sj.YUV_420, _quant(), 4, search=search)
    torch.cuda.synchronize()
    assert q == q2 and v == v2


def test_packed(engine, batch):
    devs, sizes, small_dev, small = batch
    want = sj.encode_images(small_dev, 75.0, sj.YUV_444, engine=engine, method=4)
    assert sj.encode_images(sj.Resized(devs, sizes), 75.0, sj.YUV_444, engine=engine, method=4, packed=True) == want
    planes, dims = _rgb_planes(devs)
    out, szs, offs, modes, _, _ = engine.encode_ragged_resized_packed(sj.SRC_RGB, planes, dims, sizes, sj.YUV_444, _quant(), 4)
    torch.cuda.synchronize()
    o, sz, host = offs.cpu().numpy(), szs.cpu().numpy(), out.cpu().numpy()
    assert (sz > 0).all() and (o[:-1] % 16 == 0).all()
    assert list(o[:-1]) == sorted(o[:-1]) and len(set(o[:-1])) == len(devs)        # ascending in the caller's order
    assert o[-1] == sum((int(s) + 15) & ~15 for s in sz)
    assert [host[int(o[k]):int(o[k]) + int(sz[k])].tobytes() for k in range(len(devs))] == want


def test_metadata_with_a_size_target(engine, batch):
    devs, sizes, small_dev, small = batch
    metas = [sj.PictureMetadata(exif=b"Exif\0\0" + bytes(range(40)) * (k + 1)) if k % 2 == 0 else None for k in range(len(devs))]
    metas[3] = sj.PictureMetadata(xmp=b"<x:xmpmeta>resized</x:xmpmeta>", app_markers=b"\xff\xe5\x00\x06abcd")
    targets = [max(600, x.size // 5) for x in small]
    want = sj.encode_images_full_meta(small_dev, metas, yuv_mode=sj.YUV_420, target_size=targets, engine=engine)
    assert sj.encode_images_full_meta(sj.Resized(devs, sizes), metas, yuv_mode=sj.YUV_420, target_size=targets, engine=engine) == want
    planes, dims = _rgb_planes(devs)
    search = [dict(target_mode=sj.TARGET_SIZE, target_value=t) for t in targets]
    out, szs, offs, _, _, _ = engine.encode_ragged_resized(sj.SRC_RGB, planes, dims, sizes, sj.YUV_420, _quant(), 4, search=search,
                                                           metadata=metas)
    assert _streams(out, szs, offs) == want
    out, szs, offs, _, _, _ = engine.encode_ragged_resized_packed(sj.SRC_RGB, planes, dims, sizes, sj.YUV_420, _quant(), 4,
                                                                  search=search, metadata=metas)
    assert _streams(out, szs, offs.cpu().numpy()) == want


def test_float_pixels_and_chw(engine, batch):
    """Resized around a FloatPixels, layout="chw": the transform is read before the weighted sums are made"""
    devs, sizes, small_dev, small = batch
    made = [_on_device(d.cpu().numpy(), "planar", F16, seed=40 + k) for k, d in enumerate(devs)]
    fp = sj.FloatPixels([m[1] for m in made], *XFORM3[F16])
    got = sj.encode_images(sj.Resized(fp, sizes), 75.0, sj.YUV_420, engine=engine, method=4, layout="chw")
    assert got == sj.encode_images(small_dev, 75.0, sj.YUV_420, engine=engine, method=4)
    pics = sj.resize_images(fp, sizes, engine=engine, layout="chw")
    _check_pictures([p.permute(1, 2, 0) for p in pics], small)
    assert sj.encode_images_full_chw(pics, 75.0, sj.YUV_444, engine=engine) == sj.encode_images_full(small_dev, 75.0, sj.YUV_444, engine=engine)
    engine.set_pixel_transform(255.0, 0.0)


# ---- 4. sizes that change nothing, a box, two calls back to back, the engine's memory

def test_own_sizes_are_the_plain_call(engine, batch):
    devs = batch[0]
    own = [(d.shape[1], d.shape[0]) for d in devs]
    want = sj.encode_images(devs, 75.0, sj.YUV_420, engine=engine, method=4)
    assert sj.encode_images(sj.Resized(devs, own), 75.0, sj.YUV_420, engine=engine, method=4) == want
    planes, dims = _rgb_planes(devs)
    out, szs, offs, _, _, _ = engine.encode_ragged_full(sj.SRC_RGB, planes, dims, sj.YUV_420, _quant(), 4)
    assert _streams(out, szs, offs) == want
    before = engine.scratch_bytes()                  # (what the plain _full_ call holds)
    for sizes in (own, None):
        out, szs, offs, _, _, _ = engine.encode_ragged_resized(sj.SRC_RGB, planes, dims, sizes, sj.YUV_420, _quant(), 4)
        assert _streams(out, szs, offs) == want
    assert engine.scratch_bytes() == before          # no copy: nothing was allocated for resized pictures
    # an NV12 batch passes at its own sizes
    rs = np.random.RandomState(9600)
    nv, nvdims = [], [(34, 18), (17, 9)]
    for (w, h) in nvdims:
        nv.append([torch.from_numpy(rs.randint(0, 256, (h, w)).astype(np.uint8)).cuda(),
                   torch.from_numpy(rs.randint(0, 256, ((h + 1) // 2, 2 * ((w + 1) // 2))).astype(np.uint8)).cuda()])
    out, szs, offs, _, _, _ = engine.encode_ragged_resized(sj.SRC_NV12, nv, nvdims, nvdims, sj.YUV_420, _quant(), 4)
    out2, szs2, offs2, _, _, _ = engine.encode_ragged_full(sj.SRC_NV12, nv, nvdims, sj.YUV_420, _quant(), 4)
    assert _streams(out, szs, offs) == _streams(out2, szs2, offs2)
    with pytest.raises(sj.SjpegError, match="SJPEG_HIP_SRC_NV12"):
        engine.encode_ragged_resized(sj.SRC_NV12, nv, nvdims, [(34, 18), (16, 9)], sj.YUV_420, _quant(), 4)
    # the identity through the kernel is the picture
    _check_pictures(sj.resize_images(devs, own, engine=engine), [d.cpu().numpy() for d in devs])


def test_fit_into_a_box(engine, batch):
    """Resized.fit(images, (32, 32)): pictures larger than the box are fitted, smaller ones keep their size"""
    devs = batch[0]
    fitted = sj.Resized.fit(devs, (32, 32))
    assert fitted.sizes == [(17, 9), (30, 32), (31, 32), (32, 17), (8, 8)]
    small = [torch.from_numpy(_area(d.cpu().numpy(), *s)).cuda() for d, s in zip(devs, fitted.sizes)]
    assert sj.encode_images(fitted, 75.0, sj.YUV_420, engine=engine, method=4) == sj.encode_images(small, 75.0, sj.YUV_420, engine=engine, method=4)
    assert sj.encode_images_full(fitted, engine=engine) == sj.encode_images_full(small, engine=engine)


def test_two_calls_back_to_back(batch):
    """The second call writes the engine's resized pictures while the first call's encode may still read them: the
    stream orders the two.  No wait in between; both outputs checked afterwards."""
    devs, sizes, small_dev, small = batch
    eng = sj.Engine(0)
    planes, dims = _rgb_planes(devs)
    other = [torch.from_numpy(synth.g_noise(w, h, 9620 + k)).cuda() for k, (w, h) in enumerate(ENC_DIMS)]
    oplanes, odims = _rgb_planes(other)
    first = eng.encode_ragged_resized(sj.SRC_RGB, planes, dims, sizes, sj.YUV_420, _quant(), 0)
    second = eng.encode_ragged_resized(sj.SRC_RGB, oplanes, odims, sizes, sj.YUV_420, _quant(), 0)
    got1, got2 = _streams(*first[:3]), _streams(*second[:3])
    assert got1 == sj.encode_images(small_dev, 75.0, sj.YUV_420, engine=eng)
    osmall = [torch.from_numpy(_area(o.cpu().numpy(), *s)).cuda() for o, s in zip(other, sizes)]
    assert got2 == sj.encode_images(osmall, 75.0, sj.YUV_420, engine=eng)
    eng.close()


def test_scratch_bytes_and_trim(batch):
    devs, sizes, small_dev, small = batch
    eng = sj.Engine(0)
    planes, dims = _rgb_planes(devs)
    # the plain call on the resized pictures first: what the inner call takes is there already
    rplanes, rdims = _rgb_planes(small_dev)
    eng.encode_ragged_full(sj.SRC_RGB, rplanes, rdims, sj.YUV_420, _quant(), 4)
    torch.cuda.synchronize()
    before = eng.scratch_bytes()
    frames, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
    arr = np.ascontiguousarray(np.asarray(sizes, np.int32))
    need = sj.lib().sjpeg_hip_resize_ragged_bytes(sj.SRC_RGB, len(dims), frames, arr.ctypes.data)
    out, szs, offs, _, _, _ = eng.encode_ragged_resized(sj.SRC_RGB, planes, dims, sizes, sj.YUV_420, _quant(), 4)
    _streams(out, szs, offs)
    after = eng.scratch_bytes()
    assert after >= before + need
    eng.trim()
    assert eng.scratch_bytes() <= after - need
    eng.close()
