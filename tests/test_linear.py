"""Resize in linear light on the GPU (sjpeg_hip_linear_ragged_src and the other _linear entries, sjpeg_amd.light), byte
equality throughout.  The expectation is the definition of sjpeg_hip.h in numpy integers: every byte through the table
L[], the weighted sums S of test_resize._area's weights, and out = the number of k in 1..255 with 2 S >= (L[k-1] + L[k])
W H.  The table here is evaluated in double precision from the formula (tests/test_linear_host.py holds the library's to
the 60-digit one); nothing below asks the library what a byte's light is."""
import os

import numpy as np
import pytest
import torch

import sheet_model as sm
import sjpeg_amd as sj
import sjpeg_amd.light as li
from oracle import synth
from test_flatten import AXFORM, _alphas, _flatten, _rgba_on_device, _seen_rgba
from test_orient import _upright
from test_reduce import F16, F32, FORMATS, XFORM3, _check_pictures, _on_device, _quant, _rgb_planes, _seen, _streams
from test_resize import _area, _weights

pytestmark = pytest.mark.gpu

_C = np.arange(256) / 255.0
T = np.floor(65535.0 * np.where(_C <= 0.04045, _C / 12.92, ((_C + 0.055) / 1.055) ** 2.4) + 0.5).astype(np.int64)
MIDS = T[:-1] + T[1:]

# The stage holds 16-bit words, a run per channel: 16384 / (2 * channels) samples, down to a multiple of 4
CAP3, CAP1 = 2728, 8192
# source -> target: 1 x 1; identities, the last two tiles across; a support of 2 to 3; 64 lanes a column; the same
# turned on its side; and a row just under and just over what the stage holds, so the chunked path runs
SHAPES = [((1, 1), (1, 1)), ((3, 2), (3, 2)), ((5, 7), (5, 7)), ((257, 17), (257, 17)), ((7, 5), (3, 2)), ((300, 40), (7, 3)),
          ((40, 300), (3, 7))]
CAP_SHAPES = {3: [((CAP3 - 1, 2), (1, 1)), ((CAP3 + 1, 2), (2, 1))], 1: [((CAP1 - 1, 2), (1, 1)), ((CAP1 + 1, 2), (2, 1))]}
# (name of test_reduce.FORMATS, the channels staged): the byte formats of every staging class, F16 channel-first and F32
# channels-last with test_reduce's non-default transforms
KERNEL_FORMATS = [("RGB", 3), ("BGRA", 3), ("RGBA", 3), ("RGB_PLANAR", 3), ("GRAY", 1), ("RGB_PLANAR_F16", 3), ("RGB_F32", 3)]


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.fixture(scope="module")
def risk_table():
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        tab = f.read()
    sj.set_riskiness_table(tab)
    return tab


def _linear(b, w2, h2):
    """The definition of sjpeg_hip.h on a uint8 picture [H, W] or [H, W, C]"""
    H, W = b.shape[:2]
    wy, wx = _weights(H, h2), _weights(W, w2)
    p = T[b].reshape(H, W, -1)
    S = np.stack([(wy @ p[..., c]) @ wx.T for c in range(p.shape[2])], axis=-1)
    assert 0 <= S.min() and S.max() <= 65535 * W * H < 1 << 48
    out = (2 * S[..., None] >= MIDS * (W * H)).sum(axis=-1)
    return out.astype(np.uint8).reshape((h2, w2) + b.shape[2:])


def _checker(w, h):
    return np.where((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1, 255, 0).astype(np.uint8)[..., None].repeat(3, axis=2)


@pytest.fixture(scope="module")
def sources():
    """{channels: [(u8 [H, W, 3], (w', h'))]} of the kernel tests: noise for every shape and all 255 at the widest (the
    32-bit bound of a row's sum).  Never written to."""
    out = {}
    for ch in (3, 1):
        out[ch] = [(synth.g_noise(w, h, 9700 + k), size) for k, ((w, h), size) in enumerate(SHAPES + CAP_SHAPES[ch])]
        (w, h), size = CAP_SHAPES[ch][1]
        out[ch].append((np.full((h, w, 3), 255, np.uint8), size))
    return out


def test_the_expectation_itself():
    """_linear() where the answer is known: the table's check values, identity, constants, the three known answers"""
    assert T[:6].tolist() == [0, 20, 40, 60, 80, 99] and T[252:].tolist() == [63795, 64372, 64952, 65535] and T.sum() == 5217863
    im = np.random.RandomState(2).randint(0, 256, (9, 17, 3)).astype(np.uint8)
    assert np.array_equal(_linear(im, 17, 9), im)
    for v in (0, 1, 128, 254, 255):
        assert (_linear(np.full((40, 300), v, np.uint8), 7, 3) == v).all()
    assert (_linear(_checker(16, 8), 8, 4) == 188).all() and (_area(_checker(16, 8), 8, 4) == 128).all()
    assert _linear(np.array([[0, 0], [0, 255]], np.uint8), 1, 1)[0, 0] == 137
    assert _linear(np.array([[100, 200]], np.uint8), 1, 1)[0, 0] == 160


# ---- 1. the kernel alone: ONE ragged call per format over every shape -- sizes mixed in one launch

@pytest.mark.parametrize("name,channels", KERNEL_FORMATS)
def test_linear_ragged_against_the_definition(engine, sources, name, channels):
    fmt, layout, dtype = FORMATS[name]
    if dtype is not None:
        engine.set_pixel_transform(*XFORM3[dtype])
    planes, keep, wants, dims, sizes = [], [], [], [], []
    for k, (u8, size) in enumerate(sources[channels]):
        p, dev, host = _on_device(u8, layout, dtype, seed=k, off=k % 3, pad=(k // 3) % 2)
        seen = _seen(host, layout, dtype)
        assert np.array_equal(seen, u8[..., 1] if layout == "gray" else u8)     # (the construction and b() agree)
        planes.append(p); keep.append(dev)
        wants.append(_linear(seen, *size)); dims.append((u8.shape[1], u8.shape[0])); sizes.append(size)
    rfmt, pics, buf = li.linear_ragged(engine, fmt, planes, dims, sizes)
    assert rfmt == (sj.SRC_GRAY if layout == "gray" else sj.SRC_RGB)
    for p, size in zip(pics, sizes):
        assert (p.shape[1], p.shape[0]) == size
        assert p.data_ptr() % 16 == 0 and p.stride(0) % 4 == 0
    _check_pictures(pics, wants)
    # the identities are copies, and the full-scale row came back full scale
    for (u8, size), want in zip(sources[channels], wants):
        if size == (u8.shape[1], u8.shape[0]):
            assert np.array_equal(want, u8[..., 1] if layout == "gray" else u8)
    assert (wants[-1] == 255).all()
    engine.set_pixel_transform(255.0, 0.0)


@pytest.mark.parametrize("fmt", [sj.SRC_RGB, sj.SRC_GRAY])
def test_constants_come_back_unchanged_at_every_size(engine, fmt):
    shapes = SHAPES + CAP_SHAPES[3 if fmt == sj.SRC_RGB else 1]
    planes, keep, wants, dims, sizes = [], [], [], [], []
    for k, ((w, h), size) in enumerate(shapes):
        for v in (0, 1, 128, 254, 255):
            dev = torch.full((h, w, 3) if fmt == sj.SRC_RGB else (h, w), v, dtype=torch.uint8, device="cuda")
            keep.append(dev)
            planes.append([dev.view(h, -1)]); dims.append((w, h)); sizes.append(size)
            wants.append(np.full((size[1], size[0], 3) if fmt == sj.SRC_RGB else (size[1], size[0]), v, np.uint8))
    _, pics, _ = li.linear_ragged(engine, fmt, planes, dims, sizes)
    _check_pictures(pics, wants)


def test_checkerboard_halved_is_188_and_not_the_reduction(engine):
    """the 0 / 255 checkerboard at exact 2:1: 188 everywhere; Reduced by 2 averages bytes: 128"""
    ims = [torch.from_numpy(_checker(w, h)).cuda() for (w, h) in ((16, 8), (600, 4), (2, 2))]
    sizes = [(im.shape[1] // 2, im.shape[0] // 2) for im in ims]
    got = li.linear_resize_images(ims, sizes, engine=engine)
    _check_pictures(got, [np.full((h, w, 3), 188, np.uint8) for (w, h) in sizes])
    _check_pictures(sj.reduce_images(ims, 2, engine=engine), [np.full((h, w, 3), 128, np.uint8) for (w, h) in sizes])
    # 0 and 255 at 3:1, 100 and 200 in equal parts
    one = torch.tensor([[[0] * 3, [0] * 3], [[0] * 3, [255] * 3]], dtype=torch.uint8).cuda()
    two = torch.tensor([[[100] * 3, [200] * 3]], dtype=torch.uint8).cuda()
    got = li.linear_resize_images([one, two], [(1, 1), (1, 1)], engine=engine)
    _check_pictures(got, [np.full((1, 1, 3), 137, np.uint8), np.full((1, 1, 3), 160, np.uint8)])


def test_light_coded_is_the_oriented_call(engine):
    ims = [synth.g_noise(w, h, 9750 + k) for k, (w, h) in enumerate([(17, 9), (63, 65)])]
    devs = [torch.from_numpy(x).cuda() for x in ims]
    planes, dims = _rgb_planes(devs)
    sizes, orients = [(16, 9), (5, 64)], [6, 1]
    _, got, _ = li.linear_ragged(engine, sj.SRC_RGB, planes, dims, sizes, orients, light=li.CODED)
    _, want, _ = engine.orient_ragged(sj.SRC_RGB, planes, dims, sizes, orients)
    _check_pictures(got, [w.cpu().numpy() for w in want])
    _check_pictures(got, [np.ascontiguousarray(_upright(_area(x, *s), o)) for x, s, o in zip(ims, sizes, orients)])


# ---- 2. the eight orientations commute with the average; sizes and orientations mixed in one launch

@pytest.mark.parametrize("name", ["RGB", "GRAY"])
def test_all_eight_orientations(engine, name):
    fmt, layout, dtype = FORMATS[name]
    planes, keep, wants, dims, sizes, orients = [], [], [], [], [], []
    for si, ((w, h), size) in enumerate([((7, 5), (3, 2)), ((300, 40), (260, 20))]):       # (the second: two tiles across)
        u8 = synth.g_noise(w, h, 9760 + si)
        for o in range(1, 9):
            p, dev, host = _on_device(u8, layout, dtype, seed=o, off=o % 3, pad=o % 2)
            planes.append(p); keep.append(dev); dims.append((w, h)); sizes.append(size); orients.append(o)
            wants.append(np.ascontiguousarray(_upright(_linear(_seen(host, layout, dtype), *size), o)))
    rfmt, pics, _ = li.linear_ragged(engine, fmt, planes, dims, sizes, orients)
    _check_pictures(pics, wants)


# ---- 3. flatten comes first, on bytes

@pytest.mark.parametrize("name,layout,dtype", [("RGBA", "rgba", None), ("BGRA", "bgra", None), ("RGBA_F32", "rgba", F32)])
def test_flattened_then_linear(engine, name, layout, dtype):
    fmt = getattr(sj, "SRC_" + name)
    if dtype is not None:
        engine.set_pixel_transform(*XFORM3[dtype])
    shapes = [((5, 7), (5, 7)), ((7, 5), (3, 2)), ((300, 40), (7, 3)), ((CAP3 + 1, 2), (2, 1))]
    for bg, pre in (((255, 255, 255), False), ((17, 128, 250), True)):
        flatten = sj.Flatten(bg, pre, *(AXFORM[dtype] if dtype is not None else (255.0, 0.0)))
        planes, keep, wants, dims, sizes, orients = [], [], [], [], [], []
        for k, ((w, h), size) in enumerate(shapes):
            u8, alpha = synth.g_noise(w, h, 9780 + k), _alphas(w, h, 9790 + k)[0 if k != 1 else 3]
            p, dev, host = _rgba_on_device(u8, alpha, layout, dtype, seed=k, off=k % 3, pad=k % 2)
            s, a = _seen_rgba(host, layout, dtype)
            o = (1, 6, 3, 8)[k]
            planes.append(p); keep.append(dev); dims.append((w, h)); sizes.append(size); orients.append(o)
            wants.append(np.ascontiguousarray(_upright(_linear(_flatten(s, a, bg, pre), *size), o)))
        rfmt, pics, _ = li.linear_ragged(engine, fmt, planes, dims, sizes, orients, flatten)
        assert rfmt == sj.SRC_RGB
        _check_pictures(pics, wants)
    engine.set_pixel_transform(255.0, 0.0)


# ---- 4. a 2 x 2 sheet with gutter and margin: the background's bytes exactly as given

SHEET = sj.Sheet(2, 2, (21, 17), gutter=3, margin=5, background=(200, 100, 1))
SHEET_DIMS, SHEET_ORIENTS = [(37, 23), (9, 7), (40, 64), (64, 40), (300, 40)], [1, 6, 3, 8, 2]


def _grid(sheet):
    return sheet.cols, sheet.rows, sheet.cell, sheet.gutter, sheet.margin, sheet.background


@pytest.fixture(scope="module")
def sheet_batch():
    ims = [synth.g_noise(w, h, 9800 + k) for k, (w, h) in enumerate(SHEET_DIMS)]
    given = sm.fitted_sizes(SHEET_DIMS, SHEET.cell, SHEET_ORIENTS)
    thumbs = [_linear(x, *s) for x, s in zip(ims, given)]
    # (the model places and turns thumbnails that are already at their sizes: its own average of them is the identity)
    wants, where = sm.rgb_sheets(thumbs, *_grid(SHEET), given, SHEET_ORIENTS)
    return ims, [torch.from_numpy(x).cuda() for x in ims], [np.ascontiguousarray(w) for w in wants], where


def test_sheets_against_the_model(engine, risk_table, sheet_batch):
    ims, devs, wants, where = sheet_batch
    assert len(wants) == 2
    planes, dims = _rgb_planes(devs)
    rfmt, sheets, _ = li.sheet_ragged_linear(engine, sj.SRC_RGB, planes, dims, SHEET, None, SHEET_ORIENTS)
    assert rfmt == sj.SRC_RGB
    _check_pictures(sheets, wants)
    # margin, gutter and the empty cells of the second sheet are the background's bytes
    torch.cuda.synchronize()
    got = sheets[1].cpu().numpy()
    assert (got[:5] == SHEET.background).all() and (got[:, :5] == SHEET.background).all() and (got[5 + 17:5 + 17 + 3] == SHEET.background).all()
    assert (got[5 + 17 + 3:] == SHEET.background).all()
    _check_pictures(li.make_linear_sheets(devs, SHEET, orientations=SHEET_ORIENTS, engine=engine), wants)
    # the encode entries: the sheet entry followed by the full call on SRC_RGB
    want_dev = [torch.from_numpy(w).cuda() for w in wants]
    wplanes, wdims = _rgb_planes(want_dev)
    out2, szs2, offs2, modes2, q2, v2 = engine.encode_ragged_full(sj.SRC_RGB, wplanes, wdims, sj.YUV_AUTO, _quant(), 4)
    want = _streams(out2, szs2, offs2)
    for packed in (False, True):
        out, szs, offs, modes, q, v = li.encode_ragged_sheet_linear(engine, sj.SRC_RGB, planes, dims, SHEET, None, SHEET_ORIENTS, sj.YUV_AUTO,
                                                                    _quant(), 4, packed=packed)
        torch.cuda.synchronize()
        assert _streams(out, szs, offs.cpu().numpy() if packed else offs) == want
        assert modes == modes2 and q == q2 and v == v2
        got, places = li.encode_linear_sheets(devs, SHEET, orientations=SHEET_ORIENTS, engine=engine, packed=packed)
        assert got == want and places == where


# ---- 5. the encode entries: the shape entry followed by the full call on SRC_RGB / SRC_GRAY

ENC_DIMS = [(64, 48), (31, 33), (17, 9), (130, 70)]
ENC_SIZES = [(40, 30), (31, 33), (16, 9), (33, 18)]
ENC_ORIENTS = [6, 1, 3, 8]


@pytest.fixture(scope="module")
def batch():
    """(host pictures, the same on the device, the linear, upright pictures on the device)"""
    ims = [synth.g_struct(w, h, 9850 + k) if k % 2 else synth.g_noise(w, h, 9850 + k) for k, (w, h) in enumerate(ENC_DIMS)]
    up = [np.ascontiguousarray(_upright(_linear(x, *s), o)) for x, s, o in zip(ims, ENC_SIZES, ENC_ORIENTS)]
    return ims, [torch.from_numpy(x).cuda() for x in ims], [torch.from_numpy(x).cuda() for x in up], up


@pytest.mark.parametrize("mode,method,searched", [(sj.YUV_420, 0, False), (sj.YUV_AUTO, 4, False), (sj.YUV_420, 4, True)])
def test_encode_entries_against_the_full_call(engine, risk_table, batch, mode, method, searched):
    ims, devs, up_dev, up = batch
    planes, dims = _rgb_planes(devs)
    uplanes, udims = _rgb_planes(up_dev)
    search = [dict(target_mode=sj.TARGET_SIZE, target_value=max(400, x.size // 6)) for x in up] if searched else None
    out2, szs2, offs2, modes2, q2, v2 = engine.encode_ragged_full(sj.SRC_RGB, uplanes, udims, mode, _quant(), method, search=search)
    want = _streams(out2, szs2, offs2)
    _, made, _ = li.linear_ragged(engine, sj.SRC_RGB, planes, dims, ENC_SIZES, ENC_ORIENTS)
    _check_pictures(made, up)
    for packed in (False, True):
        out, szs, offs, modes, q, v = li.encode_ragged_linear(engine, sj.SRC_RGB, planes, dims, ENC_SIZES, ENC_ORIENTS, mode, _quant(), method,
                                                              search=search, packed=packed)
        torch.cuda.synchronize()
        assert _streams(out, szs, offs.cpu().numpy() if packed else offs) == want
        assert modes == modes2 and q == q2 and v == v2


def test_gray_is_coded_as_gray(engine):
    u8 = synth.g_noise(63, 65, 9870)[..., 1].copy()
    dev = torch.from_numpy(u8).cuda()
    want_dev = torch.from_numpy(_linear(u8, 5, 64)).cuda()
    out2, szs2, offs2, _, _, _ = engine.encode_ragged_full(sj.SRC_GRAY, [[want_dev]], [(5, 64)], sj.YUV_400, _quant(), 4)
    for packed in (False, True):
        out, szs, offs, _, _, _ = li.encode_ragged_linear(engine, sj.SRC_GRAY, [[dev]], [(63, 65)], [(5, 64)], None, sj.YUV_400, _quant(), 4,
                                                          packed=packed)
        torch.cuda.synchronize()
        assert _streams(out, szs, offs.cpu().numpy() if packed else offs) == _streams(out2, szs2, offs2)


# ---- 6. the Python calls against the same model

def test_python_calls(engine, risk_table, batch):
    ims, devs, up_dev, up = batch
    _check_pictures(li.linear_resize_images(devs, ENC_SIZES, orientations=ENC_ORIENTS, engine=engine), up)
    # own sizes: the pictures themselves; a box: fitted upright
    _check_pictures(li.linear_resize_images(devs, engine=engine), ims)
    fitted = [sj.fit_size(w, h, (20, 24) if o >= 5 else (24, 20)) for (w, h), o in zip(ENC_DIMS, ENC_ORIENTS)]
    boxed = [np.ascontiguousarray(_upright(_linear(x, *s), o)) for x, s, o in zip(ims, fitted, ENC_ORIENTS)]
    _check_pictures(li.linear_resize_images(devs, box=(24, 20), orientations=ENC_ORIENTS, engine=engine), boxed)
    metas = [sj.PictureMetadata(exif=b"Exif\0\0" + bytes(range(40))), None, None, sj.PictureMetadata(xmp=b"<x:xmpmeta>linear</x:xmpmeta>")]
    want = sj.encode_images_full_meta(up_dev, metas, quality=[60.0, 75.0, 90.0, 50.0], yuv_mode=sj.YUV_AUTO, engine=engine)
    for packed in (False, True):
        got = li.encode_linear_images(devs, ENC_SIZES, orientations=ENC_ORIENTS, quality=[60.0, 75.0, 90.0, 50.0], yuv_mode=sj.YUV_AUTO,
                                      metadata=metas, packed=packed, engine=engine)
        assert got == want
    targets = [max(400, x.size // 6) for x in up]
    want = sj.encode_images_full(up_dev, 75.0, sj.YUV_420, 4, target_size=targets, engine=engine)
    assert li.encode_linear_images(devs, ENC_SIZES, orientations=ENC_ORIENTS, target_size=targets, engine=engine) == want
    # channel-first float pictures with a non-default transform, and a flatten over RGBA bytes
    scale, bias = XFORM3[F16]
    chw = [torch.from_numpy(((x.astype(np.float64) - np.asarray(bias)) / np.asarray(scale)).astype(np.float32)).to(F16).permute(2, 0, 1).contiguous().cuda()
           for x in ims]
    seen = [_seen(t.cpu().to(torch.float32).numpy(), "planar", F16) for t in chw]
    got = li.linear_resize_images(sj.FloatPixels(chw, scale, bias), ENC_SIZES, layout="chw", engine=engine)
    _check_pictures([g.permute(1, 2, 0) for g in got], [_linear(s, *z) for s, z in zip(seen, ENC_SIZES)])
    engine.set_pixel_transform(255.0, 0.0)
    alpha = [_alphas(w, h, 9880 + k)[0] for k, (w, h) in enumerate(ENC_DIMS)]
    rgba = [torch.from_numpy(np.concatenate([x, a[..., None]], axis=2)).cuda() for x, a in zip(ims, alpha)]
    flat = sj.Flatten((17, 128, 250))
    wants = [_linear(_flatten(x, a, (17, 128, 250), False), *s) for x, a, s in zip(ims, alpha, ENC_SIZES)]
    _check_pictures(li.linear_resize_images(rgba, ENC_SIZES, flatten=flat, engine=engine), wants)
    want = sj.encode_images_full([torch.from_numpy(w).cuda() for w in wants], 75.0, sj.YUV_420, 4, engine=engine)
    assert li.encode_linear_images(rgba, ENC_SIZES, flatten=flat, engine=engine) == want
