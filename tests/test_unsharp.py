"""The unsharp mask inside the ragged call on the GPU (sjpeg_hip_unsharp_ragged_src and the other _unsharp entries,
sjpeg_amd.unsharp), byte equality throughout.  The expectation is the definition of sjpeg_hip.h in numpy integers, applied
to the made picture: the made picture itself is the existing tests' model of it (the source at its own size,
test_resize._area, test_flatten._flatten, test_linear._linear), or for video what the existing entry returns.  Nothing
below asks the library what a sharpened sample is."""
import os

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
import sjpeg_amd.light as li
import sjpeg_amd.unsharp as un
import sjpeg_amd.video as sv
from oracle import synth
from test_flatten import _alphas, _flatten, _rgba_on_device, _seen_rgba
from test_linear import _linear
from test_orient import _upright
from test_reduce import F16, FORMATS, XFORM3, _check_pictures, _on_device, _quant, _rgb_planes, _seen, _streams
from test_resize import _area
from test_yuv16 import _device as _deep_device
from test_yuv16 import _source as _deep_source
from test_yuv_resize import _device_planes, _source

pytestmark = pytest.mark.gpu

TILE_DWORDS, TILE_ROWS = 64, 16             # kUnsharpTileDwords, kUnsharpTileRows (ragged_aux.h)
assert "kUnsharpTileDwords = 64, kUnsharpTileRows = 16" in open(os.path.join(sj.CSRC, "ragged_aux.h")).read()
# widths one under, at and one over one tile and two tiles of 4 * TILE_DWORDS bytes, heights likewise: row lengths mod 4
# of 3, 0, 1, 1 (gray) and 3, 2, 1, 0 (RGB: 86 pixels put a pixel across a tile's edge)
GRAY_W = [4 * TILE_DWORDS - 1, 4 * TILE_DWORDS, 4 * TILE_DWORDS + 1, 8 * TILE_DWORDS + 1]
RGB_W = [4 * TILE_DWORDS // 3, 4 * TILE_DWORDS // 3 + 1, 8 * TILE_DWORDS // 3 + 1, 8 * TILE_DWORDS // 3 + 2]
HEIGHTS = [TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS + 1]
assert GRAY_W == [255, 256, 257, 513] and RGB_W == [85, 86, 171, 172] and HEIGHTS == [15, 16, 17, 33]
SMALL = [(1, 1), (2, 1), (1, 2), (3, 3), (5, 7)]
DOWN = [((300, 40), (7, 3)), ((40, 300), (3, 7))]
# per-frame parameters, mixed in the launch: (amount, threshold)
PARAMS = [(32, 0), (64, 0), (255, 0), (32, 25), (32, 26), (1, 0), (200, 3), (0, 0), (96, 1)]


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.fixture(scope="module")
def risk_table():
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        tab = f.read()
    sj.set_riskiness_table(tab)
    return tab


def _unsharp(b, amount, threshold):
    """The definition of sjpeg_hip.h on a uint8 picture [H, W] or [H, W, C]: the channels filtered each on its own"""
    p = b.astype(np.int64)
    H, W = p.shape[:2]
    e = np.pad(p, ((1, 1), (1, 1)) + ((0, 0),) * (p.ndim - 2), mode="edge")
    S = sum(wi * wj * e[i:i + H, j:j + W] for i, wi in enumerate((1, 2, 1)) for j, wj in enumerate((1, 2, 1)))
    D = 16 * p - S
    assert S.min() >= 0 and S.max() <= 4080 and np.abs(D).max() <= 4080
    v = np.clip((512 * p + amount * D + 256) >> 9, 0, 255)          # (>> on a negative int64 is the floor)
    return np.where(np.abs(D) < 16 * threshold, p, v).astype(np.uint8)


def _checker(w, h, c=3):
    g = np.where((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1, 255, 0).astype(np.uint8)
    return g[..., None].repeat(c, axis=2) if c > 1 else g


def test_the_expectation_itself():
    """_unsharp() where the answer is known: sjpeg_hip.h's known answers"""
    rows = np.array([[100] * 4 + [200] * 4] * 5, np.uint8)
    assert (_unsharp(rows, 32, 0) == [100, 100, 100, 75, 225, 200, 200, 200]).all()
    assert (_unsharp(rows, 64, 0) == [100, 100, 100, 50, 250, 200, 200, 200]).all()
    assert np.array_equal(_unsharp(rows, 32, 26), rows) and np.array_equal(_unsharp(rows, 32, 25), _unsharp(rows, 32, 0))
    assert _unsharp(np.array([[10, 12]], np.uint8), 32, 0).tolist() == [[10, 13]]
    board = np.where((np.arange(4)[:, None] + np.arange(4)[None, :]) & 1, 200, 100).astype(np.uint8)
    assert _unsharp(board, 32, 0)[0].tolist() == [63, 250, 50, 238]
    im = np.random.RandomState(3).randint(0, 256, (9, 17, 3)).astype(np.uint8)
    assert np.array_equal(_unsharp(im, 0, 0), im) and np.array_equal(_unsharp(im, 255, 255), im)
    assert np.array_equal(_unsharp(im, 77, 2)[..., 1], _unsharp(im[..., 1], 77, 2))
    assert (_unsharp(np.full((5, 7), 91, np.uint8), 255, 0) == 91).all() and _unsharp(np.array([[201]], np.uint8), 255, 0)[0, 0] == 201


@pytest.fixture(scope="module")
def sources():
    """{channels: [(u8 [H, W, 3] source, made size (w', h'), (amount, threshold))]}: noise at every shape, the parameters
    going round; all 0, all 255 and the 0 / 255 checkerboard at amount 255 at one shape over the tile.  Never written to."""
    out = {}
    for ch, widths in ((3, RGB_W), (1, GRAY_W)):
        shapes = [(s, s) for s in SMALL + list(zip(widths, HEIGHTS)) + [(widths[0], HEIGHTS[3]), (widths[3], HEIGHTS[0])]] + DOWN
        items = [(synth.g_noise(w, h, 9900 + k), size, PARAMS[k % len(PARAMS)]) for k, ((w, h), size) in enumerate(shapes)]
        w, h = widths[2], HEIGHTS[2]
        items += [(np.zeros((h, w, 3), np.uint8), (w, h), (255, 0)), (np.full((h, w, 3), 255, np.uint8), (w, h), (255, 0)),
                  (_checker(w, h), (w, h), (255, 0)), (_checker(5, 7), (5, 7), (255, 0))]
        out[ch] = items
    return out


def _made(seen, size):
    """the made picture of a source the kernel sees as `seen`: itself at its own size, else the area average"""
    return seen if size == (seen.shape[1], seen.shape[0]) else _area(seen, *size)


# ---- 1. the kernel against the definition: ONE ragged call per format over every shape, sizes and parameters mixed

@pytest.mark.parametrize("name", ["RGB", "GRAY", "RGB_PLANAR_F16"])
def test_unsharp_ragged_against_the_definition(engine, sources, name):
    fmt, layout, dtype = FORMATS[name]
    if dtype is not None:
        engine.set_pixel_transform(*XFORM3[dtype])
    planes, keep, wants, dims, sizes, us = [], [], [], [], [], []
    for k, (u8, size, (amount, threshold)) in enumerate(sources[1 if layout == "gray" else 3]):
        p, dev, host = _on_device(u8, layout, dtype, seed=k, off=k % 3, pad=(k // 3) % 2)
        seen = _seen(host, layout, dtype)
        planes.append(p); keep.append(dev); dims.append((u8.shape[1], u8.shape[0])); sizes.append(size)
        us.append(un.Unsharp(amount, threshold))
        wants.append(_unsharp(_made(seen, size), amount, threshold))
    rfmt, pics, buf = un.unsharp_ragged(engine, fmt, planes, dims, sizes, unsharp=us)
    assert rfmt == (sj.SRC_GRAY if layout == "gray" else sj.SRC_RGB)
    for p, size in zip(pics, sizes):
        assert (p.shape[1], p.shape[0]) == size and p.data_ptr() % 16 == 0 and p.stride(0) % 4 == 0
    _check_pictures(pics, wants)
    # the sources were read, not written; amount 0 inside a sharpening call is a copy; constants came back
    for (u8, size, (amount, _)), want in zip(sources[1 if layout == "gray" else 3], wants):
        if amount == 0 and size == (u8.shape[1], u8.shape[0]):
            assert np.array_equal(want, u8[..., 1] if layout == "gray" else u8)
    assert (wants[-4] == 0).all() and (wants[-3] == 255).all() and set(np.unique(wants[-2])) == {0, 255}
    engine.set_pixel_transform(255.0, 0.0)


def test_flattened_bgra_then_unsharp(engine, sources):
    bg = (17, 128, 250)
    flatten = sj.Flatten(bg, False)
    planes, keep, wants, dims, sizes, us = [], [], [], [], [], []
    for k, (u8, size, (amount, threshold)) in enumerate(sources[3]):
        alpha = _alphas(u8.shape[1], u8.shape[0], 9950 + k)[0 if k % 4 else 3]
        p, dev, host = _rgba_on_device(u8, alpha, "bgra", None, seed=k, off=k % 3, pad=k % 2)
        s, a = _seen_rgba(host, "bgra", None)
        planes.append(p); keep.append(dev); dims.append((u8.shape[1], u8.shape[0])); sizes.append(size)
        us.append(un.Unsharp(amount, threshold))
        wants.append(_unsharp(_made(_flatten(s, a, bg, False), size), amount, threshold))
    rfmt, pics, _ = un.unsharp_ragged(engine, sj.SRC_BGRA, planes, dims, sizes, flatten=flatten, unsharp=us)
    assert rfmt == sj.SRC_RGB
    _check_pictures(pics, wants)


def test_linear_light_then_unsharp(engine):
    ims = [synth.g_noise(w, h, 9960 + k) for k, ((w, h), _) in enumerate(DOWN + [((600, 70), (172, 33))])]
    sizes = [s for _, s in DOWN] + [(172, 33)]
    devs = [torch.from_numpy(x).cuda() for x in ims]
    planes, dims = _rgb_planes(devs)
    us = [un.Unsharp(32, 0), un.Unsharp(255, 1), un.Unsharp(64, 0)]
    _, pics, _ = un.unsharp_ragged(engine, sj.SRC_RGB, planes, dims, sizes, light=li.LINEAR_SRGB, unsharp=us)
    _check_pictures(pics, [_unsharp(_linear(x, *s), u.amount, u.threshold) for x, s, u in zip(ims, sizes, us)])


# ---- 2. properties

def test_amount_0_is_the_older_call_and_threshold_255_the_identity(engine):
    ims = [synth.g_noise(w, h, 9970 + k) for k, (w, h) in enumerate([(17, 9), (63, 65), (300, 40)])]
    devs = [torch.from_numpy(x).cuda() for x in ims]
    planes, dims = _rgb_planes(devs)
    sizes, orients = [(16, 9), (5, 64), (260, 20)], [6, 1, 3]
    _, want, _ = engine.orient_ragged(sj.SRC_RGB, planes, dims, sizes, orients)
    want = [w.cpu().numpy() for w in want]
    for unsharp in (None, un.Unsharp(0, 0), [un.Unsharp(0, k) for k in range(3)], un.Unsharp(255, 255)):
        _, got, _ = un.unsharp_ragged(engine, sj.SRC_RGB, planes, dims, sizes, orients, unsharp=unsharp)
        _check_pictures(got, want)
    _, want, _ = li.linear_ragged(engine, sj.SRC_RGB, planes, dims, sizes, orients)
    want = [w.cpu().numpy() for w in want]
    for unsharp in (None, un.Unsharp(0, 9), un.Unsharp(200, 255)):
        _, got, _ = un.unsharp_ragged(engine, sj.SRC_RGB, planes, dims, sizes, orients, light=li.LINEAR_SRGB, unsharp=unsharp)
        _check_pictures(got, want)


@pytest.mark.parametrize("name", ["RGB", "GRAY"])
def test_sharpening_commutes_with_the_eight_orientations(engine, name):
    fmt, layout, dtype = FORMATS[name]
    planes, keep, dims, sizes, orients = [], [], [], [], []
    shapes = [((7, 5), (7, 5)), ((300, 40), (260, 20)), ((86, 17), (86, 17))]
    for si, ((w, h), size) in enumerate(shapes):
        u8 = synth.g_noise(w, h, 9980 + si)
        for o in range(1, 9):
            p, dev, host = _on_device(u8, layout, dtype, seed=o, off=o % 3, pad=o % 2)
            planes.append(p); keep.append(dev); dims.append((w, h)); sizes.append(size); orients.append(o)
    _, pics, _ = un.unsharp_ragged(engine, fmt, planes, dims, sizes, orients, unsharp=un.Unsharp(48, 1))
    torch.cuda.synchronize()
    got = [p.cpu().numpy() for p in pics]
    for si in range(len(shapes)):
        first = got[8 * si]
        assert not np.array_equal(first, _made(synth.g_noise(*shapes[si][0], 9980 + si)[..., 1] if layout == "gray" else
                                               synth.g_noise(*shapes[si][0], 9980 + si), shapes[si][1]))        # (it was sharpened)
        for o in range(1, 9):
            assert np.array_equal(got[8 * si + o - 1], np.ascontiguousarray(_upright(first, o))), (si, o)


# ---- 3. video: Y sharpened, U and V exactly the existing entry's

VIDEO = [("nv12", sj.SRC_NV12), ("yuv420", sj.SRC_YUV420), ("yuv444", sj.SRC_YUV444)]
VIDEO_CASES = [((5, 7), None, 1), ((1, 1), None, 1), ((18, 10), (10, 6), 6), ((600, 70), (513, 33), 1), ((257, 17), None, 3)]


def _host(pics):
    torch.cuda.synchronize()
    return [[p.cpu().numpy().copy() for p in pic] for pic in pics]


def _check_video(got, ref, us):
    got, ref = _host(got), _host(ref)
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g[0], _unsharp(r[0], us[k].amount, us[k].threshold)), (k, "Y")
        assert np.array_equal(g[1], r[1]) and np.array_equal(g[2], r[2]), (k, "U, V")


@pytest.mark.parametrize("name,fmt", VIDEO)
def test_video_luma_alone_is_sharpened(engine, name, fmt):
    dims = [c[0] for c in VIDEO_CASES]
    sizes = [c[1] if c[1] is not None else c[0] for c in VIDEO_CASES]
    orients = [c[2] for c in VIDEO_CASES]
    frames = [tuple(_device_planes(fmt, _source(fmt, w, h, 5300 + 7 * k))) for k, (w, h) in enumerate(dims)]
    us = [un.Unsharp(*PARAMS[k]) for k in range(len(dims))]
    colours = [sv.VideoColour("bt709", "limited"), sv.VideoColour("bt601", "full"), sv.VideoColour("bt601", "limited"),
               sv.VideoColour("bt709", "full"), sv.VideoColour("bt709", "limited")]
    for colour in (colours, None):
        rf, ref, _ = sv.convert_yuv_frames(frames, fmt, colour, sizes=sizes, orientations=orients, engine=engine)
        gf, got, _ = un.unsharp_video_frames(frames, fmt, colour, sizes=sizes, orientations=orients, unsharp=us, engine=engine)
        assert gf == rf
        _check_video(got, ref, us)


def test_p010_bt709_limited(engine):
    dims, sizes = [(5, 7), (34, 18), (600, 70)], [(5, 7), (17, 9), (257, 17)]
    frames = [_deep_device("nv12", _deep_source("nv12", w, h, 5400 + k, 8)) for k, (w, h) in enumerate(dims)]
    us = [un.Unsharp(255, 0), un.Unsharp(32, 2), un.Unsharp(64, 0)]
    colour = sv.VideoColour("bt709", "limited")
    _, ref, _ = sv.convert_deep_frames(frames, sj.SRC_NV12, colour, sizes=sizes, engine=engine, depth=sv.VideoDepth.P010)
    _, got, _ = un.unsharp_video_frames(frames, sj.SRC_NV12, colour, sizes=sizes, unsharp=us, depth=sv.VideoDepth.P010, engine=engine)
    _check_video(got, ref, us)


# ---- 4. the encode entries: the shape entry followed by the full call on what it made

ENC_DIMS = [(64, 48), (31, 33), (17, 9), (130, 70)]
ENC_SIZES = [(40, 30), (31, 33), (16, 9), (33, 18)]
ENC_ORIENTS = [6, 1, 3, 8]
ENC_US = [un.Unsharp(32, 0), un.Unsharp(64, 2), un.Unsharp(0, 0), un.Unsharp(255, 0)]


@pytest.fixture(scope="module")
def batch(engine):
    """(the pictures on the device, what unsharp_ragged makes of them -- held to the definition --, on the device)"""
    ims = [synth.g_struct(w, h, 9990 + k) if k % 2 else synth.g_noise(w, h, 9990 + k) for k, (w, h) in enumerate(ENC_DIMS)]
    devs = [torch.from_numpy(x).cuda() for x in ims]
    planes, dims = _rgb_planes(devs)
    _, made, _ = un.unsharp_ragged(engine, sj.SRC_RGB, planes, dims, ENC_SIZES, ENC_ORIENTS, unsharp=ENC_US)
    up = [_unsharp(np.ascontiguousarray(_upright(_area(x, *s), o)), u.amount, u.threshold) for x, s, o, u in zip(ims, ENC_SIZES, ENC_ORIENTS, ENC_US)]
    _check_pictures(made, up)
    return devs, [torch.from_numpy(x).cuda() for x in up]


@pytest.mark.parametrize("mode,method,searched,packed", [(sj.YUV_420, 4, False, False), (sj.YUV_AUTO, 4, False, True), (sj.YUV_420, 4, True, False)])
def test_encode_entries_against_the_full_call(engine, risk_table, batch, mode, method, searched, packed):
    devs, up_dev = batch
    planes, dims = _rgb_planes(devs)
    uplanes, udims = _rgb_planes(up_dev)
    search = [dict(target_mode=sj.TARGET_SIZE, target_value=max(400, int(x.numel()) // 6)) for x in up_dev] if searched else None
    out2, szs2, offs2, modes2, q2, v2 = engine.encode_ragged_full(sj.SRC_RGB, uplanes, udims, mode, _quant(), method, search=search)
    want = _streams(out2, szs2, offs2)
    out, szs, offs, modes, q, v = un.encode_ragged_unsharp(engine, sj.SRC_RGB, planes, dims, ENC_SIZES, ENC_ORIENTS, mode, _quant(), method,
                                                           unsharp=ENC_US, search=search, packed=packed)
    torch.cuda.synchronize()
    assert _streams(out, szs, offs.cpu().numpy() if packed else offs) == want
    assert modes == modes2 and q == q2 and v == v2


def test_the_final_pictures_are_engine_scratch(batch):
    """an encode keeps the made pictures and the sharpened ones apart, both in engine memory: counted, trimmed, made again"""
    devs, up_dev = batch
    planes, dims = _rgb_planes(devs)
    eng = sj.Engine(0)
    big = [(w, h) for (w, h) in dims]                                # (own sizes: the most bytes)
    need = sj.lib().sjpeg_hip_orient_ragged_bytes(sj.SRC_RGB, len(dims), sj._ragged_frames(planes, dims, None, None, None, None)[0], None, None)
    assert need > 0

    def jpegs(unsharp):
        out, szs, offs, _, _, _ = un.encode_ragged_unsharp(eng, sj.SRC_RGB, planes, dims, big, None, sj.YUV_420, _quant(), 0, unsharp=unsharp)
        return _streams(out, szs, offs)

    jpegs(None)                                                      # (the older call at own sizes: nothing is made)
    plain = eng.scratch_bytes()
    first = jpegs(un.Unsharp(32, 0))
    both = eng.scratch_bytes()
    assert both >= plain + 2 * need                                  # (the made pictures and the final ones, apart)
    eng.trim()
    assert eng.scratch_bytes() <= both - 2 * need                    # (both were released)
    assert jpegs(un.Unsharp(32, 0)) == first and eng.scratch_bytes() >= 2 * need


def test_python_calls_with_metadata(engine, risk_table, batch):
    devs, up_dev = batch
    _check_pictures(un.unsharp_images(devs, ENC_SIZES, orientations=ENC_ORIENTS, unsharp=ENC_US, engine=engine), [u.cpu().numpy() for u in up_dev])
    metas = [sj.PictureMetadata(exif=b"Exif\0\0" + bytes(range(40))), None, None, sj.PictureMetadata(xmp=b"<x:xmpmeta>unsharp</x:xmpmeta>")]
    qs = [60.0, 75.0, 90.0, 50.0]
    want = sj.encode_images_full_meta(up_dev, metas, quality=qs, yuv_mode=sj.YUV_AUTO, engine=engine)
    for packed in (False, True):
        got = un.encode_unsharp_images(devs, ENC_SIZES, orientations=ENC_ORIENTS, unsharp=ENC_US, quality=qs, yuv_mode=sj.YUV_AUTO,
                                       metadata=metas, packed=packed, engine=engine)
        assert got == want
    # sharpen only: no sizes, one Unsharp for all
    ims = [d.cpu().numpy() for d in devs]
    _check_pictures(un.unsharp_images(devs, unsharp=un.Unsharp(40, 1), engine=engine), [_unsharp(x, 40, 1) for x in ims])


def test_video_encode(engine):
    fmt = sj.SRC_NV12
    dims, sizes = [(34, 18), (64, 48)], [(17, 9), (64, 48)]
    frames = [tuple(_device_planes(fmt, _source(fmt, w, h, 5500 + k))) for k, (w, h) in enumerate(dims)]
    us = [un.Unsharp(64, 0), un.Unsharp(32, 1)]
    colour = sv.VideoColour("bt709", "limited")
    _, made, _ = un.unsharp_video_frames(frames, fmt, colour, sizes=sizes, unsharp=us, engine=engine)
    want = sj.encode_yuv_frames([tuple(p.clone() for p in pic) for pic in made], sj.SRC_YUV420, quality=80.0, engine=engine)
    for packed in (False, True):
        assert un.encode_unsharp_video_frames(frames, fmt, colour, sizes=sizes, unsharp=us, quality=80.0, packed=packed, engine=engine) == want
