"""Resampling with Pillow's filters inside the ragged call on the GPU (sjpeg_hip_resample_ragged_src and the _resampled_
entries, sjpeg_amd.resample), byte equality throughout.  The expectation is tests/resample_model.py -- the definition
of sjpeg_hip.h in numpy integers and Python doubles, which test_resample_model_host.py holds to what Pillow 12.2.0 made --
applied to the bytes the encoder sees.  Nothing below asks the library what a resampled sample is."""
import os

import numpy as np
import pytest
import torch

import resample_model as rm
import sjpeg_amd as sj
import sjpeg_amd.resample as rs
import sjpeg_amd.unsharp as un
from oracle import synth
from test_flatten import _alphas, _flatten, _rgba_on_device, _seen_rgba
from test_reduce import F16, FORMATS, XFORM3, _check_pictures, _on_device, _quant, _rgb_planes, _seen, _streams
from test_unsharp import _unsharp

pytestmark = pytest.mark.gpu

TILE_COLS, TILE_ROWS, KSIZE_MAX = 32, 16, 385      # kResampleTileCols, kResampleTileRows, kResampleKsizeMax (ragged_aux.h)
_aux = open(os.path.join(sj.CSRC, "ragged_aux.h")).read()
assert "kResampleTileCols = 32, kResampleTileRows = 16" in _aux and "kResampleKsizeMax = 385" in _aux
# made widths and heights one under, at and one over one tile and two tiles; 34 adds the row length that is 2 mod 4:
# gray rows 3, 0, 1, 2, 3, 0, 1 and RGB rows 1, 0, 3, 2, 1, 0, 3 mod 4
WIDTHS = [TILE_COLS - 1, TILE_COLS, TILE_COLS + 1, TILE_COLS + 2, 2 * TILE_COLS - 1, 2 * TILE_COLS, 2 * TILE_COLS + 1]
HEIGHTS = [TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, TILE_ROWS + 2, 2 * TILE_ROWS - 1, 2 * TILE_ROWS, 2 * TILE_ROWS + 1]
assert sorted({w % 4 for w in WIDTHS}) == [0, 1, 2, 3] and sorted({3 * w % 4 for w in WIDTHS}) == [0, 1, 2, 3]
# (source size, made size): the tile edges from a source that shrinks on one axis and grows on the other in turn;
# tiny sources and results; each axis alone, neither, one up while the other goes down; enlarging by 1.5 and by 7; a
# ratio that is no integer; a strip whose windows span several row chunks and a long segment; the cap on both axes
SHAPES = ([((48, 24), (w, h)) for w, h in zip(WIDTHS, HEIGHTS)] + [((48, 24), (WIDTHS[6], HEIGHTS[0])), ((48, 24), (WIDTHS[0], HEIGHTS[6]))] +
          [((1, 1), (1, 1)), ((1, 1), (3, 3)), ((2, 1), (1, 2)), ((1, 2), (2, 1)), ((3, 3), (1, 1)), ((3, 3), (3, 3)), ((3, 3), (2, 1)),
           ((2, 1), (3, 3))] +
          [((50, 40), (50, 17)), ((50, 40), (23, 40)), ((50, 40), (50, 40)), ((50, 40), (75, 13)), ((50, 40), (20, 90))] +
          [((20, 12), (30, 18)), ((9, 7), (63, 49)), ((100, 60), (37, 23)), ((700, 5), (3, 2)), ((192, 192), (3, 3))])
assert rm.ksize(rm.LANCZOS, 192, 3) == KSIZE_MAX


def _content(w, h, k):
    """random bytes, 0 / 255 noise and the 0 / 255 checkerboard in turn: the last two drive the sums to both clips"""
    if k % 3 == 0:
        return synth.g_noise(w, h, 9100 + k)
    if k % 3 == 1:
        return (synth.g_noise(w, h, 9100 + k) >> 7) * np.uint8(255)
    g = np.where((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1, 255, 0).astype(np.uint8)
    return np.ascontiguousarray(g[..., None].repeat(3, axis=2))


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.fixture(scope="module")
def risk_table():
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        tab = f.read()
    sj.set_riskiness_table(tab)
    return tab


@pytest.fixture(scope="module")
def sources():
    """[(u8 [H, W, 3] source, made size, filter)]: every shape, the five filters and the three contents going round --
    the cap's frame with Lanczos.  Never written to."""
    out = [(_content(w, h, k), size, rm.FILTERS[k % 5]) for k, ((w, h), size) in enumerate(SHAPES)]
    out[-1] = (out[-1][0], out[-1][1], rm.LANCZOS)
    assert {f for _, _, f in out} == set(rm.FILTERS)
    return out


def test_the_expectation_itself():
    """resample_model where the answer is known: sjpeg_hip.h's known answers, and the clips are reached"""
    up = np.array([[0, 255]], np.uint8)
    assert [rm.resample(up, (4, 1), f)[0].tolist() for f in rm.FILTERS] == [[0, 0, 255, 255], [0, 64, 191, 255], [0, 19, 236, 255],
                                                                           [0, 53, 202, 255], [0, 59, 196, 255]]
    down = np.array([[10, 20, 30, 40, 250, 240, 230, 220]], np.uint8)
    assert [rm.resample(down, (2, 1), f)[0].tolist() for f in rm.FILTERS] == [[25, 235], [57, 207], [38, 224], [47, 217], [46, 220]]
    im = _content(9, 7, 1)
    assert np.array_equal(rm.resample(im, (9, 7), rm.LANCZOS), im)
    b, K = rm.identity_table(5)
    assert np.array_equal(rm.apply_axis(im[:5], b, K), im[:5])
    # a clipped sum: Lanczos overshoots on a 0 / 255 edge
    edge = np.array([[0] * 8 + [255] * 8], np.uint8)
    b, K = rm.table(rm.LANCZOS, 16, 48)
    sums = [(1 << 21) + int((K[x, :b[x, 1]].astype(np.int64) * edge[0, b[x, 0]:b[x, 0] + b[x, 1]]).sum()) for x in range(48)]
    assert min(sums) < 0 and max(sums) >> 22 > 255


# ---- 1. the kernel against the definition: ONE ragged call per format over every shape, filters mixed per frame

def _batch(items, layout, dtype):
    planes, keep, wants, dims, sizes, filters = [], [], [], [], [], []
    for k, (u8, size, filt) in enumerate(items):
        p, dev, host = _on_device(u8, layout, dtype, seed=k, off=k % 3, pad=(k // 3) % 2)
        planes.append(p); keep.append(dev); dims.append((u8.shape[1], u8.shape[0])); sizes.append(size); filters.append(rs.Filter(filt))
        wants.append(rm.resample(_seen(host, layout, dtype), size, filt))
    return planes, keep, wants, dims, sizes, filters


@pytest.mark.parametrize("name", ["RGB", "GRAY"])
def test_every_shape_with_the_filters_mixed(engine, sources, name):
    fmt, layout, dtype = FORMATS[name]
    planes, keep, wants, dims, sizes, filters = _batch(sources, layout, dtype)
    rfmt, pics, buf = rs.resample_ragged(engine, fmt, planes, dims, sizes, filters)
    assert rfmt == (sj.SRC_GRAY if layout == "gray" else sj.SRC_RGB)
    for p, size in zip(pics, sizes):
        assert (p.shape[1], p.shape[0]) == size and p.data_ptr() % 16 == 0 and p.stride(0) % 4 == 0
    _check_pictures(pics, wants)
    assert any((w == 0).any() and (w == 255).any() for w in wants)


@pytest.mark.parametrize("name", ["BGRA", "RGBA", "RGB_PLANAR", "RGB_PLANAR_F16", "GRAY_F16"])
def test_every_format_class(engine, sources, name):
    """packed four bytes (the fourth sample dropped), planar, and float kinds through a per-channel transform"""
    fmt, layout, dtype = FORMATS[name]
    if dtype is not None:
        engine.set_pixel_transform(*XFORM3[dtype])
    items = [sources[k] for k in (0, 3, 6, 9, 12, 16, 20, 22, 23, 24, 25)]
    planes, keep, wants, dims, sizes, filters = _batch(items, layout, dtype)
    _, pics, _ = rs.resample_ragged(engine, fmt, planes, dims, sizes, filters)
    _check_pictures(pics, wants)
    engine.set_pixel_transform(255.0, 0.0)


def test_flatten_on_rgba(engine, sources):
    bg = (17, 128, 250)
    planes, keep, wants, dims, sizes, filters = [], [], [], [], [], []
    for k, (u8, size, filt) in enumerate(sources[k] for k in (1, 5, 10, 19, 23, 24)):
        alpha = _alphas(u8.shape[1], u8.shape[0], 9150 + k)[0 if k % 4 else 3]
        p, dev, host = _rgba_on_device(u8, alpha, "rgba", None, seed=k, off=k % 3, pad=k % 2)
        s, a = _seen_rgba(host, "rgba", None)
        planes.append(p); keep.append(dev); dims.append((u8.shape[1], u8.shape[0])); sizes.append(size); filters.append(rs.Filter(filt))
        wants.append(rm.resample(_flatten(s, a, bg, False), size, filt))
    rfmt, pics, _ = rs.resample_ragged(engine, sj.SRC_RGBA, planes, dims, sizes, filters, flatten=sj.Flatten(bg, False))
    assert rfmt == sj.SRC_RGB
    _check_pictures(pics, wants)


@pytest.mark.parametrize("name", ["RGB", "GRAY"])
def test_the_eight_orientations_on_a_frame_that_is_not_square(engine, name):
    """U = turn(R): resample the stored picture, then turn"""
    fmt, layout, dtype = FORMATS[name]
    planes, keep, dims, sizes, orients, wants = [], [], [], [], [], []
    for si, ((w, h), size, filt) in enumerate([((40, 23), (57, 11), rm.LANCZOS), ((23, 40), (23, 40), rm.BICUBIC), ((70, 50), (33, 35), rm.HAMMING)]):
        u8 = synth.g_noise(w, h, 9200 + si)
        for o in range(1, 9):
            p, dev, host = _on_device(u8, layout, dtype, seed=o, off=o % 3, pad=o % 2)
            planes.append(p); keep.append(dev); dims.append((w, h)); sizes.append(size); orients.append(o)
            wants.append(np.ascontiguousarray(rm.turn(rm.resample(_seen(host, layout, dtype), size, filt), o)))
    filters = [rs.Filter.LANCZOS] * 8 + [rs.Filter.BICUBIC] * 8 + [rs.Filter.HAMMING] * 8
    _, pics, _ = rs.resample_ragged(engine, fmt, planes, dims, sizes, filters, orients)
    _check_pictures(pics, wants)


def test_negative_row_stride(engine):
    ims = [synth.g_noise(w, h, 9300 + k) for k, (w, h) in enumerate([(17, 9), (63, 65), (130, 70)])]
    sizes = [(40, 4), (20, 100), (33, 18)]
    devs = [torch.from_numpy(np.ascontiguousarray(im[::-1])).cuda() for im in ims]         # stored bottom-up
    planes = [[(d.data_ptr() + (d.shape[0] - 1) * d.stride(0), -d.stride(0))] for d in devs]
    _, pics, _ = rs.resample_ragged(engine, sj.SRC_RGB, planes, [(im.shape[1], im.shape[0]) for im in ims], sizes, rs.Filter.BICUBIC)
    _check_pictures(pics, [rm.resample(im, s, rm.BICUBIC) for im, s in zip(ims, sizes)])


# ---- 2. unsharp behind it, and the encode entries: the family's JPEG contract

ENC_DIMS = [(64, 48), (31, 33), (17, 9), (130, 70)]
ENC_SIZES = [(40, 30), (31, 33), (51, 27), (33, 18)]
ENC_ORIENTS = [6, 1, 3, 8]
ENC_FILTERS = [rs.Filter.LANCZOS, rs.Filter.BOX, rs.Filter.BICUBIC, rs.Filter.BILINEAR]
ENC_US = [un.Unsharp(32, 0), un.Unsharp(64, 2), un.Unsharp(0, 0), un.Unsharp(255, 0)]


@pytest.fixture(scope="module")
def batch():
    """(the pictures on the device, the model's upright pictures, the model's sharpened ones)"""
    ims = [synth.g_struct(w, h, 9400 + k) if k % 2 else synth.g_noise(w, h, 9400 + k) for k, (w, h) in enumerate(ENC_DIMS)]
    devs = [torch.from_numpy(x).cuda() for x in ims]
    up = [np.ascontiguousarray(rm.turn(rm.resample(x, s, int(f)), o)) for x, s, f, o in zip(ims, ENC_SIZES, ENC_FILTERS, ENC_ORIENTS)]
    return devs, up, [_unsharp(x, u.amount, u.threshold) for x, u in zip(up, ENC_US)]


def test_unsharp_behind_the_resample(engine, batch):
    devs, up, sharp = batch
    planes, dims = _rgb_planes(devs)
    _, pics, _ = rs.resample_ragged(engine, sj.SRC_RGB, planes, dims, ENC_SIZES, ENC_FILTERS, ENC_ORIENTS, unsharp=ENC_US)
    _check_pictures(pics, sharp)
    _, pics, _ = rs.resample_ragged(engine, sj.SRC_RGB, planes, dims, ENC_SIZES, ENC_FILTERS, ENC_ORIENTS, unsharp=un.Unsharp(0, 7))
    _check_pictures(pics, up)


@pytest.mark.parametrize("sharpened", [False, True])
def test_the_jpeg_contract_through_the_python_calls(engine, risk_table, batch, sharpened):
    devs, up, sharp = batch
    model = [torch.from_numpy(x).cuda() for x in (sharp if sharpened else up)]
    _check_pictures(rs.resample_images(devs, ENC_SIZES, ENC_FILTERS, ENC_ORIENTS, engine=engine), up)
    qs = [60.0, 75.0, 90.0, 50.0]
    want = sj.encode_images_full(model, quality=qs, yuv_mode=sj.YUV_AUTO, engine=engine)
    for packed in (False, True):
        got = rs.encode_resampled_images(devs, ENC_SIZES, filter=ENC_FILTERS, unsharp=ENC_US if sharpened else None, orientations=ENC_ORIENTS,
                                         quality=qs, yuv_mode=sj.YUV_AUTO, packed=packed, engine=engine)
        assert got == want


def test_box_never_enlarges_and_metadata_goes_along(engine, batch):
    devs, _, _ = batch
    ims = [d.cpu().numpy() for d in devs]
    fitted = [sj.fit_size(w, h, (48, 48)) for w, h in ENC_DIMS]
    assert fitted[2] == (17, 9)
    model = [torch.from_numpy(rm.resample(x, s, rm.LANCZOS)).cuda() for x, s in zip(ims, fitted)]
    metas = [sj.PictureMetadata(exif=b"Exif\0\0" + bytes(range(40))), None, None, sj.PictureMetadata(xmp=b"<x:xmpmeta>resample</x:xmpmeta>")]
    want = sj.encode_images_full_meta(model, metas, quality=80.0, yuv_mode=sj.YUV_420, engine=engine)
    assert rs.encode_resampled_images(devs, box=(48, 48), metadata=metas, quality=80.0, yuv_mode=sj.YUV_420, engine=engine) == want


def test_pipelined_engine(batch):
    devs, up, _ = batch
    planes, dims = _rgb_planes(devs)
    uplanes, udims = _rgb_planes([torch.from_numpy(x).cuda() for x in up])
    eng = sj.Engine(0)
    out2, szs2, offs2, _, _, _ = eng.encode_ragged_full(sj.SRC_RGB, uplanes, udims, sj.YUV_420, _quant(), 4)
    eng.wait()
    want = _streams(out2, szs2, offs2)
    eng.set_pipelined(True)
    for _ in range(2):
        out, szs, offs, _, _, _ = rs.encode_ragged_resampled(eng, sj.SRC_RGB, planes, dims, ENC_SIZES, ENC_ORIENTS, sj.YUV_420, _quant(), 4,
                                                            filter=ENC_FILTERS)
        eng.wait()
        torch.cuda.synchronize()
        assert _streams(out, szs, offs) == want


def test_the_tables_and_the_pictures_are_engine_scratch(batch):
    devs, up, _ = batch
    planes, dims = _rgb_planes(devs)
    eng = sj.Engine(0)

    def jpegs():
        out, szs, offs, _, _, _ = rs.encode_ragged_resampled(eng, sj.SRC_RGB, planes, dims, ENC_SIZES, ENC_ORIENTS, sj.YUV_420, _quant(), 0,
                                                            filter=ENC_FILTERS)
        torch.cuda.synchronize()
        return _streams(out, szs, offs)

    eng.trim()
    before = eng.scratch_bytes()
    first = jpegs()
    need = sum(x.shape[0] * ((x.shape[1] * 3 + 3) & ~3) for x in up)
    tables = sum(4 * (2 * o + o * rm.ksize(int(f), i, o)) for (w, h), (w2, h2), f in zip(ENC_DIMS, ENC_SIZES, ENC_FILTERS)
                 for i, o in ((w, w2), (h, h2)) if i != o)
    assert eng.scratch_bytes() >= before + need + tables
    grown = eng.scratch_bytes()
    eng.trim()
    assert eng.scratch_bytes() <= grown - need - tables
    assert jpegs() == first
