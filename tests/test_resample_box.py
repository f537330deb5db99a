"""Image.thumbnail and ImageOps.fit inside the ragged call on the GPU (sjpeg_hip_resample_box_ragged_src and the
_resampled_box_ entries; source_box=, reducing_gap=, thumbnail_images, fit_images and their encodes in
sjpeg_amd.resample), byte equality throughout.  The expectation is tests/resample_box_model.py -- the definition of
sjpeg_hip.h in numpy integers and Python doubles, which test_resample_box_model_host.py holds to what Pillow 12.2.0 made --
applied to the bytes the encoder sees; the fixture's own thumbnails and fits are made once more here and compared with
Pillow's recorded bytes directly.  Nothing below asks the library what a sample is."""
import os

import numpy as np
import pytest
import torch

import resample_box_model as bm
import resample_model as rm
import sjpeg_amd as sj
import sjpeg_amd.resample as rs
from oracle import synth
from test_flatten import ALPHA_FORMATS, AXFORM, _alphas, _flatten, _rgba_on_device, _seen_rgba
from test_reduce import FORMATS, XFORM3, _check_pictures, _on_device, _seen

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_pillow_box.npz")
# ((w, h), size, filter, source box, reducing_gap): the smallest shapes that can still go wrong
GEOMS = [((37, 29), (6, 7), rm.BICUBIC, None, 2.0),                               # factors (3, 2), neither side a multiple: four multipliers
         ((40, 30), (11, 9), rm.BICUBIC, (0.1, 0.2, 30.7, 20.3), None),            # a box whose double and float32 tables differ
         ((64, 48), (13, 7), rm.LANCZOS, (10.5, 8.25, 29.75, 21.5), None),         # an interior box: taps read outside it
         ((45, 45), (5, 5), rm.BOX, (0.3, 0.3, 44.6, 44.6), 1.5),                  # a box on the picture's edge: windows clamp
         ((64, 48), (8, 6), rm.BILINEAR, (5.5, 3.25, 60.0, 44.75), 1.0),           # a safe box whose origin is no multiple of the factor
         ((300, 160), (70, 37), rm.BICUBIC, None, 2.0),                            # more than one tile on both axes, partial last tiles
         ((300, 160), (70, 37), rm.HAMMING, (20.5, 10.5, 290.25, 150.75), 1.0),
         ((90, 20), (6, 9), rm.HAMMING, (11, 2, 83, 19), 3.0),                     # one axis reduced, the other enlarged
         ((31, 29), (40, 35), rm.BICUBIC, (2.3, 4.1, 17.9, 19.6), 2.0),            # a gap whose factors are both 1
         ((50, 40), (50, 40), rm.LANCZOS, None, None)]                             # the picture itself, beside reduced frames
assert {g[2] for g in GEOMS} == set(rm.FILTERS)


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
    """the pictures of GEOMS, u8 [H, W, 3]: random bytes and 0 / 255 noise in turn.  Never written to."""
    return [synth.g_noise(w, h, 9500 + k) if k % 2 == 0 else (synth.g_noise(w, h, 9500 + k) >> 7) * np.uint8(255) for k, ((w, h), *_) in enumerate(GEOMS)]


def _args(geoms):
    return dict(sizes=[g[1] for g in geoms], filter=[rs.Filter(g[2]) for g in geoms], source_box=[g[3] for g in geoms],
                reducing_gap=[g[4] for g in geoms])


def test_the_expectation_itself():
    (fx, fy), safe, size, inner = bm.decide(rm.BICUBIC, 37, 29, (6, 7), None, 2.0)
    assert (fx, fy) == (3, 2) and safe == (0, 0, 37, 29) and size == (13, 15)
    assert len({bm.multiplier(n) for n in (6, 2, 3, 1)}) == 4
    (fx, fy), safe, size, inner = bm.decide(rm.BILINEAR, 64, 48, (8, 6), GEOMS[4][3], 1.0)
    assert (fx, fy) == (6, 6) and safe[0] % fx != 0
    assert bm.decide(rm.BICUBIC, 31, 29, (40, 35), GEOMS[8][3], 2.0)[0] == (1, 1)
    single, double = bm.box_table(rm.BICUBIC, 40, 11, 0.1, 30.7), bm.box_table(rm.BICUBIC, 40, 11, 0.1, 30.7, double=True)
    assert not np.array_equal(single[1], double[1])
    # an interior box reads outside itself
    b, _ = bm.box_table(rm.LANCZOS, 64, 13, 10.5, 29.75)
    assert b[0, 0] < 10 and b[-1, 0] + b[-1, 1] > 30


# ---- 1. the kernel against the definition: ONE ragged call per staging class over every shape, filters mixed per frame

@pytest.mark.parametrize("name", ["RGB", "BGRA", "RGB_PLANAR", "GRAY", "RGB_F32", "GRAY_F16"])
def test_every_staging_class(engine, sources, name):
    """packed three and four bytes (the fourth dropped), planes, gray, float elements through a per-channel transform"""
    fmt, layout, dtype = FORMATS[name]
    if dtype is not None:
        engine.set_pixel_transform(*XFORM3[dtype])
    planes, keep, wants, dims = [], [], [], []
    for k, (u8, (_, size, filt, box, gap)) in enumerate(zip(sources, GEOMS)):
        p, dev, host = _on_device(u8, layout, dtype, seed=k, off=k % 3, pad=(k // 3) % 2)
        planes.append(p); keep.append(dev); dims.append((u8.shape[1], u8.shape[0]))
        wants.append(bm.resize(_seen(host, layout, dtype), size, filt, box, gap))
    a = _args(GEOMS)
    rfmt, pics, _ = rs.resample_ragged(engine, fmt, planes, dims, a["sizes"], a["filter"], source_box=a["source_box"], reducing_gap=a["reducing_gap"])
    engine.set_pixel_transform(255.0, 0.0)
    assert rfmt == (sj.SRC_GRAY if layout == "gray" else sj.SRC_RGB)
    _check_pictures(pics, wants)


@pytest.mark.parametrize("name", ["BGRA", "RGBA_F16"])
def test_the_flat_forms(engine, sources, name):
    """four bytes and four float elements a pixel, flattened over a background before they are summed"""
    fmt, layout, dtype = ALPHA_FORMATS[name]
    if dtype is not None:
        engine.set_pixel_transform(*XFORM3[dtype])
    bg = (17, 128, 250)
    flatten = sj.Flatten(bg, False, *(AXFORM[dtype] if dtype is not None else (255.0, 0.0)))
    planes, keep, wants, dims = [], [], [], []
    for k, (u8, (_, size, filt, box, gap)) in enumerate(zip(sources, GEOMS)):
        alpha = _alphas(u8.shape[1], u8.shape[0], 9550 + k)[0 if k % 4 else 3]
        p, dev, host = _rgba_on_device(u8, alpha, layout, dtype, seed=k, off=k % 3, pad=k % 2)
        s, al = _seen_rgba(host, layout, dtype)
        planes.append(p); keep.append(dev); dims.append((u8.shape[1], u8.shape[0]))
        wants.append(bm.resize(_flatten(s, al, bg, False), size, filt, box, gap))
    a = _args(GEOMS)
    rfmt, pics, _ = rs.resample_ragged(engine, fmt, planes, dims, a["sizes"], a["filter"], flatten=flatten, source_box=a["source_box"],
                                       reducing_gap=a["reducing_gap"])
    engine.set_pixel_transform(255.0, 0.0)
    assert rfmt == sj.SRC_RGB
    _check_pictures(pics, wants)


def test_pillows_rounding_not_the_half_up_average(engine):
    """24 x 24 to 8 x 8 with reducing_gap 1.0 is the reduce by 3 x 3 alone; the blocks' sums are those for which Pillow's
    rule and the exact half-up average of reduce_round.h disagree.  All-255 and all-0 pictures beside it."""
    n = 9
    sums = [S for S in range(255 * n + 1) if bm.reduce_sample(S, n) != bm.half_up(S, n)]
    assert len(sums) >= 64
    img = np.zeros((24, 24), np.uint8)
    for k in range(64):
        S = sums[k * len(sums) // 64]
        block = np.full(n, S // n, np.uint8)
        block[:S % n] += 1
        img[k // 8 * 3:k // 8 * 3 + 3, k % 8 * 3:k % 8 * 3 + 3] = block.reshape(3, 3)
    want = bm.resize(img, (8, 8), rm.BICUBIC, None, 1.0)
    assert np.array_equal(want, bm.reduce(img, 3, 3))
    wrong = ((2 * img.reshape(8, 3, 8, 3).astype(np.int64).sum(axis=(1, 3)) + n) // (2 * n)).astype(np.uint8)
    assert (want != wrong).all()
    ims = [img, np.full((24, 24), 255, np.uint8), np.zeros((24, 24), np.uint8)]
    devs = [torch.from_numpy(x).cuda() for x in ims]
    planes = [[(d.data_ptr(), d.stride(0))] for d in devs]
    _, pics, _ = rs.resample_ragged(engine, sj.SRC_GRAY, planes, [(24, 24)] * 3, [(8, 8)] * 3, rs.Filter.BICUBIC, reducing_gap=1.0)
    _check_pictures(pics, [want, np.full((8, 8), 255, np.uint8), np.zeros((8, 8), np.uint8)])
    # ... and with a resample behind the reduce, where an all-255 picture stays all 255
    _, pics, _ = rs.resample_ragged(engine, sj.SRC_GRAY, planes, [(24, 24)] * 3, [(5, 4)] * 3, rs.Filter.LANCZOS, reducing_gap=2.0)
    _check_pictures(pics, [bm.resize(x, (5, 4), rm.LANCZOS, None, 2.0) for x in ims])
    assert (pics[1].cpu().numpy() == 255).all() and (pics[2].cpu().numpy() == 0).all()


@pytest.mark.parametrize("name", ["RGB", "GRAY"])
def test_orientations_1_6_and_7(engine, name):
    """U = turn(R): boxes and sizes are in the stored orientation"""
    fmt, layout, dtype = FORMATS[name]
    u8 = synth.g_noise(57, 41, 9600)
    geoms = [((57, 41), (9, 6), rm.BICUBIC, (1.25, 0.5, 56.0, 40.5), 2.0), ((57, 41), (35, 17), rm.LANCZOS, (3.5, 2.5, 50.0, 40.0), None)]
    planes, keep, wants, dims, picked, orients = [], [], [], [], [], []
    for g in geoms:
        for o in (1, 6, 7):
            p, dev, host = _on_device(u8, layout, dtype, seed=o, off=o % 3, pad=o % 2)
            planes.append(p); keep.append(dev); dims.append((57, 41)); picked.append(g); orients.append(o)
            wants.append(np.ascontiguousarray(rm.turn(bm.resize(_seen(host, layout, dtype), g[1], g[2], g[3], g[4]), o)))
    a = _args(picked)
    _, pics, _ = rs.resample_ragged(engine, fmt, planes, dims, a["sizes"], a["filter"], orients, source_box=a["source_box"],
                                    reducing_gap=a["reducing_gap"])
    _check_pictures(pics, wants)


def test_the_reduce_lifts_the_cap(engine):
    """4000 x 8 to 40 x 4 with Lanczos: a window of 601 samples, refused; behind a reduce by 50 one of 13"""
    img = synth.g_noise(4000, 8, 9700)[..., 1].copy()
    dev = torch.from_numpy(img).cuda()
    planes = [[(dev.data_ptr(), dev.stride(0))]]
    with pytest.raises(sj.SjpegError, match="takes a window of 601 samples, above the cap of 385"):
        rs.resample_ragged(engine, sj.SRC_GRAY, planes, [(4000, 8)], [(40, 4)], rs.Filter.LANCZOS)
    assert bm.decide(rm.LANCZOS, 4000, 8, (40, 4), None, 2.0)[0] == (50, 1)
    _, pics, _ = rs.resample_ragged(engine, sj.SRC_GRAY, planes, [(4000, 8)], [(40, 4)], rs.Filter.LANCZOS, reducing_gap=2.0)
    _check_pictures(pics, [bm.resize(img, (40, 4), rm.LANCZOS, None, 2.0)])


def test_the_fixed_points(engine, sources):
    """no reduce and the whole box: byte for byte today's resample_images; a gap whose factors are both 1 changes nothing"""
    devs = [torch.from_numpy(x).cuda() for x in sources[:5]]
    sizes = [(30, 20), (40, 30), (90, 30), (23, 45), (64, 48)]
    filters = [rs.Filter(f) for f in rm.FILTERS]
    plain = [p.cpu().numpy() for p in rs.resample_images(devs, sizes, filters, engine=engine)]
    whole = [(0.0, 0.0, float(x.shape[1]), float(x.shape[0])) for x in sources[:5]]
    for kw in (dict(source_box=whole), dict(source_box=(0, 0, 0, 0)), dict(reducing_gap=1.0), dict(source_box=whole, reducing_gap=1.3)):
        if "reducing_gap" in kw:
            assert all(bm.decide(int(f), x.shape[1], x.shape[0], s, None, kw["reducing_gap"])[0] == (1, 1) for f, x, s in zip(filters, sources, sizes))
        _check_pictures(rs.resample_images(devs, sizes, filters, engine=engine, **kw), plain)
    _check_pictures([torch.from_numpy(x) for x in plain], [rm.resample(x, s, int(f)) for x, s, f in zip(sources, sizes, filters)])


# ---- 2. Image.thumbnail and ImageOps.fit, and the family's JPEG contract

def test_the_fixtures_thumbnails_and_fits_are_pillows_bytes(engine):
    g = np.load(GOLDEN)
    seen = set()
    for k, call in enumerate(g["calls"]):
        if call not in (3, 4):
            continue
        src, want, (f, w2, h2, _), d = g["in_%d" % k], g["out_%d" % k], g["ints"][k], g["doubles"][k]
        # (a gray picture goes as R = G = B: the channels are independent)
        dev = [torch.from_numpy(src if src.ndim == 3 else np.ascontiguousarray(np.repeat(src[..., None], 3, axis=2))).cuda()]
        if call == 3:
            got = rs.thumbnail_images(dev, (float(d[0]), float(d[1])), rs.Filter(int(f)), float(d[4]) or None, engine=engine)
        else:
            got = rs.fit_images(dev, (int(w2), int(h2)), rs.Filter(int(f)), float(d[0]), (float(d[1]), float(d[2])), engine=engine)
        torch.cuda.synchronize()
        got = got[0].cpu().numpy()
        assert np.array_equal(got if src.ndim == 3 else got[..., 1], want), (k, call)
        assert src.ndim == 3 or (got[..., 0] == got[..., 2]).all()
        seen.add(int(call))
    assert seen == {3, 4}


DIMS = [(128, 72), (48, 64), (33, 47), (20, 10)]


@pytest.fixture(scope="module")
def batch():
    ims = [synth.g_struct(w, h, 9800 + k) if k % 2 else synth.g_noise(w, h, 9800 + k) for k, (w, h) in enumerate(DIMS)]
    return ims, [torch.from_numpy(x).cuda() for x in ims]


@pytest.mark.parametrize("packed", [False, True])
def test_encode_thumbnails_and_encode_fitted_images(engine, risk_table, batch, packed):
    ims, devs = batch
    thumbs = [bm.thumbnail(x, (16, 16)) for x in ims]
    assert [t.shape[:2] for t in thumbs] == [(9, 16), (16, 12), (16, 11), (8, 16)]
    _check_pictures(rs.thumbnail_images(devs, (16, 16), engine=engine), thumbs)
    qs = [60.0, 75.0, 90.0, 50.0]
    want = sj.encode_images_full([torch.from_numpy(x).cuda() for x in thumbs], quality=qs, yuv_mode=sj.YUV_AUTO, engine=engine)
    assert rs.encode_thumbnails(devs, (16, 16), quality=qs, yuv_mode=sj.YUV_AUTO, packed=packed, engine=engine) == want
    fits = [bm.fit(x, (24, 16), rm.LANCZOS, 0.05, (0.3, 0.8)) for x in ims]
    _check_pictures(rs.fit_images(devs, (24, 16), rs.Filter.LANCZOS, 0.05, (0.3, 0.8), engine=engine), fits)
    want = sj.encode_images_full([torch.from_numpy(x).cuda() for x in fits], quality=80.0, yuv_mode=sj.YUV_420, engine=engine)
    assert rs.encode_fitted_images(devs, (24, 16), rs.Filter.LANCZOS, 0.05, (0.3, 0.8), quality=80.0, yuv_mode=sj.YUV_420, packed=packed,
                                   engine=engine) == want


def test_a_turned_thumbnail_with_metadata(engine, batch):
    ims, devs = batch
    orients = [6, 1, 7, 3]
    up = [np.ascontiguousarray(rm.turn(bm.thumbnail(x, (20, 14), rm.BICUBIC, 2.0), o)) for x, o in zip(ims, orients)]
    metas = [sj.PictureMetadata(exif=b"Exif\0\0" + bytes(range(40))), None, None, sj.PictureMetadata(xmp=b"<x:xmpmeta>thumbnail</x:xmpmeta>")]
    want = sj.encode_images_full_meta([torch.from_numpy(x).cuda() for x in up], metas, quality=80.0, yuv_mode=sj.YUV_420, engine=engine)
    assert rs.encode_thumbnails(devs, (20, 14), orientations=orients, metadata=metas, quality=80.0, yuv_mode=sj.YUV_420, engine=engine) == want


# ---- 3. the refusals, by name, before any device work

def test_the_named_refusals(engine, batch):
    ims, devs = batch
    one = devs[:1]
    for kw, words in ((dict(source_box=(0, 0, 128.5, 72)), "frame 0: box .* is empty or leaves the 128x72 picture"),
                      (dict(source_box=(-1, 0, 100, 72)), "is empty or leaves"), (dict(source_box=(5, 5, 5, 9)), "is empty or leaves"),
                      (dict(reducing_gap=0.5), "reducing_gap 0.5 is not None or a number of 1.0 or more")):
        with pytest.raises(sj.SjpegError, match=words):
            rs.resample_images(one, (16, 9), rs.Filter.BICUBIC, engine=engine, **kw)
        with pytest.raises(sj.SjpegError, match=words):
            rs.encode_resampled_images(one, sizes=(16, 9), filter=rs.Filter.BICUBIC, engine=engine, **kw)
    wide = [torch.zeros((2, 60000, 3), dtype=torch.uint8, device="cuda")]
    with pytest.raises(sj.SjpegError, match="frame 0: reduce factors 1500x2 are above the cap of 255"):
        rs.resample_images(wide, (40, 1), rs.Filter.BICUBIC, reducing_gap=1.0, engine=engine)
    tall = [torch.zeros((300, 2, 3), dtype=torch.uint8, device="cuda")]
    for call in (lambda: rs.resample_images(tall, (2, 299), rs.Filter.BICUBIC, source_box=(0, 0, 2, 300), engine=engine),
                 lambda: rs.thumbnail_images(tall, (2, 200), engine=engine),
                 lambda: rs.encode_fitted_images(tall, (2, 250), engine=engine)):
        with pytest.raises(sj.SjpegError, match="more than 100 times as tall as wide, brought to fewer rows is not made"):
            call()
    # (the plain call does not refuse it: its behaviour is unchanged)
    assert rs.resample_images(tall, (2, 299), rs.Filter.BICUBIC, engine=engine)[0].shape == (299, 2, 3)
    with pytest.raises(sj.SjpegError, match="one box or a sequence of one per frame"):
        rs.resample_images(devs, (16, 9), source_box=[(0, 0, 5, 5)] * 3, engine=engine)
