"""Pillow's BoxBlur, GaussianBlur and UnsharpMask inside the ragged call on the GPU (sjpeg_hip_filter_ragged_src and the
_filtered_ entries; post= in sjpeg_amd.resample), byte equality throughout.  The expectation is
tests/pillow_filter_model.py -- the definition of sjpeg_hip.h in numpy integers and float32 scalars, which
test_pillow_filter_model_host.py holds to what Pillow 12.2.0 made -- applied to the upright picture
tests/resample_box_model.py makes of the bytes the encoder sees: filter(turn(resample(flatten(stored)))).  The
fixture's own chain, thumbnail then UnsharpMask(2, 150, 3), is made once more here and compared with Pillow's recorded
bytes directly.  Nothing below asks the library what a sample is."""
import os

import numpy as np
import pytest
import torch

import pillow_filter_cases as pc
import pillow_filter_model as pm
import resample_box_model as bm
import resample_model as rm
import sjpeg_amd as sj
import sjpeg_amd.resample as rs
import sjpeg_amd.unsharp as un
from oracle import synth
from test_reduce import FORMATS, XFORM3, _check_pictures, _on_device, _seen

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pillow_filter.npz"))
# ((w, h), size, resample filter, post): the smallest thumbnails that can still go wrong, kinds mixed in ONE call
GEOMS = [((3, 2), (1, 1), rm.BOX, ("gaussian", 2)),                                # a degenerate line
         ((9, 11), (5, 7), rm.BICUBIC, ("box", 5)),                                # both clamps at once
         ((90, 50), (70, 37), rm.BICUBIC, ("gaussian", 2)),                        # a partial last tile
         ((300, 160), (300, 160), rm.LANCZOS, ("gaussian", 2)),                    # a frame at its own size; more than one tile on both axes
         ((310, 170), (300, 160), rm.BILINEAR, ("gaussian", (1.5, 4))),            # ... seams with two radii
         ((300, 20), (300, 20), rm.BICUBIC, ("box", 63)),                          # r = 63, one pass: a halo of 64
         ((40, 310), (20, 300), rm.HAMMING, ("box", 63.9)),                        # the same, for columns
         ((640, 6), (640, 6), rm.BICUBIC, ("gaussian", 64)),                       # r = 63, THREE passes: a halo of 192 on both sides of
         ((12, 610), (6, 600), rm.BILINEAR, ("unsharp", 64, 150, 3)),              # interior tiles, wider than the tile; the LDS is full
         ((50, 40), (33, 27), rm.BICUBIC, None),                                   # kind 0 beside the others: the made picture
         ((60, 45), (41, 33), rm.BICUBIC, ("unsharp", 2, 150, 3)),                 # the unsharp cases of the host list
         ((30, 20), (17, 9), rm.LANCZOS, ("unsharp", 0.6, 500, 1)),
         ((30, 20), (17, 9), rm.BOX, ("unsharp", 1, 80, 0)),
         ((20, 20), (5, 7), rm.BICUBIC, ("unsharp", 2, 150, 255)),
         ((4, 6), (2, 3), rm.BILINEAR, ("unsharp", 0, 150, 0)),
         ((40, 30), (33, 27), rm.BICUBIC, ("box", (0, 2))),                        # a skipped axis: copied by the row launch
         ((40, 30), (33, 27), rm.BICUBIC, ("gaussian", (3.3, 0)))]


def _post(spec):
    if spec is None:
        return None
    if spec[0] == "box":
        return rs.PillowFilter.box_blur(spec[1])
    if spec[0] == "gaussian":
        return rs.PillowFilter.gaussian_blur(spec[1])
    return rs.PillowFilter.unsharp_mask(*spec[1:])


ENTRIES = ("sjpeg_hip_pillow_filter_weights", "sjpeg_hip_filter_ragged_src", "sjpeg_hip_encode_ragged_filtered_src",
           "sjpeg_hip_encode_ragged_filtered_packed_src")


@pytest.fixture(scope="module", autouse=True)
def the_entries_are_exported():
    """everything below is about these entries: the library declares and exports them"""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sjpeg_hip.h")).read()
    for name in ENTRIES:
        assert name in sj.EXPORTED_C_SYMBOLS and hasattr(rs._lib(), name) and name + "(" in header, name


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
    return [synth.g_noise(w, h, 9900 + k) if k % 2 == 0 else (synth.g_noise(w, h, 9900 + k) >> 7) * np.uint8(255) for k, ((w, h), *_) in enumerate(GEOMS)]


_WANTS = {}


def _want(k, seen):
    """filter(resample(seen)) of GEOMS[k], computed once per distinct picture the encoder sees"""
    key = (k, seen.shape, seen.tobytes())
    if key not in _WANTS:
        _, size, filt, spec = GEOMS[k]
        _WANTS[key] = pm.apply(bm.resize(seen, size, filt, None, None), spec)
    return _WANTS[key]


def test_the_expectation_itself():
    assert pm.axis_weights(pm.BOX, 5)[0] == 5 and pm.axis_weights(pm.BOX, 63)[0] == 63 and pm.axis_weights(pm.BOX, 63.9)[0] == 63
    assert pm.axis_weights(pm.GAUSSIAN, 2)[:1] == (1,) and pm.axis_weights(pm.GAUSSIAN, 4)[0] == 3 and pm.axis_weights(pm.GAUSSIAN, 0)[3] == 0
    # 300 x 160 is more than one tile of either launch on both axes (128 pixels, 64 rows).  Sigma 64 is r = 63 three
    # times: a halo of 192, wider than either tile, and whole on both sides of the row tile [256, 384) of 640 pixels and
    # of the column tile [192, 256) of 600 rows
    assert 300 > 128 and 160 > 64
    assert pm.axis_weights(pm.GAUSSIAN, 64)[0] == 63 and pm.axis_weights(pm.GAUSSIAN, 64)[3] == 3
    halo = 3 * (63 + 1)
    assert halo > 128 and 256 - halo >= 0 and 384 + halo <= 640 and 192 - halo >= 0 and 256 + halo <= 600
    img = pc.picture("RGB", (17, 9), 3)
    assert not np.array_equal(pm.gaussian_blur(img, (1.5, 4)), pm.gaussian_blur(img, (4, 1.5)))


# ---- 1. the kernel against the definition: ONE ragged call per staging class over every shape, kinds mixed per frame

@pytest.mark.parametrize("name", ["RGB", "BGRA", "RGB_PLANAR", "GRAY", "RGB_F32"])
def test_every_staging_class(engine, sources, name):
    """packed three and four bytes (the fourth dropped), planes, gray, float elements through a per-channel transform"""
    fmt, layout, dtype = FORMATS[name]
    if dtype is not None:
        engine.set_pixel_transform(*XFORM3[dtype])
    planes, keep, wants, dims = [], [], [], []
    for k, (u8, (_, size, filt, spec)) in enumerate(zip(sources, GEOMS)):
        p, dev, host = _on_device(u8, layout, dtype, seed=k, off=k % 3, pad=(k // 3) % 2)
        planes.append(p); keep.append(dev); dims.append((u8.shape[1], u8.shape[0]))
        wants.append(_want(k, _seen(host, layout, dtype)))
    rfmt, pics, _ = rs.resample_ragged(engine, fmt, planes, dims, [g[1] for g in GEOMS], [rs.Filter(g[2]) for g in GEOMS],
                                       post=[_post(g[3]) for g in GEOMS])
    engine.set_pixel_transform(255.0, 0.0)
    assert rfmt == (sj.SRC_GRAY if layout == "gray" else sj.SRC_RGB)
    _check_pictures(pics, wants)


@pytest.mark.parametrize("name", ["RGB", "GRAY"])
def test_the_eight_orientations_with_two_radii(engine, name):
    """the filter runs over the UPRIGHT picture: filter(turn(...)), rx along its rows"""
    fmt, layout, dtype = FORMATS[name]
    u8 = synth.g_noise(57, 41, 9950)
    specs = [("gaussian", (1.5, 4)), ("box", (3, 0.7))]
    planes, keep, wants, dims, orients, posts = [], [], [], [], [], []
    for o in range(1, 9):
        p, dev, host = _on_device(u8, layout, dtype, seed=o, off=o % 3, pad=o % 2)
        made = np.ascontiguousarray(rm.turn(bm.resize(_seen(host, layout, dtype), (23, 17), rm.BICUBIC, None, 2.0), o))
        spec = specs[o % 2]
        planes.append(p); keep.append(dev); dims.append((57, 41)); orients.append(o); posts.append(_post(spec))
        wants.append(pm.apply(made, spec))
        swapped = (spec[0], spec[1][::-1])
        assert not np.array_equal(pm.apply(made, swapped), wants[-1])
    _, pics, _ = rs.resample_ragged(engine, fmt, planes, dims, [(23, 17)] * 8, rs.Filter.BICUBIC, orients, reducing_gap=2.0, post=posts)
    _check_pictures(pics, wants)


def test_trap_3_on_the_device(engine):
    """a difference equal to the threshold leaves the sample; one below it does not"""
    img, thr = pc.trap3_picture(), pc.trap3_threshold()
    dev = torch.from_numpy(img).cuda()
    planes = [[(dev.data_ptr(), dev.stride(0))]] * 2
    posts = [rs.PillowFilter.unsharp_mask(pc.TRAP3_RADIUS, 150, thr), rs.PillowFilter.unsharp_mask(pc.TRAP3_RADIUS, 150, thr - 1)]
    _, pics, _ = rs.resample_ragged(engine, sj.SRC_GRAY, planes, [(9, 9)] * 2, None, rs.Filter.BICUBIC, post=posts)
    _check_pictures(pics, [GOLDEN["trap3_out"], pm.unsharp_mask(img, pc.TRAP3_RADIUS, 150, thr - 1)])
    got = [p.cpu().numpy() for p in pics]
    assert got[0][4, 4] == img[4, 4] and got[1][4, 4] != img[4, 4]


# ---- 2. the chain of a Python thumbnailer, and the family's JPEG contract

def test_the_fixtures_chain_is_pillows_bytes(engine):
    """im.thumbnail(box); im.filter(UnsharpMask(2, 150, 3)) -- made on the GPU, compared with what Pillow recorded"""
    dev = [torch.from_numpy(pc.chain_picture()).cuda()]
    _check_pictures(rs.thumbnail_images(dev, pc.CHAIN_BOX, engine=engine), [GOLDEN["chain_thumbnail"]])
    _check_pictures(rs.thumbnail_images(dev, pc.CHAIN_BOX, post=rs.PillowFilter.unsharp_mask(), engine=engine), [GOLDEN["chain"]])


DIMS = [(128, 72), (48, 64), (33, 47), (20, 10)]
POSTS = [("unsharp", 2, 150, 3), ("gaussian", 3), None, ("box", (1, 2.5))]


@pytest.fixture(scope="module")
def batch():
    ims = [synth.g_struct(w, h, 9960 + k) if k % 2 else synth.g_noise(w, h, 9960 + k) for k, (w, h) in enumerate(DIMS)]
    return ims, [torch.from_numpy(x).cuda() for x in ims]


@pytest.mark.parametrize("packed", [False, True])
def test_the_encode_entries_jpegs(engine, risk_table, batch, packed):
    """the JPEGs of the encode and packed entries are encode_images_full of the model's pictures"""
    ims, devs = batch
    posts = [_post(s) for s in POSTS]
    thumbs = [pm.apply(bm.thumbnail(x, (32, 32)), s) for x, s in zip(ims, POSTS)]
    _check_pictures(rs.thumbnail_images(devs, (32, 32), post=posts, engine=engine), thumbs)
    qs = [60.0, 75.0, 90.0, 50.0]
    want = sj.encode_images_full([torch.from_numpy(x).cuda() for x in thumbs], quality=qs, yuv_mode=sj.YUV_AUTO, engine=engine)
    assert rs.encode_thumbnails(devs, (32, 32), post=posts, quality=qs, yuv_mode=sj.YUV_AUTO, packed=packed, engine=engine) == want
    one = rs.PillowFilter.gaussian_blur(8)
    fits = [pm.gaussian_blur(bm.fit(x, (24, 16), rm.LANCZOS, 0.05, (0.3, 0.8)), 8) for x in ims]
    want = sj.encode_images_full([torch.from_numpy(x).cuda() for x in fits], quality=80.0, yuv_mode=sj.YUV_420, engine=engine)
    assert rs.encode_fitted_images(devs, (24, 16), rs.Filter.LANCZOS, 0.05, (0.3, 0.8), post=one, quality=80.0, yuv_mode=sj.YUV_420, packed=packed,
                                   engine=engine) == want
    sized = [pm.box_blur(bm.resize(x, (20, 12), rm.LANCZOS, None, None), 2) for x in ims]
    want = sj.encode_images_full([torch.from_numpy(x).cuda() for x in sized], quality=70.0, yuv_mode=sj.YUV_444, engine=engine)
    assert rs.encode_resampled_images(devs, sizes=(20, 12), post=rs.PillowFilter.box_blur(2), quality=70.0, yuv_mode=sj.YUV_444, packed=packed,
                                      engine=engine) == want
    _check_pictures(rs.resample_images(devs, (20, 12), post=rs.PillowFilter.box_blur(2), engine=engine), sized)
    _check_pictures(rs.fit_images(devs, (24, 16), rs.Filter.LANCZOS, 0.05, (0.3, 0.8), post=one, engine=engine), fits)


def test_no_filter_is_the_box_call_byte_for_byte(engine, batch):
    """post=None, and kind 0 for every frame, answer as the _resampled_box_ entry does: pictures, JPEGs and messages"""
    ims, devs = batch
    plain = [p.cpu().numpy() for p in rs.thumbnail_images(devs, (32, 32), engine=engine)]
    _check_pictures(rs.thumbnail_images(devs, (32, 32), post=None, engine=engine), plain)
    _check_pictures(rs.thumbnail_images(devs, (32, 32), post=[None] * 4, engine=engine), plain)
    _check_pictures(rs.thumbnail_images(devs, (32, 32), post=rs.PillowFilter.none(), engine=engine), plain)
    # ... and a frame of kind 0 beside filtered ones is the made picture
    mixed = rs.thumbnail_images(devs, (32, 32), post=[rs.PillowFilter.gaussian_blur(2), None, None, rs.PillowFilter.box_blur(1)], engine=engine)
    _check_pictures(mixed[1:3], plain[1:3])
    want = rs.encode_thumbnails(devs, (32, 32), quality=75.0, yuv_mode=sj.YUV_420, engine=engine)
    for packed in (False, True):
        assert rs.encode_thumbnails(devs, (32, 32), post=[None] * 4, quality=75.0, yuv_mode=sj.YUV_420, packed=packed, engine=engine) == want
    with pytest.raises(sj.SjpegError, match="sjpeg_hip_resample_box_ragged_src: frame 0: box .* is empty or leaves"):
        rs.resample_images(devs[:1], (16, 9), source_box=(0, 0, 128.5, 72), post=[None], engine=engine)


# ---- 3. the refusals, by name, before any device work

def test_the_named_refusals(engine, batch):
    ims, devs = batch
    F = rs.PillowFilter
    for post, words in (([None, F.box_blur(64), None, None], "frame 1: filter: radius_x gives a box radius above 63 \\(Pillow has no such limit"),
                        ([None, None, F.gaussian_blur((1, 70)), None], "frame 2: filter: radius_y gives a box radius above 63"),
                        (F.gaussian_blur(float("nan")), "filter: radius_x is not a finite number of 0 or more"),
                        ([None, None, None, F.box_blur((1, -2))], "frame 3: filter: radius_y is not a finite number of 0 or more"),
                        ([F(3, (2, 3), 150, 3), None, None, None], "frame 0: filter: an unsharp mask has one radius")):
        with pytest.raises(sj.SjpegError, match="sjpeg_hip_filter_ragged_src: " + words):
            rs.thumbnail_images(devs, (32, 32), post=post, engine=engine)
        with pytest.raises(sj.SjpegError, match="sjpeg_hip_encode_ragged_filtered_src: " + words):
            rs.encode_thumbnails(devs, (32, 32), post=post, engine=engine)
        with pytest.raises(sj.SjpegError, match="sjpeg_hip_encode_ragged_filtered_packed_src: " + words):
            rs.encode_thumbnails(devs, (32, 32), post=post, packed=True, engine=engine)
    with pytest.raises(sj.SjpegError, match="encode_resampled_images: post= and unsharp= are both given"):
        rs.encode_thumbnails(devs, (32, 32), post=F.unsharp_mask(), unsharp=un.Unsharp(16), engine=engine)
    with pytest.raises(sj.SjpegError, match="resample_ragged: post= and unsharp= are both given"):
        rs.resample_ragged(engine, sj.SRC_RGB, [[(devs[0].data_ptr(), devs[0].stride(0))]], [DIMS[0]], None, post=F.unsharp_mask(), unsharp=un.Unsharp(16))
    # the box entries' refusals, under this entry's name
    with pytest.raises(sj.SjpegError, match="sjpeg_hip_filter_ragged_src: frame 0: box .* is empty or leaves"):
        rs.resample_images(devs[:1], (16, 9), source_box=(0, 0, 128.5, 72), post=F.box_blur(1), engine=engine)
