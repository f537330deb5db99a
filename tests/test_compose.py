"""The compose stage inside the ragged call on the GPU (sjpeg_hip_compose_ragged_src and the _composed_ entries;
compose= in sjpeg_amd.resample), byte equality throughout.  The expectation is tests/compose_model.py -- the definition
of sjpeg_hip.h in numpy integers, which test_compose_model_host.py holds to what Pillow 12.2.0 made -- applied to what
tests/pillow_filter_model.py and tests/resample_box_model.py make of the bytes the encoder sees:
compose(filter(turn(resample(stored)))).  The fixture's own chain -- thumbnail, UnsharpMask, ImageOps.pad, paste -- and
its pad pictures are made once more here and compared with Pillow's recorded bytes directly.  Nothing below asks the
library what a sample is."""
import os

import numpy as np
import pytest
import torch

import compose_cases as cc
import compose_model as cm
import pillow_filter_cases as pc
import pillow_filter_model as pm
import resample_box_model as bm
import resample_model as rm
import sjpeg_amd as sj
import sjpeg_amd.resample as rs
from test_reduce import _check_pictures

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compose_pillow.npz"))
ENTRIES = ("sjpeg_hip_contain_size", "sjpeg_hip_pad_place", "sjpeg_hip_compose_sample", "sjpeg_hip_compose_ragged_bytes",
           "sjpeg_hip_compose_ragged_src", "sjpeg_hip_encode_ragged_composed_src", "sjpeg_hip_encode_ragged_composed_packed_src")
UNSHARP = ("unsharp", 2, 150, 3)


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


def _rgba(w, h, seed, alpha=None):
    a = np.ascontiguousarray(np.concatenate([pc.picture("RGB", (w, h), seed), pc.picture("L", (w, h), seed + 1)[..., None]], axis=2))
    if alpha is not None:
        a[..., 3] = alpha
    return a


class Logos:
    """the overlays of the batch, on the host and on the device: 0 random, 1 a crop of a larger tensor (a stride above
    4 * width), 2 alpha all 0, 3 alpha all 255, 4 larger than the small canvases, 5 half white, 6 half black"""

    def __init__(self):
        big = _rgba(12, 10, 701)
        self.big = torch.from_numpy(big).cuda()
        self.host = [_rgba(4, 3, 700), np.ascontiguousarray(big[2:6, 3:8]), _rgba(3, 3, 702, 0), _rgba(3, 2, 703, 255), _rgba(40, 30, 704),
                     cc.overlay(0), cc.overlay(1)]
        devs = [torch.from_numpy(h).cuda() for h in self.host]
        devs[1] = self.big[2:6, 3:8]
        self.dev = [rs.Overlay(d) for d in devs]
        assert self.dev[1].stride == 48 and self.dev[1].width == 5


@pytest.fixture(scope="module")
def logos():
    return Logos()


def _frames(L):
    """((w, h) of the source, size, post spec, orientation, compose as the model's keywords with overlays by index) of
    the mixed batch: the smallest geometries that can still go wrong, in ONE call"""
    def at(canvas, xy, overlays=()):
        return dict(canvas=canvas, at=xy, colour=(10, 200, 90), overlays=list(overlays))
    f = [((3, 2), (1, 1), None, 1, at((2, 2), (1, 1)))]                                                # 1: 1 x 1 at (1, 1)
    f += [((9, 6), (5, 3), None, 1, at((10, 5), (px, 1))) for px in (1, 2, 3)]                         # 2: every phase of 3 * px; 30 bytes a row
    f += [((9, 6), (5, 3), UNSHARP, 1, at((9, 6), (4, 3)))]                                             # 3: the right and the bottom edge
    f += [((260, 15), (250, 11), None, 1, at((300, 20), (37, 5), [(0, (60, 14), 0), (1, (2, 2), 3)])),  # 4: tile seams on both axes
          ((20, 280), (13, 270), ("gaussian", 1.5), 1, at((20, 300), (3, 17), [(1, (1, 150), 1), (3, (0, 15), 0)]))]
    f += [((12, 9), (7, 4), None, 1, None),                                                             # 5: no compose
          ((80, 40), (70, 33), None, 1, dict(canvas=(90, 35), centering=(0.5, 0.5), colour=(1, 2, 3)))]  # ... a canvas and no place
    f += [((12, 9), (9, 8), None, 1, at((12, 10), (1, 1), [(0, (-2, 3), 0), (0, (-2, 3), 1), (0, (3, -1), 0), (0, (3, -1), 2), (0, (50, 50), 0),
                                                           (0, (-20, 0), 0)]))]                        # 6: over each edge, and wholly outside
    f += [((12, 9), (9, 8), None, 1, at((12, 10), (2, 1), [(4, (0, 0), 4)]))]                           # 7: the whole canvas, padding included
    f += [((12, 9), (9, 8), None, 1, at((12, 10), (2, 1), [(5, (2, 2), 0), (6, (4, 3), 0)])),           # 8: two that overlap, both orders
          ((12, 9), (9, 8), None, 1, at((12, 10), (2, 1), [(6, (4, 3), 0), (5, (2, 2), 0)]))]
    f += [((40, 30), (30, 20), ("box", 1), 1, at((33, 22), (1, 1), [(0, (0, 0), 0), (1, (0, 0), 1), (2, (0, 0), 2), (3, (0, 0), 3), (0, (0, 0), 4),
                                                                   (5, (1, 1), 0), (6, (2, 2), 4), (1, (3, 3), 3)]))]   # 9: eight places
    f += [((40, 30), (30, 20), None, 6, dict(canvas=(40, 40), centering=(0.3, 0.6), colour=(250, 240, 20), overlays=[(0, (8, 8), 3)]))]   # 14
    f += [((140, 40), (130, 35), None, 1, dict(canvas=None, overlays=[(2, (5, 5), 0), (3, (64, 15), 0)]))]   # its own size, overlays on a seam
    return f


def _model(made, kw, L):
    if kw is None:
        return made
    kw = dict(kw)
    kw["overlays"] = [(L.host[o], xy, anchor) for o, xy, anchor in kw.get("overlays", ())]
    return cm.compose(made, **kw)


def _compose(kw, L):
    if kw is None:
        return None
    kw = dict(kw)
    kw["overlays"] = [(L.dev[o], xy, anchor) for o, xy, anchor in kw.get("overlays", ())]
    return rs.Compose(**kw)


_BATCH = {}


def _batch(L):
    """the mixed batch, made once: sources on the device, the call's arguments, the model's canvases.  Never written to."""
    if not _BATCH:
        fr = _frames(L)
        srcs = [pc.picture("RGB", wh, 800 + k) for k, (wh, *_) in enumerate(fr)]
        wants = []
        for img, (_, size, spec, o, kw) in zip(srcs, fr):
            stored = (size[1], size[0]) if o >= 5 else size
            made = np.ascontiguousarray(rm.turn(bm.resize(img, stored, rm.BICUBIC, None, None), o))
            assert made.shape[:2] == (size[1], size[0])
            wants.append(_model(pm.apply(made, spec) if spec else made, kw, L))
        _BATCH.update(devs=[torch.from_numpy(x).cuda() for x in srcs], wants=wants,
                      sizes=[((s[1], s[0]) if o >= 5 else s) for _, s, _, o, _ in fr], orients=[o for *_, o, _ in fr],
                      posts=[None if s is None else {"unsharp": rs.PillowFilter.unsharp_mask, "gaussian": rs.PillowFilter.gaussian_blur,
                                                     "box": rs.PillowFilter.box_blur}[s[0]](*s[1:]) for _, _, s, _, _ in fr],
                      composes=[_compose(kw, L) for *_, kw in fr])
    return _BATCH


def test_the_expectation_itself(logos):
    """the geometries are what they claim: seams of the 64-dword x 16-row tile, a padded last dword, an order that matters"""
    b = _batch(logos)
    assert (300 * 3 + 3) // 4 > 3 * 64 and 20 > 16 and 300 > 16 * 18 and (10 * 3) % 4 != 0
    assert [c.shape for c in b["wants"][:5]] == [(2, 2, 3)] + [(5, 10, 3)] * 3 + [(6, 9, 3)]
    assert not np.array_equal(b["wants"][11], b["wants"][12])
    assert b["wants"][14].shape == (40, 40, 3) and b["orients"][14] == 6 and sum(p is not None for p in b["posts"]) == 3
    assert cm.blend(cm.blend(0, 255, 128), 0, 128) == 64 and cm.blend(cm.blend(0, 0, 128), 255, 128) == 128


def test_the_mixed_batch_in_one_call(engine, logos):
    b = _batch(logos)
    pics = rs.resample_images(b["devs"], b["sizes"], rs.Filter.BICUBIC, orientations=b["orients"], post=b["posts"], compose=b["composes"],
                              engine=engine)
    _check_pictures(pics, b["wants"])


@pytest.mark.parametrize("packed", [False, True])
def test_the_encode_entries_jpegs(engine, risk_table, logos, packed):
    """each JPEG of the composed entries is encode_images_full of the model's canvas picture"""
    b = _batch(logos)
    qs = [50.0 + (7 * k) % 45 for k in range(len(b["devs"]))]
    want = sj.encode_images_full([torch.from_numpy(x).cuda() for x in b["wants"]], quality=qs, yuv_mode=sj.YUV_AUTO, engine=engine)
    got = rs.encode_resampled_images(b["devs"], sizes=b["sizes"], filter=rs.Filter.BICUBIC, orientations=b["orients"], post=b["posts"],
                                     compose=b["composes"], quality=qs, yuv_mode=sj.YUV_AUTO, packed=packed, engine=engine)
    assert got == want


def test_a_gray_source_with_a_canvas_and_an_overlay(engine, logos):
    """the luma of the overlay's colour is blended; the canvas is colour[0]"""
    imgs = [pc.picture("L", (31, 17), 900), cc.base("L", (31, 17), 50 + 4)]
    devs = [torch.from_numpy(x).cuda() for x in imgs]
    planes = [[(d.data_ptr(), d.stride(0))] for d in devs]
    size = rs.contain_size(31, 17, (23, 23))
    comps = [rs.Compose(canvas=(37, 21), at=(3, 2), colour=(77, 1, 2), overlays=[(logos.dev[0], (1, 1), "bottom-right"), (logos.dev[1], (-2, 0), 0)]),
             rs.Compose.pad((23, 23), 77)]
    rfmt, pics, _ = rs.resample_ragged(engine, sj.SRC_GRAY, planes, [(31, 17)] * 2, [(31, 17), size], rs.Filter.BICUBIC, compose=comps)
    assert rfmt == sj.SRC_GRAY
    want0 = cm.compose(imgs[0], (37, 21), at=(3, 2), colour=(77, 1, 2), overlays=[(logos.host[0], (1, 1), 3), (logos.host[1], (-2, 0), 0)])
    _check_pictures(pics, [want0, GOLDEN["pad_4"]])


def test_one_struct_for_pictures_of_three_sizes(engine, logos):
    """compose_per_frame = 0: pad to 40 x 40 by a centering and a logo 2, 3 from the bottom-right corner"""
    imgs = [pc.smooth_picture(w, h, 3, 910 + k) for k, (w, h) in enumerate(((128, 72), (48, 64), (33, 47)))]
    devs = [torch.from_numpy(x).cuda() for x in imgs]
    one = rs.Compose.pad((40, 40), (250, 240, 20), (0.3, 0.6), overlays=[(logos.dev[0], (2, 3), "bottom-right")])
    keep = rs._ComposeArgs("t", 3, one, [(1, 1)] * 3)
    assert keep.args[1] == 0 and len(keep.carr) == 1
    wants = [cm.compose(bm.thumbnail(x, (32, 32)), (40, 40), centering=(0.3, 0.6), colour=(250, 240, 20), overlays=[(logos.host[0], (2, 3), 3)])
             for x in imgs]
    _check_pictures(rs.thumbnail_images(devs, (32, 32), compose=one, engine=engine), wants)


def test_the_fixtures_chain_is_pillows_bytes(engine, risk_table):
    """thumbnail((40, 40)); filter(UnsharpMask(2, 150, 3)); ImageOps.pad((40, 40), color); paste(logo) -- made on the
    GPU, compared with what Pillow recorded"""
    logo = rs.Overlay(torch.from_numpy(cc.logo()).cuda())
    comp = rs.Compose.pad(cc.CHAIN_BOX, cc.CHAIN_COLOUR, overlays=[(logo, cc.CHAIN_LOGO_AT, "top-left")])
    devs = [torch.from_numpy(cc.chain_source(k)).cuda() for k in range(2)]
    wants = [GOLDEN["chain_%d" % k] for k in range(2)]
    _check_pictures(rs.thumbnail_images(devs, cc.CHAIN_BOX, post=rs.PillowFilter.unsharp_mask(), engine=engine), [GOLDEN["chain_%d_sharp" % k] for k in range(2)])
    _check_pictures(rs.thumbnail_images(devs, cc.CHAIN_BOX, post=rs.PillowFilter.unsharp_mask(), compose=comp, engine=engine), wants)
    want = sj.encode_images_full([torch.from_numpy(x).cuda() for x in wants], quality=80.0, yuv_mode=sj.YUV_420, engine=engine)
    assert rs.encode_thumbnails(devs, cc.CHAIN_BOX, post=rs.PillowFilter.unsharp_mask(), compose=comp, quality=80.0, yuv_mode=sj.YUV_420,
                                engine=engine) == want


def test_pad_images_against_the_fixtures_pad_pictures(engine):
    for k, (mode, size, box, colour, centering) in enumerate(cc.PADS):
        if mode != "RGB":
            continue                                                # (the gray case: test_a_gray_source_with_a_canvas_and_an_overlay)
        dev = [torch.from_numpy(cc.base(mode, size, 50 + k)).cuda()]
        _check_pictures(rs.pad_images(dev, box, colour=colour, centering=centering, engine=engine), [GOLDEN["pad_%d" % k]])
    # orientation 6: ImageOps.pad of the UPRIGHT picture
    img = cc.base("RGB", (31, 17), 52)
    stored = np.ascontiguousarray(rm.turn(img, 8))                 # (turned by 6 it is img again)
    assert np.array_equal(rm.turn(stored, 6), img)
    got = rs.pad_images([torch.from_numpy(stored).cuda()], (23, 23), colour=(9, 99, 199), centering=(0.2, 0.8), orientations=6, engine=engine)
    assert got[0].shape == (23, 23, 3)
    size = cm.contain_size(31, 17, (23, 23))
    made = np.ascontiguousarray(rm.turn(bm.resize(stored, (size[1], size[0]), rm.BICUBIC, None, None), 6))
    _check_pictures(got, [cm.compose(made, (23, 23), centering=(0.2, 0.8), colour=(9, 99, 199))])
    jpegs = rs.encode_padded_images([torch.from_numpy(cc.base("RGB", (90, 50), 50)).cuda()], (40, 40), colour=(250, 240, 20), quality=75.0,
                                    yuv_mode=sj.YUV_420, engine=engine)
    assert jpegs == sj.encode_images_full([torch.from_numpy(GOLDEN["pad_0"]).cuda()], quality=75.0, yuv_mode=sj.YUV_420, engine=engine)


def test_the_identity_route_is_the_call_without_compose(engine, logos):
    """compose=None, a Compose of nothing, and a canvas of the picture's own size answer as the call without compose:
    pictures, JPEGs and messages under the other entry's name"""
    imgs = [pc.smooth_picture(w, h, 3, 920 + k) for k, (w, h) in enumerate(((128, 72), (48, 64)))]
    devs = [torch.from_numpy(x).cuda() for x in imgs]
    post = rs.PillowFilter.gaussian_blur(2)
    plain = [p.cpu().numpy() for p in rs.thumbnail_images(devs, (32, 32), post=post, engine=engine)]
    own = [rs.Compose(canvas=(p.shape[1], p.shape[0]), at=(0, 0)) for p in plain]
    for comp in (rs.Compose(), [None, None], own, [rs.Compose(), own[1]]):
        _check_pictures(rs.thumbnail_images(devs, (32, 32), post=post, compose=comp, engine=engine), plain)
    want = rs.encode_thumbnails(devs, (32, 32), post=post, quality=75.0, engine=engine)
    for packed in (False, True):
        assert rs.encode_thumbnails(devs, (32, 32), post=post, compose=own, quality=75.0, packed=packed, engine=engine) == want
    with pytest.raises(sj.SjpegError, match="sjpeg_hip_resample_box_ragged_src: frame 0: box .* is empty or leaves"):
        rs.resample_images(devs[:1], (16, 9), source_box=(0, 0, 128.5, 72), compose=[None], engine=engine)
    with pytest.raises(sj.SjpegError, match="sjpeg_hip_filter_ragged_src: frame 0: box .* is empty or leaves"):
        rs.resample_images(devs[:1], (16, 9), source_box=(0, 0, 128.5, 72), post=post, compose=rs.Compose(), engine=engine)


def test_the_named_refusals(engine, logos):
    devs = [torch.from_numpy(pc.picture("RGB", (20, 10), 930 + k)).cuda() for k in range(2)]
    for comp, words in (([None, rs.Compose(canvas=(9, 9), at=(0, 0))], "frame 1: compose: the 10x5 picture at \\(0, 0\\) is not wholly inside the 9x9 canvas"),
                        (rs.Compose(canvas=(12, 12), at=(3, 0)), "frame 0: compose: the 10x5 picture at \\(3, 0\\) is not wholly inside"),
                        (rs.Compose(canvas=(70000, 12)), "compose: canvas 70000x12 is not 0x0"),
                        ([rs.Compose(canvas=(12, 12), centering=(float("nan"), 0.5)), None], "frame 0: compose: the centering is not finite")):
        with pytest.raises(sj.SjpegError, match="sjpeg_hip_compose_ragged_src: " + words):
            rs.resample_images(devs, (10, 5), compose=comp, engine=engine)
        for packed in (False, True):
            with pytest.raises(sj.SjpegError, match="sjpeg_hip_encode_ragged_composed_%ssrc: " % ("packed_" if packed else "") + words):
                rs.encode_resampled_images(devs, sizes=(10, 5), compose=comp, packed=packed, engine=engine)
    import sjpeg_amd.unsharp as un
    with pytest.raises(sj.SjpegError, match="compose= and unsharp= are both given"):
        rs.encode_resampled_images(devs, sizes=(10, 5), compose=rs.Compose(), unsharp=un.Unsharp(16), engine=engine)
