"""tests/compose_model.py -- the definition of the compose stage in numpy integers and Python doubles -- against what
Pillow 12.2.0 recorded in tests/golden/compose_pillow.npz, and against the installed Pillow where there is one (the
blend over all 256^3 triples and the luma over all 256^3 colours, by whole images); the library's host helpers
(sjpeg_hip_compose_sample, sjpeg_hip_contain_size, sjpeg_hip_pad_place) against the model; and the words of every
refusal of the compose entries, through the C entries with a stand-in engine that no refused call reads.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import compose_cases as cc
import compose_model as cm
import sjpeg_amd as sj
import sjpeg_amd.resample as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "compose_pillow.npz"))
ENTRIES = ("sjpeg_hip_contain_size", "sjpeg_hip_pad_place", "sjpeg_hip_compose_sample", "sjpeg_hip_compose_ragged_bytes",
           "sjpeg_hip_compose_ragged_src", "sjpeg_hip_encode_ragged_composed_src", "sjpeg_hip_encode_ragged_composed_packed_src")
FAKE = 1 << 20                                   # the stand-in engine and buffers: never read by a refused call
EINVAL = -1                                      # SJPEG_HIP_EINVAL


@pytest.fixture(scope="module", autouse=True)
def the_entries_are_exported():
    """everything below is about these entries: the library declares and exports them"""
    header = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    for name in ENTRIES:
        assert name in sj.EXPORTED_C_SYMBOLS and hasattr(rs._lib(), name) and name + "(" in header, name


def _pillow():
    PIL = pytest.importorskip("PIL")
    if PIL.__version__ != "12.2.0":
        pytest.skip("the definition is Pillow 12.2.0's")
    from PIL import Image, ImageOps
    return Image, ImageOps


# ---- the model against the fixture

def test_the_cases_cover_what_they_must():
    assert cc.SIZES[:4] == [(3, 2, (5, 5), (0.5, 0.5)), (2, 3, (6, 5), (0.5, 0.5)), (5, 5, (6, 1), (0.5, 0.5)), (1920, 1080, (256, 256), (0.5, 0.5))]
    ratios = [np.sign(w / h - bw / bh) for w, h, (bw, bh), _ in cc.SIZES]
    assert {-1.0, 0.0, 1.0} == set(ratios)
    assert any(not 0 <= c <= 1 for *_, cen in cc.SIZES for c in cen)
    assert cc.PASTES[0][2] == cc.PASTES[1][2][::-1] and {m for m, *_ in cc.PASTES} == {"RGB", "L"}
    outside = [p for _, (w, h), ps in cc.PASTES for o, p in ps if p[0] >= w or p[1] >= h or p[0] <= -20]
    assert len(outside) == 2
    assert cc.CHAIN_SOURCES == [(90, 50), (50, 90)] and cc.CHAIN_BOX == (40, 40)
    assert cc.logo()[..., 3].min() == 0 and cc.logo()[..., 3].max() == 255


def test_the_models_sizes_and_places_are_the_recorded_ones():
    for (w, h, box, centering), rec in zip(cc.SIZES, GOLDEN["sizes"].tolist()):
        size = cm.contain_size(w, h, box)
        assert size == tuple(rec[:2]) and cm.pad_place(*size, box, centering) == tuple(rec[2:]), (w, h, box, centering)
    # the observed values, half to even
    assert (cm.contain_size(3, 2, (5, 5)), cm.pad_place(5, 3, (5, 5))) == ((5, 3), (0, 1))
    assert (cm.contain_size(2, 3, (6, 5)), cm.pad_place(3, 5, (6, 5))) == ((3, 5), (2, 0))
    assert (cm.contain_size(5, 5, (6, 1)), cm.pad_place(1, 1, (6, 1))) == ((1, 1), (2, 0))
    assert (cm.contain_size(1920, 1080, (256, 256)), cm.pad_place(256, 144, (256, 256))) == ((256, 144), (0, 56))
    for w, h, box in cc.SIZES_REFUSED:
        assert 0 in cm.contain_size(w, h, box)


@pytest.mark.parametrize("k", range(len(cc.PASTES)))
def test_the_model_makes_the_recorded_pastes(k):
    mode, size, pastes = cc.PASTES[k]
    out = cc.base(mode, size, k)
    for o, at in pastes:
        out = cm.paste(out, cc.overlay(o), at)
    assert np.array_equal(out, GOLDEN["paste_%d" % k])


def test_the_order_of_two_overlays_matters():
    assert not np.array_equal(GOLDEN["paste_0"], GOLDEN["paste_1"])
    assert cm.blend(cm.blend(0, 255, 128), 0, 128) == 64 and cm.blend(cm.blend(0, 0, 128), 255, 128) == 128
    # an overlay wholly outside leaves the picture
    assert np.array_equal(GOLDEN["paste_6"], cc.base("RGB", (12, 10), 6)) and np.array_equal(GOLDEN["paste_7"], cc.base("RGB", (12, 10), 7))


def test_the_blend_is_the_division_and_not_two_rounded_products():
    a, d, s = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij", sparse=True)
    got = cm.blend(d, s, a)
    assert np.array_equal(got, (d * (255 - a) + s * a + 127) // 255)
    mul = lambda x, y: (((x * y + 128) >> 8) + x * y + 128) >> 8
    assert 4_000_000 < int((got != mul(d, 255 - a) + mul(s, a)).sum()) < 4_300_000
    assert np.array_equal(got[0], np.broadcast_to(d[0], (256, 256))) and np.array_equal(got[255], np.broadcast_to(s[0], (256, 256)))


@pytest.mark.parametrize("k", range(2))
def test_the_model_makes_the_recorded_chain(k):
    want = cm.compose(GOLDEN["chain_%d_sharp" % k], cc.CHAIN_BOX, colour=cc.CHAIN_COLOUR, overlays=[(cc.logo(), cc.CHAIN_LOGO_AT, "top-left")])
    assert np.array_equal(want, GOLDEN["chain_%d" % k])
    assert np.array_equal(cm.compose(GOLDEN["chain_%d_sharp" % k], cc.CHAIN_BOX, colour=cc.CHAIN_COLOUR), GOLDEN["chain_%d_pad" % k])
    import pillow_filter_model as pm
    import resample_box_model as bm
    assert np.array_equal(bm.thumbnail(cc.chain_source(k), cc.CHAIN_BOX), GOLDEN["chain_%d_thumbnail" % k])
    assert np.array_equal(pm.unsharp_mask(GOLDEN["chain_%d_thumbnail" % k], 2, 150, 3), GOLDEN["chain_%d_sharp" % k])


@pytest.mark.parametrize("k", range(len(cc.PADS)))
def test_the_model_makes_the_recorded_pads(k):
    import resample_box_model as bm
    import resample_model as rm
    mode, size, box, colour, centering = cc.PADS[k]
    img = cc.base(mode, size, 50 + k)
    made = bm.resize(img, cm.contain_size(size[0], size[1], box), rm.BICUBIC, None, None)
    assert np.array_equal(cm.compose(made, box, centering=centering, colour=colour), GOLDEN["pad_%d" % k])


def test_the_anchors():
    for anchor, want in (("top-left", (1, 2)), ("top-right", (5, 2)), ("bottom-left", (1, 4)), ("bottom-right", (5, 4)), ("centre", (4, 5))):
        assert cm.anchor_place(anchor, (10, 8), (4, 2), (1, 2)) == want
    assert cm.anchor_place("centre", (4, 3), (7, 8), (0, 0)) == (-2, -3)


# ---- live, where Pillow 12.2.0 is installed: whole images, a second or two each

def test_live_the_blend_over_all_triples():
    Image, _ = _pillow()
    for a in range(256):
        d, s = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
        base = Image.fromarray(d)
        over = Image.fromarray(np.ascontiguousarray(np.stack([s, s, s, np.full_like(s, a)], axis=2)), "RGBA")
        rgb = Image.merge("RGB", [base] * 3)
        rgb.paste(over, (0, 0), over)
        assert np.array_equal(np.asarray(rgb)[..., 1], cm.blend(d, s, a)), a
        if a % 16 == 0:
            comp = Image.alpha_composite(Image.merge("RGBA", [base] * 3 + [Image.new("L", (256, 256), 255)]), over)
            assert np.array_equal(np.asarray(comp)[..., 2], cm.blend(d, s, a)), a


def test_live_the_luma_over_all_colours():
    Image, _ = _pillow()
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for r in range(256):
        rgb = np.ascontiguousarray(np.stack([np.full_like(g, r), g, b], axis=2))
        assert np.array_equal(np.asarray(Image.fromarray(rgb).convert("L")), cm.luma(r, g, b)), r
    # ... and a gray base is blended with it
    base = cc.base("L", (12, 10), 8)
    im, logo = Image.fromarray(base), Image.fromarray(cc.overlay(2), "RGBA")
    im.paste(logo, (1, 1), logo)
    assert np.array_equal(np.asarray(im), cm.paste(base, cc.overlay(2), (1, 1))) and np.array_equal(np.asarray(im), GOLDEN["paste_8"])


def test_live_the_sizes_the_places_and_the_pads():
    Image, ImageOps = _pillow()
    for (w, h, box, centering), rec in zip(cc.SIZES, GOLDEN["sizes"].tolist()):
        assert ImageOps.contain(Image.new("L", (w, h)), box).size == tuple(rec[:2])
    for w, h, box in cc.SIZES_REFUSED:
        with pytest.raises(ValueError):
            ImageOps.contain(Image.new("L", (w, h)), box)
    for k, (mode, size, box, colour, centering) in enumerate(cc.PADS):
        im = Image.fromarray(cc.base(mode, size, 50 + k))
        got = ImageOps.pad(im, box, Image.Resampling.BICUBIC, color=colour if mode == "RGB" else colour[0], centering=centering)
        assert np.array_equal(np.asarray(got), GOLDEN["pad_%d" % k])


# ---- the library's host helpers against the model

def test_the_librarys_sample_is_the_models():
    rng = np.random.RandomState(5)
    for d, r, g, b, a in rng.randint(0, 256, (4000, 5)).tolist() + [[0, 255, 0, 0, 128], [128, 0, 0, 0, 128], [7, 9, 9, 9, 0], [7, 9, 200, 3, 255]]:
        assert rs.compose_sample(d, r, a) == int(cm.blend(d, r, a))
        assert rs.compose_sample(d, (r, g, b), a, gray=True) == int(cm.blend(d, cm.luma(r, g, b), a))


def test_the_librarys_sizes_and_places_are_the_models():
    rng = np.random.RandomState(6)
    cases = [(w, h, box, cen) for w, h, box, cen in cc.SIZES]
    cases += [(int(w), int(h), (int(bw), int(bh)), (float(cx), float(cy))) for w, h, bw, bh, cx, cy in
              np.column_stack([rng.randint(1, 700, (3000, 4)), rng.uniform(-0.5, 1.5, (3000, 2))]).tolist()]
    for w, h, box, cen in cases:
        size = cm.contain_size(w, h, box)
        if 0 in size:
            with pytest.raises(sj.SjpegError, match="has a side of 0 \\(Pillow raises\\)"):
                rs.contain_size(w, h, box)
            continue
        assert rs.contain_size(w, h, box) == size and rs.pad_place(size[0], size[1], box, cen) == cm.pad_place(size[0], size[1], box, cen), (w, h, box, cen)
    with pytest.raises(sj.SjpegError, match="sjpeg_hip_contain_size: a 1000x1 picture contained in 10x10 has a side of 0"):
        rs.contain_size(1000, 1, (10, 10))
    with pytest.raises(sj.SjpegError, match="sjpeg_hip_pad_place: the 6x1 picture is not wholly inside the 5x5 canvas"):
        rs.pad_place(6, 1, (5, 5))
    with pytest.raises(sj.SjpegError, match="sjpeg_hip_pad_place: the centering is not finite"):
        rs.pad_place(1, 1, (5, 5), (float("inf"), 0))


def test_the_structs_have_the_sizes_the_header_states():
    assert (C.sizeof(rs._OverlayStruct), C.sizeof(rs._PlaceStruct), C.sizeof(rs._ComposeStruct)) == (24, 16, 48)
    assert rs._ComposeStruct.cx.offset == 24 and rs._ComposeStruct.first_place.offset == 40
    header = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    for words in ("} sjpeg_hip_overlay;              /* 24 bytes */", "} sjpeg_hip_overlay_place;        /* 16 bytes */",
                  "} sjpeg_hip_compose;              /* 48 bytes */"):
        assert words in header


# ---- the refusals, through the C entries: every one is SJPEG_HIP_EINVAL before the engine is read

N = 3
DIMS = [(20, 10), (9, 7), (6, 6)]


def _call(entry, compose, per_frame, overlays=(), places=(), fmt=None, nplaces=None, noverlays=None, filt=None):
    """(return code, sjpeg_hip_last_error()) of one C call over three RGB frames at their own sizes"""
    L = rs._lib()
    fmt = sj.SRC_RGB if fmt is None else fmt
    frames, _, _, _ = sj._ragged_frames([[(4096 * (k + 1), 64)] for k in range(N)], DIMS, None, None, None, None)
    for k in range(N):
        frames[k].out_offset, frames[k].out_capacity = 65536 * k, 65536
    resample, box = (rs._ResampleStruct * 1)(rs._ResampleStruct(3)), (rs._BoxStruct * 1)()
    carr = None if compose is None else (rs._ComposeStruct * len(compose))(*compose)
    oarr = (rs._OverlayStruct * max(len(overlays), 1))(*overlays)
    parr = (rs._PlaceStruct * max(len(places), 1))(*places)
    farr = None if filt is None else (rs._FilterStruct * 1)(filt)
    six = (None if carr is None else C.addressof(carr), per_frame, C.addressof(oarr) if overlays else None, len(overlays) if noverlays is None else noverlays,
           C.addressof(parr) if places else None, len(places) if nplaces is None else nplaces)
    shape = (None, None, None, C.addressof(resample), 0, C.addressof(box), 0, None if farr is None else C.addressof(farr), 0)
    if entry == "sjpeg_hip_compose_ragged_src":
        made, rfmt = (sj.RaggedFrame * N)(), C.c_int(-1)
        rc = L.sjpeg_hip_compose_ragged_src(FAKE, fmt, N, frames, *shape, *six, FAKE, 1 << 30, made, C.byref(rfmt), None)
    else:
        call = sj.Engine._full_call(None, "t", N, DIMS, sj.YUV_444, sj._quality_quant([75.0] * N), 4, None, 0x78, 12, 1, None, [65536] * N, None)
        tail = (FAKE, 1 << 30, FAKE, FAKE) if entry.endswith("packed_src") else (FAKE, FAKE)
        rc = getattr(L, entry)(FAKE, fmt, N, frames, call.params, *shape, *six, *call.meta, *tail, *call.results, None)
    return rc, (L.sjpeg_hip_last_error() or b"").decode()


def _c(cw=0, ch=0, mode=0, px=0, py=0, cx=0.0, cy=0.0, first=0, n=0, reserved=0):
    c = rs._ComposeStruct()
    c.canvas_width, c.canvas_height, c.mode, c.px, c.py, c.cx, c.cy, c.first_place, c.nplaces = cw, ch, mode, px, py, cx, cy, first, n
    c.reserved[2] = reserved
    return c


def _o(rgba=4096, w=4, h=3, stride=16):
    return rs._OverlayStruct(rgba, w, h, stride)


def _p(overlay=0, x=0, y=0, anchor=0, reserved=0):
    p = rs._PlaceStruct(overlay, x, y, anchor)
    p.reserved[0] = reserved
    return p


REFUSALS = [
    ("a canvas side of 0", dict(compose=[_c(0, 5)], per_frame=0), "compose: canvas 0x5 is not 0x0 \\(the picture's own size\\) or 1..65535 a side"),
    ("a canvas side above 65535", dict(compose=[_c(), _c(30, 65536), _c()], per_frame=1), "frame 1: compose: canvas 30x65536 is not 0x0"),
    ("a picture that leaves its canvas", dict(compose=[_c(), _c(), _c(8, 8, px=3)], per_frame=1),
     "frame 2: compose: the 6x6 picture at \\(3, 0\\) is not wholly inside the 8x8 canvas"),
    ("a picture larger than the canvas of the call", dict(compose=[_c(19, 19, mode=1, cx=0.5, cy=0.5)], per_frame=0),
     "frame 0: compose: the 20x10 picture is not wholly inside the 19x19 canvas"),
    ("a negative place of the picture", dict(compose=[_c(40, 40, px=-1)], per_frame=0), "frame 0: compose: the 20x10 picture at \\(-1, 0\\) is not wholly inside"),
    ("a centering that is not finite", dict(compose=[_c(40, 40, mode=1, cx=float("nan"), cy=0.5)], per_frame=0), "compose: the centering is not finite"),
    ("... along y", dict(compose=[_c(), _c(40, 40, mode=1, cx=0.5, cy=float("inf")), _c()], per_frame=1), "frame 1: compose: the centering is not finite"),
    ("an unknown placement mode", dict(compose=[_c(40, 40, mode=2)], per_frame=0), "compose: mode 2 is not 0 \\(at px, py\\) or 1 \\(by the centering\\)"),
    ("an unknown anchor", dict(compose=[_c(n=2)], per_frame=0, overlays=[_o()], places=[_p(), _p(anchor=5)]),
     "place 1: anchor 5 is not one of 0..4 \\(top-left, top-right, bottom-left, bottom-right, centre\\)"),
    ("places beyond the call's", dict(compose=[_c(), _c(first=1, n=2), _c()], per_frame=1, overlays=[_o()], places=[_p(), _p()]),
     "frame 1: compose: places 1 .. 3 are not within the call's 2 places"),
    ("a negative first place", dict(compose=[_c(first=-1, n=1)], per_frame=0, overlays=[_o()], places=[_p()]), "compose: places -1 .. 0 are not within the call's 1 places"),
    ("more than 8 places", dict(compose=[_c(n=9)], per_frame=0, overlays=[_o()], places=[_p()] * 9), "compose: 9 places are more than 8"),
    ("an overlay index out of range", dict(compose=[_c(n=1)], per_frame=0, overlays=[_o()], places=[_p(overlay=1)]),
     "place 0: overlay 1 is not one of the call's 1 overlays"),
    ("a negative overlay index", dict(compose=[_c(n=1)], per_frame=0, overlays=[_o()], places=[_p(overlay=-1)]), "place 0: overlay -1 is not one of"),
    ("an overlay without pixels", dict(compose=[_c(n=1)], per_frame=0, overlays=[_o(), _o(rgba=None)], places=[_p()]), "overlay 1: rgba == NULL"),
    ("an overlay that is no multiple of 4", dict(compose=[_c(n=1)], per_frame=0, overlays=[_o(rgba=4098)], places=[_p()]), "overlay 0: rgba must be a multiple of 4"),
    ("an overlay side of 0", dict(compose=[_c(n=1)], per_frame=0, overlays=[_o(w=0)], places=[_p()]), "overlay 0: width 0 or height 3 is not one of 1..65535"),
    ("an overlay side above 65535", dict(compose=[_c(n=1)], per_frame=0, overlays=[_o(h=65536, stride=16)], places=[_p()]), "overlay 0: width 4 or height 65536 is not"),
    ("an overlay stride below its row", dict(compose=[_c(n=1)], per_frame=0, overlays=[_o(stride=12)], places=[_p()]),
     "overlay 0: stride 12 is below 4 \\* width or not a multiple of 4"),
    ("an overlay stride that is no multiple of 4", dict(compose=[_c(n=1)], per_frame=0, overlays=[_o(stride=18)], places=[_p()]), "overlay 0: stride 18 is below"),
    ("overlays missing", dict(compose=[_c(n=1)], per_frame=0, overlays=[], places=[_p()], noverlays=1), "overlays == NULL or noverlays is negative"),
    ("places missing", dict(compose=[_c(n=1)], per_frame=0, overlays=[_o()], places=[], nplaces=1), "places == NULL or nplaces is negative"),
    ("a reserved byte of the compose", dict(compose=[_c(), _c(), _c(reserved=1)], per_frame=1), "frame 2: compose: reserved must be 0"),
    ("a reserved byte of a place", dict(compose=[_c(n=1)], per_frame=0, overlays=[_o()], places=[_p(reserved=9)]), "place 0: reserved must be 0"),
    ("what the filtered entries refuse: a filter", dict(compose=[_c(40, 40)], per_frame=0, filt=rs._FilterStruct(1, 0, 0, 64.0, 1.0)),
     "filter: radius_x gives a box radius above 63"),
]


@pytest.mark.parametrize("entry", ENTRIES[4:])
@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_the_refusals_by_their_words(entry, k):
    import re
    label, kw, words = REFUSALS[k]
    rc, text = _call(entry, **kw)
    assert rc == EINVAL, (label, rc, text)
    assert re.match(re.escape(entry) + ": " + words, text), (label, text)


def test_made_pictures_that_are_neither_rgb_nor_gray_are_refused():
    L = rs._lib()
    frames = (sj.RaggedFrame * 1)()
    frames[0].width, frames[0].height = 16, 8
    for c, (w, h) in enumerate(((16, 8), (8, 4), (8, 4))):
        frames[0].plane[c], frames[0].row_stride[c] = 4096 * (c + 1), 16
    resample, box, comp = (rs._ResampleStruct * 1)(rs._ResampleStruct(3)), (rs._BoxStruct * 1)(), (rs._ComposeStruct * 1)(_c(40, 40))
    made, rfmt = (sj.RaggedFrame * 1)(), C.c_int(-1)
    rc = L.sjpeg_hip_compose_ragged_src(FAKE, sj.SRC_YUV420, 1, frames, None, None, None, C.addressof(resample), 0, C.addressof(box), 0, None, 0,
                                        C.addressof(comp), 0, None, 0, None, 0, FAKE, 1 << 30, made, C.byref(rfmt), None)
    text = L.sjpeg_hip_last_error().decode()
    # (the resample plan refuses YUV planes by name before the compose plan could: everything the _filtered_ entries refuse)
    assert rc == EINVAL and text.startswith("sjpeg_hip_compose_ragged_src: ") and ("YUV" in text or "are not composed" in text), text


@pytest.mark.parametrize("entry,under", [("sjpeg_hip_compose_ragged_src", "sjpeg_hip_resample_box_ragged_src"),
                                         ("sjpeg_hip_encode_ragged_composed_src", "sjpeg_hip_encode_ragged_resampled_box_src"),
                                         ("sjpeg_hip_encode_ragged_composed_packed_src", "sjpeg_hip_encode_ragged_resampled_box_packed_src")])
def test_the_identity_route_speaks_under_the_other_entrys_name(entry, under):
    """compose NULL, a canvas of 0 x 0 and a canvas of the picture's own size are the _filtered_ entry -- which, without
    a filter, is the _resampled_box_ entry: its messages, under its name"""
    own = [_c(w, h) for w, h in DIMS]
    for compose, per in ((None, 0), ([_c()], 0), ([_c()] * 3, 1), ([_c(mode=1, cx=0.5, cy=0.5)], 0)):
        rc, text = _call(entry, compose, per, fmt=99)
        assert rc != 0 and text == under + ": unknown source format", (compose, text)
    rc, text = _call(entry, own, 1, filt=rs._FilterStruct(1, 0, 0, 64.0, 1.0))
    assert rc != 0 and text.startswith(under.replace("resample_box_ragged", "filter_ragged").replace("resampled_box", "filtered") + ": filter: radius_x"), text
    # ... and one canvas that is not the picture's size is the compose entry
    rc, text = _call(entry, [_c(20, 10), _c(9, 7), _c(6, 7)], 1, fmt=99)
    assert rc != 0 and text == entry + ": unknown source format", text
