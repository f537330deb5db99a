"""tests/pillow_filter_model.py -- the definition of the _filtered_ entries in numpy integers and float32 scalars --
against what Pillow 12.2.0 recorded in tests/golden/pillow_filter.npz, and against the installed Pillow where there is
one; the library's host arithmetic (sjpeg_hip_pillow_filter_weights, resample.PillowFilter) against the model.  The
three traps each have a test: the weight divided in float32, the radius formula rounded operation by operation, the
strict threshold.  No GPU."""
import os

import numpy as np
import pytest

import pillow_filter_cases as pc
import pillow_filter_model as pm
import sjpeg_amd as sj
import sjpeg_amd.resample as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "pillow_filter.npz"))

ENTRIES = ("sjpeg_hip_pillow_filter_weights", "sjpeg_hip_filter_ragged_src", "sjpeg_hip_encode_ragged_filtered_src",
           "sjpeg_hip_encode_ragged_filtered_packed_src")


@pytest.fixture(scope="module", autouse=True)
def the_entries_are_exported():
    """everything below is about these entries: the library declares and exports them"""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sjpeg_hip.h")).read()
    for name in ENTRIES:
        assert name in sj.EXPORTED_C_SYMBOLS and hasattr(rs._lib(), name) and name + "(" in header, name


def _pillow():
    PIL = pytest.importorskip("PIL")
    if PIL.__version__ != "12.2.0":
        pytest.skip("the definition is Pillow 12.2.0's")
    from PIL import Image, ImageFilter
    return Image, ImageFilter


def _pil_filter(ImageFilter, spec):
    return {"box": ImageFilter.BoxBlur, "gaussian": ImageFilter.GaussianBlur, "unsharp": ImageFilter.UnsharpMask}[spec[0]](*spec[1:])


def test_the_cases_cover_what_they_must():
    modes, sizes = {c[0] for c in pc.CASES}, {c[1] for c in pc.CASES}
    assert modes == {"L", "RGB"} and sizes == {(1, 1), (2, 3), (5, 7), (17, 9), (97, 33)}
    specs = {c[2] for c in pc.CASES}
    for r in (0.3, 2.7, 0.5, 1, 5, 63.9, (0, 2), (3, 0)):
        assert ("box", r) in specs
    assert ("L", (5, 7), ("box", 5)) in pc.CASES and ("L", (17, 9), ("box", 63.9)) in pc.CASES
    for s in (1, 2, 3.3, (1.5, 4), (0, 3), 0):
        assert ("gaussian", s) in specs
    for u in ((2, 150, 3), (1, 80, 0), (0.6, 500, 1), (2, 150, 255), (0, 150, 0)):
        assert ("unsharp",) + u in specs
    assert pm.axis_weights(pm.GAUSSIAN, 1)[0] == 0 and pm.axis_weights(pm.GAUSSIAN, 1)[3] == 3


@pytest.mark.parametrize("k", range(len(pc.CASES)))
def test_the_model_makes_the_recorded_bytes(k):
    mode, size, spec = pc.CASES[k]
    img, want = pc.picture(mode, size, k), GOLDEN["out_%d" % k]
    assert want.shape == img.shape
    assert np.array_equal(pm.apply(img, spec), want), (mode, size, spec)


def test_the_unsharp_cases_clip_both_ways_and_truncate_toward_zero():
    k = pc.CASES.index(("L", (97, 33), ("unsharp", 0.6, 500, 1)))
    img, want = pc.picture("L", (97, 33), k), GOLDEN["out_%d" % k]
    d = img.astype(np.int64) - pm.gaussian_blur(img, 0.6).astype(np.int64)
    raw = img + np.sign(d) * (np.abs(d) * 500 // 100)
    assert (raw < 0).any() and (raw > 255).any() and int(want.min()) == 0 and int(want.max()) == 255
    # a negative difference whose product is no multiple of 100: floor division would give one less
    k = pc.CASES.index(("L", (17, 9), ("unsharp", 1, 80, 0)))
    img, want = pc.picture("L", (17, 9), k), GOLDEN["out_%d" % k]
    d = img.astype(np.int64) - pm.gaussian_blur(img, 1).astype(np.int64)
    floored = np.clip(img + (d * 80) // 100, 0, 255)
    assert ((d < 0) & ((d * 80) % 100 != 0)).any() and not np.array_equal(floored, want)
    # threshold 255 and sigma 0: the picture itself
    for spec in (("unsharp", 2, 150, 255), ("unsharp", 0, 150, 0)):
        k = [c[2] for c in pc.CASES].index(spec)
        assert np.array_equal(GOLDEN["out_%d" % k], pc.picture(pc.CASES[k][0], pc.CASES[k][1], k))


def test_trap_1_the_weight_is_divided_in_float32():
    """2^24 / (2 fr + 1) in double gives another ww for 0.3 and 2.7, and other bytes"""
    for fr in (0.3, 2.7):
        r, ww, fw = pm.box_weights(fr)
        ww64 = int(16777216.0 / (float(np.float32(fr)) * 2.0 + 1.0))
        assert ww64 != ww, fr
        k = pc.CASES.index(("L", (97, 33), ("box", fr)))
        img = pc.picture("L", (97, 33), k)
        wrong = pm.box_pass(pm.box_pass(img, 1, r, ww64, ((1 << 24) - (2 * r + 1) * ww64) // 2), 0, r, ww64, ((1 << 24) - (2 * r + 1) * ww64) // 2)
        assert not np.array_equal(wrong, GOLDEN["out_%d" % k])
        assert np.array_equal(pm.box_blur(img, fr), GOLDEN["out_%d" % k])


def test_trap_2_the_radius_is_rounded_operation_by_operation():
    """the worked values, and a sigma whose radius -- and weights -- differ where the formula runs in doubles"""
    assert float(pm.gaussian_radius(2)) == 1.375
    assert abs(float(pm.gaussian_radius(1)) - 0.25) < 1e-7 and abs(float(pm.gaussian_radius(63)) - 62.496) < 1e-3
    differ = [s for s in np.arange(0.5, 20.0, 0.0137) if pm.box_weights(pm.gaussian_radius(s)) != pm.box_weights(np.float32(pm.gaussian_radius_double(np.float32(s))))]
    assert differ, "no sigma whose weights differ"
    s = float(differ[0])
    assert sj_weights(pm.GAUSSIAN, s)[:3] == pm.box_weights(pm.gaussian_radius(s))
    assert sj_weights(pm.GAUSSIAN, s)[:3] != pm.box_weights(np.float32(pm.gaussian_radius_double(np.float32(s))))


def test_trap_3_the_threshold_is_strict():
    img, thr = pc.trap3_picture(), pc.trap3_threshold()
    assert thr == int(GOLDEN["trap3"][0]) and thr > 0
    want = GOLDEN["trap3_out"]
    assert np.array_equal(pm.unsharp_mask(img, pc.TRAP3_RADIUS, 150, thr), want)
    assert want[4, 4] == img[4, 4]                                  # a difference EQUAL to the threshold: unchanged
    assert pm.unsharp_mask(img, pc.TRAP3_RADIUS, 150, thr - 1)[4, 4] != img[4, 4]


def sj_weights(kind, radius):
    return rs.pillow_filter_weights(kind, radius)


def test_the_librarys_weights_are_the_models():
    for kind in (pm.BOX, pm.GAUSSIAN, pm.UNSHARP):
        for radius in list(np.arange(0.0, 63.9, 0.173)) + [0.3, 2.7, 0.5, 1, 5, 63.9, 1e-4, 63.99]:
            if kind != pm.BOX and radius > 63.9:
                continue
            assert sj_weights(kind, radius) == pm.axis_weights(pm.BOX if kind == pm.BOX else pm.GAUSSIAN, radius), (kind, radius)
    assert sj_weights(pm.BOX, 0) == (0, 1 << 24, 0, 0) and sj_weights(pm.GAUSSIAN, 0)[3] == 0


def test_the_librarys_refusals_of_an_axis():
    for kind, radius, words in ((pm.BOX, 64, "box radius above 63"), (pm.GAUSSIAN, 70, "box radius above 63"), (pm.BOX, -1, "finite number of 0 or more"),
                                (pm.BOX, float("nan"), "finite"), (pm.GAUSSIAN, float("inf"), "finite"), (0, 1, "kind 0"), (4, 1, "kind 4"),
                                # (sigmas whose radius formula cancels or overflows in float32: refused, not skipped)
                                (pm.GAUSSIAN, 1.4e15, "box radius above 63"), (pm.UNSHARP, 1e16, "box radius above 63"),
                                (pm.GAUSSIAN, 3e38, "box radius above 63")):
        with pytest.raises(sj.SjpegError, match=words):
            sj_weights(kind, radius)


def test_the_python_filters_and_their_refusals():
    u = rs.PillowFilter.unsharp_mask()
    assert (u.kind, u.radius, u.percent, u.threshold) == (3, (2.0, 2.0), 150, 3)
    assert rs.PillowFilter.gaussian_blur((1.5, 4)).radius == (1.5, 4.0) and rs.PillowFilter.box_blur(3).kind == 1
    assert rs.PillowFilter.gaussian_blur().radius == (2.0, 2.0) and rs.PillowFilter.none().kind == 0
    with pytest.raises(sj.SjpegError, match="one radius"):
        rs.PillowFilter.unsharp_mask((1, 2))
    with pytest.raises(sj.SjpegError, match="percent"):
        rs.PillowFilter.unsharp_mask(2, 70000)
    with pytest.raises(sj.SjpegError, match="threshold"):
        rs.PillowFilter.unsharp_mask(2, 150, 256)
    with pytest.raises(sj.SjpegError, match="pair"):
        rs.PillowFilter.box_blur("wide")
    import sjpeg_amd.unsharp as un
    with pytest.raises(sj.SjpegError, match=r"post= and unsharp="):
        rs._post_args("encode_thumbnails", 2, u, un.Unsharp(16))
    with pytest.raises(sj.SjpegError, match="one .* per frame"):
        rs._post_args("resample_images", 3, [u, None])
    keep, addr, per = rs._post_args("resample_images", 2, [u, None])
    assert per == 1 and keep[1].kind == 0 and keep[0].kind == 3 and C_sizeof(keep[0]) == 16


def C_sizeof(s):
    import ctypes
    return ctypes.sizeof(s)


# ---- live, where Pillow 12.2.0 is installed

def test_live_the_cases_and_the_chain():
    Image, ImageFilter = _pillow()
    for k, (mode, size, spec) in enumerate(pc.CASES):
        img = pc.picture(mode, size, k)
        got = np.asarray(Image.fromarray(img).filter(_pil_filter(ImageFilter, spec)))
        assert np.array_equal(got, GOLDEN["out_%d" % k]) and np.array_equal(pm.apply(img, spec), got), (mode, size, spec)
    im = Image.fromarray(pc.chain_picture())
    im.thumbnail(pc.CHAIN_BOX)
    assert np.array_equal(np.asarray(im), GOLDEN["chain_thumbnail"])
    assert np.array_equal(np.asarray(im.filter(ImageFilter.UnsharpMask(2, 150, 3))), GOLDEN["chain"])
    assert np.array_equal(pm.unsharp_mask(GOLDEN["chain_thumbnail"], 2, 150, 3), GOLDEN["chain"])


def test_live_a_sweep_of_sigmas_against_pillow():
    """the radius formula: a row of noise blurred along x alone, for sigmas from 0 to 64"""
    Image, ImageFilter = _pillow()
    img = pc.picture("L", (160, 2), 99)
    im = Image.fromarray(img)
    for s in np.arange(0.0, 64.0, 0.0411):
        s = float(s)
        want = np.asarray(im.filter(ImageFilter.GaussianBlur((s, 0))))
        assert np.array_equal(pm.gaussian_blur(img, (s, 0)), want), s
