"""tests/resample_box_model.py -- the definition of the box entries in numpy integers and Python doubles -- held to
Pillow: to tests/golden/resample_pillow_box.npz, what Image.reduce, Image.resize(box=, reducing_gap=), Image.thumbnail
and ImageOps.fit of Pillow 12.2.0 made of small pictures (always runs), and to an installed Pillow live on random cases
(skips only when PIL cannot be imported).  The library's host helpers -- the size rule, the crop, the plan's decision and
the box-taking table -- are held to the model, and so to Pillow; nothing here needs a device."""
import os

import numpy as np
import pytest

import resample_box_model as bm
import resample_model as rm
import sjpeg_amd as sj
import sjpeg_amd.resample as rs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_pillow_box.npz")
REDUCE, RESIZE_BOX, RESIZE_GAP, THUMBNAIL, FIT = range(5)
# a box for which the float32 and the double tables differ (the test below shows that they do)
F32_BOX = (0.1, 0.2, 30.7, 20.3)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _model_of(g, k):
    call, i, d, src = int(g["calls"][k]), [int(v) for v in g["ints"][k]], [float(v) for v in g["doubles"][k]], g["in_%d" % k]
    if call == REDUCE:
        return bm.reduce(src, i[0], i[1], tuple(int(v) for v in d[:4]))
    if call in (RESIZE_BOX, RESIZE_GAP):
        return bm.resize(src, (i[1], i[2]), i[0], tuple(d[:4]), d[4] or None)
    if call == THUMBNAIL:
        return bm.thumbnail(src, (d[0], d[1]), i[0], d[4] or None)
    return bm.fit(src, (i[1], i[2]), i[0], d[0], (d[1], d[2]))


def test_the_fixture_is_small_and_covers_the_five_calls(golden):
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "resample_pillow.npz"))
    calls = golden["calls"]
    assert set(calls) == {REDUCE, RESIZE_BOX, RESIZE_GAP, THUMBNAIL, FIT} and min(np.bincount(calls)) >= 6
    assert set(golden["ints"][calls != REDUCE][:, 0]) == set(rm.FILTERS)


def test_the_model_equals_what_pillow_recorded(golden):
    for k in range(len(golden["calls"])):
        assert np.array_equal(_model_of(golden, k), golden["out_%d" % k]), (k, golden["calls"][k], golden["ints"][k], golden["doubles"][k])


def test_pillows_reduce_is_not_the_half_up_average():
    """over every block size 1..64 and every sum: the two rules disagree on 14 535 of 530 464 pairs"""
    differ = pairs = 0
    for n in range(1, 65):
        S = np.arange(255 * n + 1, dtype=np.int64)
        pillow = ((S + n // 2) * bm.multiplier(n)) >> 24
        assert ((S + n // 2) * bm.multiplier(n)).max() < 2 ** 32 and pillow.max() == 255
        differ += int((pillow != (2 * S + n) // (2 * n)).sum())
        pairs += len(S)
    assert (pairs, differ) == (530464, 14535)
    # and for every block the entries take: the product stays inside a uint32
    for n in {a * b for a in (1, 2, 3, 127, 254, 255) for b in range(1, 256)}:
        assert (255 * n + n // 2) * bm.multiplier(n) < 2 ** 32, n


def test_the_float32_box_is_part_of_the_definition():
    """with doubles throughout the tables of this box differ: Pillow's C layer receives the box as float32"""
    differ = 0
    for f in rm.FILTERS:
        for (n_in, n_out, b0, b1) in ((40, 11, F32_BOX[0], F32_BOX[2]), (30, 9, F32_BOX[1], F32_BOX[3])):
            single, double = bm.box_table(f, n_in, n_out, b0, b1), bm.box_table(f, n_in, n_out, b0, b1, double=True)
            differ += int(not (np.array_equal(single[0], double[0]) and np.array_equal(single[1], double[1])))
            lb, lK = rs.resample_box_table(f, n_in, n_out, b0, b1)
            assert np.array_equal(lb, single[0]) and np.array_equal(lK, single[1]), (f, n_in, n_out)
    assert differ > 0


def test_the_whole_box_gives_the_parents_tables():
    for f in rm.FILTERS:
        for (n_in, n_out) in ((1, 1), (7, 3), (16, 24), (100, 7), (257, 3), (1920, 320)):
            want = rm.table(f, n_in, n_out)
            for got in (bm.box_table(f, n_in, n_out, 0, n_in), rs.resample_box_table(f, n_in, n_out, 0, n_in), rs.resample_table(f, n_in, n_out)):
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (f, n_in, n_out)


def test_the_librarys_tables_of_random_boxes_are_the_models():
    rng = np.random.default_rng(11)
    for _ in range(120):
        f, n_in, n_out = int(rng.integers(0, 5)), int(rng.integers(1, 70)), int(rng.integers(1, 40))
        b0 = float(rng.uniform(0, n_in - 0.5)) if rng.integers(0, 3) else 0.0
        b1 = float(rng.uniform(b0 + 0.25, n_in)) if rng.integers(0, 3) else float(n_in)
        want, got = bm.box_table(f, n_in, n_out, b0, b1), rs.resample_box_table(f, n_in, n_out, b0, b1)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (f, n_in, n_out, b0, b1)
        max_k, max_sum = rm.bound_sums(want[1])
        assert max_k < 2 ** 23 and max_sum < 2 ** 31
        # what the kernel relies on: windows in order and inside the axis
        xmin, n = want[0][:, 0].astype(int), want[0][:, 1].astype(int)
        assert (xmin >= 0).all() and (n >= 1).all() and (xmin + n <= n_in).all() and (np.diff(xmin) >= 0).all() and (np.diff(xmin + n) >= 0).all()


def test_the_decision_of_the_library_is_the_models():
    rng = np.random.default_rng(12)
    seen = set()
    for k in range(400):
        f, W, H = int(rng.integers(0, 5)), int(rng.integers(1, 300)), int(rng.integers(1, 300))
        w2, h2 = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        if k % 20 == 0:
            W, H = int(rng.integers(1, 3)), int(rng.integers(250, 300))      # (tall, unless the reduce makes it short)
        box = None
        if rng.integers(0, 2):
            l, t = float(rng.uniform(0, W - 0.5)), float(rng.uniform(0, H - 0.5))
            box = (l, t, float(rng.uniform(l + 0.25, W)), float(rng.uniform(t + 0.25, H)))
        gap = [None, 1.0, 2.0, 3.0, 1.37][int(rng.integers(0, 5))]
        try:
            (fx, fy), safe, size, inner = bm.decide(f, W, H, (w2, h2), box, gap)
        except bm.Refused as e:
            assert e.args[0] == "tall"
            with pytest.raises(sj.SjpegError, match="100 times as tall"):
                rs.box_decision(f, W, H, (w2, h2), box, gap)
            seen.add("tall")
            continue
        d = rs.box_decision(f, W, H, (w2, h2), box, gap)
        assert d["factor"] == (fx, fy) and d["safe_box"] == tuple(safe) and d["reduced_size"] == size and d["inner_box"] == tuple(inner)
        ex, ey = safe[2] - safe[0] - (size[0] - 1) * fx, safe[3] - safe[1] - (size[1] - 1) * fy
        assert d["multiplier"] == tuple(bm.multiplier(n) for n in (fx * fy, ex * fy, fx * ey, ex * ey))
        seen.add("reduced" if fx > 1 or fy > 1 else "plain")
        if safe[0] % fx or safe[1] % fy:
            seen.add("origin off the factor")
    assert seen == {"tall", "reduced", "plain", "origin off the factor"}


def test_the_named_refusals_of_the_decision():
    for box, gap, words in (((0, 0, 0, 5), None, "empty or leaves"), ((-0.5, 0, 5, 5), None, "empty or leaves"), ((0, 0, 40.5, 30), None, "empty or leaves"),
                            ((3, 3, 3, 9), None, "empty or leaves"), ((0, 0, float("nan"), 30), None, "empty or leaves"),
                            (None, 0.5, "reducing_gap"), (None, float("nan"), "reducing_gap")):
        with pytest.raises(sj.SjpegError, match=words):
            rs._lib()
            b = rs._BoxStruct((rs.C.c_double * 4)(*(box or (0, 0, 0, 0))), gap or 0.0)
            d = rs._DecisionStruct()
            if rs._lib().sjpeg_hip_resample_box_decide(3, 40, 30, 8, 6, rs.C.addressof(b), rs.C.addressof(d)) != 0:
                raise sj.SjpegError(rs._last_error())
    with pytest.raises(sj.SjpegError, match="above the cap of 255"):
        rs.box_decision(rm.BICUBIC, 60000, 8, (40, 4), None, 1.0)
    with pytest.raises(bm.Refused, match="factor"):
        bm.decide(rm.BICUBIC, 60000, 8, (40, 4), None, 1.0)
    # the limit the reduce lifts: 4000 -> 40 with Lanczos is a window of 601 samples, behind a factor of 50 one of 13
    assert rs.resample_ksize(rm.LANCZOS, 4000, 40) == 601 > rs.KSIZE_MAX
    d = rs.box_decision(rm.LANCZOS, 4000, 8, (40, 4), None, 2.0)
    assert d["factor"] == (50, 1) and d["reduced_size"] == (80, 8)
    assert rs.resample_box_table(rm.LANCZOS, 80, 40, d["inner_box"][0], d["inner_box"][2])[1].shape[1] == 13


def test_thumbnail_size_and_fit_crop_are_the_models():
    rng = np.random.default_rng(13)
    for _ in range(600):
        W, H = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        box = (float(rng.uniform(1, 300)), float(rng.uniform(1, 300))) if rng.integers(0, 2) else (int(rng.integers(1, 300)), int(rng.integers(1, 300)))
        assert rs.thumbnail_size(W, H, box) == bm.thumbnail_size(W, H, box), (W, H, box)
        size = (int(rng.integers(1, 200)), int(rng.integers(1, 200)))
        bleed, centering = float(rng.choice([0.0, 0.0, 0.1, 0.49, 0.5, -1.0])), (float(rng.uniform(-0.2, 1.2)), float(rng.uniform(-0.2, 1.2)))
        assert rs.fit_crop(W, H, size, bleed, centering) == bm.fit_crop(W, H, size, bleed, centering), (W, H, size, bleed, centering)
    for bad in ((0.5, 10), (10, 0), (float("nan"), 3)):
        with pytest.raises(sj.SjpegError, match="below 1x1"):
            rs.thumbnail_size(10, 10, bad)


def test_the_model_and_the_helpers_equal_an_installed_pillow_live():
    PIL = pytest.importorskip("PIL")
    from PIL import Image, ImageOps
    pil = {rm.BOX: Image.BOX, rm.BILINEAR: Image.BILINEAR, rm.HAMMING: Image.HAMMING, rm.BICUBIC: Image.BICUBIC, rm.LANCZOS: Image.LANCZOS}
    rng = np.random.default_rng(14)

    def picture(w, h):
        return rng.integers(0, 256, (h, w, 3) if rng.integers(0, 2) else (h, w), dtype=np.uint8)

    for _ in range(40):                                          # reduce: edge and corner blocks, random integer boxes
        w, h, fx, fy = int(rng.integers(1, 70)), int(rng.integers(1, 70)), int(rng.integers(1, 9)), int(rng.integers(1, 9))
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        box = (x0, y0, int(rng.integers(x0 + 1, w + 1)), int(rng.integers(y0 + 1, h + 1)))
        img = picture(w, h)
        assert np.array_equal(bm.reduce(img, fx, fy, box), np.asarray(Image.fromarray(img).reduce((fx, fy), box=box))), (w, h, fx, fy, box)
    for k in range(60):                                          # resize(box=, reducing_gap=)
        w, h, f = int(rng.integers(2, 90)), int(rng.integers(2, 90)), int(rng.integers(0, 5))
        w2, h2 = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        box = None
        if k % 3:
            l, t = float(rng.uniform(0, w - 1)), float(rng.uniform(0, h - 1))
            box = (l, t, float(rng.uniform(l + 0.5, w)), float(rng.uniform(t + 0.5, h)))
            if k % 3 == 2:
                box = tuple(float(round(v)) for v in box) if round(box[2]) > round(box[0]) and round(box[3]) > round(box[1]) else None
        gap = [None, 1.0, 2.0, 3.0][k % 4]
        img = picture(w, h)
        try:
            mine = bm.resize(img, (w2, h2), f, box, gap)
        except bm.Refused:
            continue
        want = np.asarray(Image.fromarray(img).resize((w2, h2), pil[f], box=box, reducing_gap=gap))
        assert np.array_equal(mine, want), (PIL.__version__, w, h, w2, h2, f, box, gap)
    for _ in range(30):                                          # thumbnail and fit, their size and crop rules included
        w, h, f = int(rng.integers(2, 120)), int(rng.integers(2, 120)), int(rng.integers(0, 5))
        img = picture(w, h)
        box = (float(rng.uniform(1, 40)), float(rng.uniform(1, 40)))
        im = Image.fromarray(img)
        im.thumbnail(box, pil[f])
        assert im.size == bm.thumbnail_size(w, h, box) == rs.thumbnail_size(w, h, box)
        try:
            assert np.array_equal(bm.thumbnail(img, box, f), np.asarray(im)), (w, h, box, f)
        except bm.Refused:
            pass
        size = (int(rng.integers(1, 30)), int(rng.integers(1, 30)))
        bleed, centering = float(rng.choice([0.0, 0.05, 0.2])), (float(rng.uniform(0, 1)), float(rng.uniform(0, 1)))
        try:
            mine = bm.fit(img, size, f, bleed, centering)
        except bm.Refused:
            continue
        assert np.array_equal(mine, np.asarray(ImageOps.fit(Image.fromarray(img), size, pil[f], bleed, centering))), (w, h, size, f, bleed, centering)
