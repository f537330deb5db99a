"""tests/resample_model.py -- the definition of the resampling entries in numpy integers and Python doubles -- held to
Pillow: to tests/golden/resample_pillow.npz, what Image.resize of Pillow 12.2.0 made of small pictures with the five
filters (always runs: it pins the definition where Pillow is not installed), and to an installed Pillow live on a grid of
sizes (skips only when PIL cannot be imported).  The library's host entry for the tables is held to the model too."""
import os

import numpy as np
import pytest

import resample_model as rm
import sjpeg_amd.resample as rs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_pillow.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_fixture_is_small_and_covers_the_filters(golden):
    assert os.path.getsize(GOLDEN) < 200 * 1024
    cases = golden["cases"]
    assert len(cases) >= 60 and set(cases[:, 0]) == set(rm.FILTERS) and set(cases[:, 6]) == {0, 1, 2} and set(cases[:, 3]) == {1, 3}
    w, h, w2, h2 = cases[:, 1], cases[:, 2], cases[:, 4], cases[:, 5]
    # shrinking, enlarging, each axis alone, neither, one up and one down, 1 x 1 sources and results
    assert (w2 < w).any() and (w2 > w).any() and ((w2 == w) & (h2 != h)).any() and ((h2 == h) & (w2 != w)).any()
    assert ((w2 == w) & (h2 == h)).any() and ((w2 > w) & (h2 < h)).any() and ((w == 1) & (h == 1)).any() and ((w2 == 1) & (h2 == 1)).any()


def test_the_model_equals_what_pillow_recorded(golden):
    for k, (filt, w, h, c, w2, h2, kind) in enumerate(golden["cases"]):
        src, want = golden["in_%d" % k], golden["out_%d" % k]
        assert src.shape == ((h, w) if c == 1 else (h, w, c)) and want.shape == ((h2, w2) if c == 1 else (h2, w2, c))
        assert np.array_equal(rm.resample(src, (int(w2), int(h2)), int(filt)), want), (k, rm.NAMES[filt], w, h, w2, h2)


def test_the_known_answers_of_the_header(golden):
    for name, n in (("known_up", 4), ("known_down", 2)):
        src, want = golden[name + "_in"], golden[name + "_out"]
        for f in rm.FILTERS:
            assert np.array_equal(rm.resample(src, (n, 1), f)[0], want[f])
    assert golden["known_up_out"].tolist() == [[0, 0, 255, 255], [0, 64, 191, 255], [0, 19, 236, 255], [0, 53, 202, 255], [0, 59, 196, 255]]
    assert golden["known_down_out"].tolist() == [[25, 235], [57, 207], [38, 224], [47, 217], [46, 220]]


def test_the_recorded_tables_are_the_models_and_the_librarys(golden):
    for k, (filt, n_in, n_out) in enumerate(golden["tables"]):
        bounds, K = rm.table(int(filt), int(n_in), int(n_out))
        assert np.array_equal(bounds, golden["bounds_%d" % k]) and np.array_equal(K, golden["K_%d" % k]), (filt, n_in, n_out)
        lb, lK = rs.resample_table(int(filt), int(n_in), int(n_out))
        assert np.array_equal(lb, bounds) and np.array_equal(lK, K), (filt, n_in, n_out)
        assert rs.resample_ksize(int(filt), int(n_in), int(n_out)) == rm.ksize(int(filt), int(n_in), int(n_out)) == K.shape[1]
        max_k, max_sum = rm.bound_sums(K)
        assert max_k < 2 ** 23 and max_sum < 2 ** 31


def test_the_model_equals_an_installed_pillow_on_a_grid():
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    pil = {rm.BOX: Image.BOX, rm.BILINEAR: Image.BILINEAR, rm.HAMMING: Image.HAMMING, rm.BICUBIC: Image.BICUBIC, rm.LANCZOS: Image.LANCZOS}
    rng = np.random.default_rng(5)
    n = 0
    for (w, h) in [(1, 1), (2, 1), (3, 3), (17, 13), (64, 48), (100, 37), (257, 5)]:
        for (w2, h2) in [(1, 1), (2, 3), (7, 5), (w, h), (w, 9), (33, h), (50, 50), (w * 3 // 2 + 1, h * 7)]:
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            if (w + h) % 2:
                img = (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
            for f in rm.FILTERS:
                want = np.asarray(Image.fromarray(img).resize((w2, h2), pil[f]))
                assert np.array_equal(rm.resample(img, (w2, h2), f), want), (PIL.__version__, rm.NAMES[f], w, h, w2, h2)
                n += 1
    assert n == 7 * 8 * 5
