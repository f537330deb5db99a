"""Writes tests/golden/resample_pillow_box.npz: small pictures and what Pillow 12.2.0 made of them with the calls behind
Image.thumbnail and ImageOps.fit -- Image.reduce, Image.resize(box=), Image.resize(box=, reducing_gap=), Image.thumbnail
and ImageOps.fit -- so that tests/resample_box_model.py is pinned where Pillow is not installed.  Every case is written
only after the model equalled Pillow byte for byte on it.

    python tests/golden/make_resample_pillow_box.py          (needs Pillow 12.2.0)

Arrays: `calls` int32 [n] (REDUCE, RESIZE_BOX, RESIZE_GAP, THUMBNAIL, FIT); `ints` int32 [n, 4]: (fx, fy, 0, 0) of a
reduce, else (filter, w2, h2, 0) -- a thumbnail's w2, h2 are 0: its size follows from its box --; `doubles` float64
[n, 5]: a reduce's integer box, a resize's source box (l, t, r, b) and reducing_gap (0: none), a thumbnail's (bw, bh, 0,
0, reducing_gap), a fit's (bleed, cx, cy, 0, 0); in_<k> uint8 [h, w(, 3)]; out_<k> what Pillow made."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resample_box_model as bm  # noqa: E402
import resample_model as rm  # noqa: E402

REDUCE, RESIZE_BOX, RESIZE_GAP, THUMBNAIL, FIT = range(5)

# (w, h, channels, fx, fy, box): edge and corner blocks with fewer samples, origins that are no multiple of the factor
REDUCES = [(29, 23, 3, 3, 2, (0, 0, 29, 23)), (30, 17, 1, 4, 4, (3, 1, 30, 16)), (16, 16, 3, 2, 2, (0, 0, 16, 16)), (31, 9, 1, 7, 3, (2, 2, 31, 9)),
           (12, 40, 1, 1, 8, (1, 5, 11, 38)), (40, 6, 3, 8, 1, (7, 0, 40, 5)), (25, 25, 1, 5, 6, (0, 0, 25, 25)), (9, 9, 3, 3, 3, (1, 1, 9, 9))]
# (w, h, channels, w2, h2, filter, box): fractional and whole boxes, interior and on the edge, shrinking and enlarging
BOXES = [(40, 30, 1, 11, 9, rm.BICUBIC, (0.1, 0.2, 30.7, 20.3)), (40, 30, 3, 13, 7, rm.LANCZOS, (10.5, 8.25, 29.75, 21.5)),
         (24, 18, 1, 24, 18, rm.BILINEAR, (0.5, 0.5, 24, 18)), (24, 18, 3, 9, 18, rm.HAMMING, (3, 0, 21, 18)),
         (31, 29, 1, 40, 35, rm.BICUBIC, (2.3, 4.1, 17.9, 19.6)), (31, 29, 1, 7, 5, rm.BOX, (0, 0, 30.5, 28.5)),
         (20, 20, 3, 6, 6, rm.LANCZOS, (0, 0, 20, 20)), (33, 12, 1, 5, 4, rm.BOX, (1.7, 0.3, 32.2, 11.9)),
         (17, 13, 3, 4, 3, rm.BILINEAR, (0.25, 0.75, 16.5, 12.25)), (50, 10, 1, 9, 10, rm.HAMMING, (12.6, 0, 49.4, 10))]
# (w, h, channels, w2, h2, filter, box or None, gap)
GAPS = [(37, 29, 3, 6, 7, rm.BICUBIC, None, 2.0), (64, 48, 1, 7, 5, rm.LANCZOS, None, 2.0), (64, 48, 1, 8, 6, rm.BILINEAR, (5.5, 3.25, 60.0, 44.75), 1.0),
        (90, 20, 1, 6, 9, rm.HAMMING, (11, 2, 83, 19), 3.0), (45, 45, 1, 5, 5, rm.BOX, (0.3, 0.3, 44.6, 44.6), 1.5),
        (30, 30, 1, 10, 10, rm.BICUBIC, None, 2.0), (200, 4, 1, 5, 2, rm.LANCZOS, None, 2.0), (41, 37, 3, 4, 9, rm.BICUBIC, (9.2, 0, 41, 30.1), 1.0)]
# (w, h, channels, box, filter, gap or None)
THUMBNAILS = [(64, 36, 3, (16, 16), rm.BICUBIC, 2.0), (48, 64, 1, (10.9, 20), rm.BICUBIC, 2.0), (70, 50, 1, (9, 9), rm.LANCZOS, 3.0),
              (33, 47, 1, (12, 12), rm.BILINEAR, None), (20, 10, 3, (64, 64), rm.BICUBIC, 2.0), (100, 7, 1, (13, 5), rm.HAMMING, 1.0)]
# (w, h, channels, w2, h2, filter, bleed, centering)
FITS = [(40, 30, 3, 8, 8, rm.BICUBIC, 0.0, (0.5, 0.5)), (30, 40, 1, 9, 5, rm.LANCZOS, 0.0, (0.5, 0.5)), (37, 23, 1, 7, 7, rm.BICUBIC, 0.1, (0.0, 1.0)),
        (23, 37, 3, 6, 4, rm.BILINEAR, 0.03, (0.3, 0.8)), (32, 32, 1, 11, 11, rm.HAMMING, 0.0, (0.5, 0.5)), (19, 31, 1, 25, 25, rm.BOX, 0.0, (2.0, 0.5))]


def main():
    import PIL
    from PIL import Image, ImageOps
    assert PIL.__version__ == "12.2.0", PIL.__version__
    pil = {rm.BOX: Image.BOX, rm.BILINEAR: Image.BILINEAR, rm.HAMMING: Image.HAMMING, rm.BICUBIC: Image.BICUBIC, rm.LANCZOS: Image.LANCZOS}
    rng = np.random.default_rng(20261021)
    arrays, calls, ints, doubles = {}, [], [], []

    def record(call, i, d, img, out, mine):
        assert np.array_equal(mine, out), (call, i, d)
        k = len(calls)
        calls.append(call); ints.append(tuple(i) + (0,) * (4 - len(i))); doubles.append(tuple(d) + (0.0,) * (5 - len(d)))
        arrays["in_%d" % k], arrays["out_%d" % k] = img, out

    def picture(w, h, c):
        return rng.integers(0, 256, (h, w) if c == 1 else (h, w, c), dtype=np.uint8)

    for (w, h, c, fx, fy, box) in REDUCES:
        img = picture(w, h, c)
        record(REDUCE, (fx, fy), box, img, np.asarray(Image.fromarray(img).reduce((fx, fy), box=box)), bm.reduce(img, fx, fy, box))
    for (w, h, c, w2, h2, f, box) in BOXES:
        img = picture(w, h, c)
        record(RESIZE_BOX, (f, w2, h2), box, img, np.asarray(Image.fromarray(img).resize((w2, h2), pil[f], box=box)), bm.resize(img, (w2, h2), f, box))
    for (w, h, c, w2, h2, f, box, gap) in GAPS:
        img = picture(w, h, c)
        out = np.asarray(Image.fromarray(img).resize((w2, h2), pil[f], box=box, reducing_gap=gap))
        record(RESIZE_GAP, (f, w2, h2), (box or (0, 0, w, h)) + (gap,), img, out, bm.resize(img, (w2, h2), f, box, gap))
    for (w, h, c, box, f, gap) in THUMBNAILS:
        img = picture(w, h, c)
        im = Image.fromarray(img)
        im.thumbnail(box, pil[f], reducing_gap=gap)
        assert im.size == bm.thumbnail_size(w, h, box)
        record(THUMBNAIL, (f, 0, 0), tuple(box) + (0, 0, gap or 0.0), img, np.asarray(im), bm.thumbnail(img, box, f, gap))
    for (w, h, c, w2, h2, f, bleed, centering) in FITS:
        img = picture(w, h, c)
        out = np.asarray(ImageOps.fit(Image.fromarray(img), (w2, h2), pil[f], bleed, centering))
        record(FIT, (f, w2, h2), (bleed,) + tuple(centering), img, out, bm.fit(img, (w2, h2), f, bleed, centering))
    arrays["calls"], arrays["ints"], arrays["doubles"] = np.array(calls, np.int32), np.array(ints, np.int32), np.array(doubles, np.float64)
    path = os.path.join(HERE, "resample_pillow_box.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(calls), "cases")


if __name__ == "__main__":
    main()
