"""Writes tests/golden/resample_pillow.npz: small pictures, what Image.resize of Pillow 12.2.0 made of them with each of
the five filters, and a few whole tables.  Pillow does not hand out its coefficient tables; the recorded ones are those
of tests/resample_model.py, written only after the model equalled Pillow byte for byte on every case recorded here --
they pin the C++ table builder (the host's sin and cos included) where Pillow is not installed.

    python tests/golden/make_resample_pillow.py          (needs Pillow 12.2.0)

Arrays: `cases` int32 [n, 7] = (filter, w, h, channels, w2, h2, picture kind); in_<k> uint8 [h, w(, 3)]; out_<k> what
Pillow made; `tables` int32 [m, 3] = (filter, in, out); bounds_<k> int32 [out, 2], K_<k> int32 [out, ksize]."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resample_model as rm  # noqa: E402

RANDOM, NOISE, CHECKER = range(3)
# (w, h, w2, h2): shrinking and enlarging, each axis alone, neither, mixed, 1 x 1 and other tiny ones, a long strip
GEOMETRIES = [(1, 1, 1, 1), (1, 1, 5, 3), (2, 1, 1, 2), (3, 3, 1, 1), (3, 3, 7, 2), (24, 18, 7, 5), (24, 18, 24, 11), (24, 18, 36, 18),
              (9, 7, 63, 11), (16, 16, 24, 10), (20, 12, 20, 12), (257, 3, 3, 2), (31, 29, 13, 40)]
TABLES = [(f, i, o) for f in rm.FILTERS for (i, o) in ((1, 1), (1, 4), (7, 3), (16, 24), (100, 7), (257, 3))] + [(rm.LANCZOS, 1920, 320),
                                                                                                                (rm.BICUBIC, 1080, 180)]


def picture(rng, kind, h, w, c):
    shape = (h, w) if c == 1 else (h, w, c)
    if kind == RANDOM:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == NOISE:
        return (rng.integers(0, 2, shape) * 255).astype(np.uint8)
    yy, xx = np.mgrid[:h, :w]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    return board if c == 1 else np.repeat(board[:, :, None], c, axis=2).copy()


def main():
    import PIL
    from PIL import Image
    assert PIL.__version__ == "12.2.0", PIL.__version__
    pil = {rm.BOX: Image.BOX, rm.BILINEAR: Image.BILINEAR, rm.HAMMING: Image.HAMMING, rm.BICUBIC: Image.BICUBIC, rm.LANCZOS: Image.LANCZOS}
    rng = np.random.default_rng(20261020)
    arrays, cases = {}, []
    for g, (w, h, w2, h2) in enumerate(GEOMETRIES):
        for filt in rm.FILTERS:
            k = len(cases)
            kind, c = (g + filt) % 3, 1 if (g + filt) % 4 == 3 else 3
            img = picture(rng, kind, h, w, c)
            out = np.asarray(Image.fromarray(img).resize((w2, h2), pil[filt]))
            assert np.array_equal(rm.resample(img, (w2, h2), filt), out), (filt, w, h, w2, h2)
            cases.append((filt, w, h, c, w2, h2, kind))
            arrays["in_%d" % k], arrays["out_%d" % k] = img, out
    # the known answers the header states: two rows, to 4 and to 2 samples, per filter
    for name, row, n in (("known_up", [0, 255], 4), ("known_down", [10, 20, 30, 40, 250, 240, 230, 220], 2)):
        src = np.array([row], np.uint8)
        arrays[name + "_in"] = src
        arrays[name + "_out"] = np.stack([np.asarray(Image.fromarray(src).resize((n, 1), pil[f]))[0] for f in rm.FILTERS])
    arrays["cases"] = np.array(cases, np.int32)
    arrays["tables"] = np.array(TABLES, np.int32)
    for k, (filt, n_in, n_out) in enumerate(TABLES):
        arrays["bounds_%d" % k], arrays["K_%d" % k] = rm.table(filt, n_in, n_out)
    path = os.path.join(HERE, "resample_pillow.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases,", len(TABLES), "tables")


if __name__ == "__main__":
    main()
