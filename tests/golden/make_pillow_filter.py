"""Writes tests/golden/pillow_filter.npz: what Pillow 12.2.0's ImageFilter.BoxBlur, GaussianBlur and UnsharpMask made of
small pictures, so that tests/pillow_filter_model.py is pinned where Pillow is not installed.  Every case is written
only after the model equalled Pillow byte for byte on it.  The pictures themselves are not stored: they are
pillow_filter_cases.picture(), integers of the position alone.

    python tests/golden/make_pillow_filter.py          (needs Pillow 12.2.0)

Arrays: out_<k> uint8, what Pillow made of case k of pillow_filter_cases.CASES; `trap3` int32 [1], the threshold of the
constructed case -- the blurred difference at its centre; `chain` uint8: im.thumbnail(CHAIN_BOX) then
filter(UnsharpMask(2, 150, 3)) of pillow_filter_cases.chain_picture()."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pillow_filter_cases as pc  # noqa: E402
import pillow_filter_model as pm  # noqa: E402


def pillow_filter(spec):
    from PIL import ImageFilter
    return {"box": ImageFilter.BoxBlur, "gaussian": ImageFilter.GaussianBlur, "unsharp": ImageFilter.UnsharpMask}[spec[0]](*spec[1:])


def main():
    import PIL
    from PIL import Image
    assert PIL.__version__ == "12.2.0", PIL.__version__
    arrays = {}
    for k, (mode, size, spec) in enumerate(pc.CASES):
        img = pc.picture(mode, size, k)
        out = np.asarray(Image.fromarray(img).filter(pillow_filter(spec)))
        assert np.array_equal(pm.apply(img, spec), out), (k, mode, size, spec)
        arrays["out_%d" % k] = out
    img, thr = pc.trap3_picture(), pc.trap3_threshold()
    out = np.asarray(Image.fromarray(img).filter(pillow_filter(("unsharp", pc.TRAP3_RADIUS, 150, thr))))
    assert np.array_equal(pm.unsharp_mask(img, pc.TRAP3_RADIUS, 150, thr), out) and out[4, 4] == img[4, 4]
    assert np.asarray(Image.fromarray(img).filter(pillow_filter(("unsharp", pc.TRAP3_RADIUS, 150, thr - 1))))[4, 4] != img[4, 4]
    arrays["trap3"], arrays["trap3_out"] = np.array([thr], np.int32), out
    im = Image.fromarray(pc.chain_picture())
    im.thumbnail(pc.CHAIN_BOX)                                     # (BICUBIC, reducing_gap 2.0: Pillow's defaults)
    arrays["chain_thumbnail"] = np.asarray(im)
    arrays["chain"] = np.asarray(im.filter(pillow_filter(("unsharp", 2, 150, 3))))
    path = os.path.join(HERE, "pillow_filter.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(pc.CASES), "cases")


if __name__ == "__main__":
    main()
