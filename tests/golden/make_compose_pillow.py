"""Writes tests/golden/compose_pillow.npz: what Pillow 12.2.0's ImageOps.contain / pad and Image.paste of an RGBA
overlay with itself as mask made of small pictures, so that tests/compose_model.py is pinned where Pillow is not
installed.  Every case is written only after the model equalled Pillow on it.  The pictures and overlays themselves are
not stored: they are compose_cases' functions, integers of the position alone.

    python tests/golden/make_compose_pillow.py          (needs Pillow 12.2.0)

Arrays: `sizes` int32 [len(SIZES), 4]: contain's (w', h') and pad's (x, y) of compose_cases.SIZES; paste_<k> uint8: case k
of PASTES; chain_<k>_thumbnail, chain_<k>_sharp, chain_<k>_pad, chain_<k> uint8: thumbnail(CHAIN_BOX), then
filter(UnsharpMask(2, 150, 3)), then ImageOps.pad(CHAIN_BOX, color=CHAIN_COLOUR), then paste(logo, CHAIN_LOGO_AT, logo)
of chain_source(k); pad_<k> uint8: case k of PADS."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import compose_cases as cc  # noqa: E402
import compose_model as cm  # noqa: E402


def main():
    import PIL
    from PIL import Image, ImageFilter, ImageOps
    assert PIL.__version__ == "12.2.0", PIL.__version__
    arrays = {}
    sizes = []
    for w, h, box, centering in cc.SIZES:
        im = Image.new("L", (w, h), 200)
        contained = ImageOps.contain(im, box)
        padded = np.asarray(ImageOps.pad(im, box, color=0, centering=centering))
        ys, xs = np.nonzero(padded == 200)
        assert padded.shape == (box[1], box[0]) and len(xs) == contained.width * contained.height
        sizes.append((contained.width, contained.height, int(xs.min()), int(ys.min())))
        assert cm.contain_size(w, h, box) == sizes[-1][:2] and cm.pad_place(*sizes[-1][:2], box, centering) == sizes[-1][2:], (w, h, box)
    arrays["sizes"] = np.array(sizes, np.int32)
    for w, h, box in cc.SIZES_REFUSED:
        try:
            ImageOps.contain(Image.new("L", (w, h)), box)
            raise AssertionError("Pillow made a picture with a side of 0")
        except ValueError:
            assert 0 in cm.contain_size(w, h, box)
    for k, (mode, size, pastes) in enumerate(cc.PASTES):
        img = cc.base(mode, size, k)
        im, want = Image.fromarray(img), img
        for o, at in pastes:
            logo = Image.fromarray(cc.overlay(o), "RGBA")
            im.paste(logo, at, logo)
            want = cm.paste(want, cc.overlay(o), at)
        out = np.asarray(im)
        assert np.array_equal(out, want), (k, mode, size, pastes)
        arrays["paste_%d" % k] = out
    assert not np.array_equal(arrays["paste_0"], arrays["paste_1"])
    logo = Image.fromarray(cc.logo(), "RGBA")
    for k in range(len(cc.CHAIN_SOURCES)):
        im = Image.fromarray(cc.chain_source(k))
        im.thumbnail(cc.CHAIN_BOX)                                    # (BICUBIC, reducing_gap 2.0: Pillow's defaults)
        arrays["chain_%d_thumbnail" % k] = np.asarray(im)
        im = im.filter(ImageFilter.UnsharpMask(2, 150, 3))
        arrays["chain_%d_sharp" % k] = np.asarray(im)
        im = ImageOps.pad(im, cc.CHAIN_BOX, color=cc.CHAIN_COLOUR)
        arrays["chain_%d_pad" % k] = np.asarray(im)
        im.paste(logo, cc.CHAIN_LOGO_AT, logo)
        arrays["chain_%d" % k] = np.asarray(im)
        want = cm.compose(arrays["chain_%d_sharp" % k], cc.CHAIN_BOX, colour=cc.CHAIN_COLOUR, overlays=[(cc.logo(), cc.CHAIN_LOGO_AT, "top-left")])
        assert np.array_equal(want, arrays["chain_%d" % k]), k
    for k, (mode, size, box, colour, centering) in enumerate(cc.PADS):
        im = Image.fromarray(cc.base(mode, size, 50 + k))
        arrays["pad_%d" % k] = np.asarray(ImageOps.pad(im, box, Image.Resampling.BICUBIC, color=colour if mode == "RGB" else colour[0], centering=centering))
    path = os.path.join(HERE, "compose_pillow.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
