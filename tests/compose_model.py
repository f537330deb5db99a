"""The compose stage's definition (include/sjpeg_hip.h, "composed behind that") in numpy integers and Python doubles:
Pillow 12.2.0's paste of an RGBA overlay with itself as mask, its luma for a gray base, ImageOps.contain's size,
ImageOps.pad's place and the anchors of an overlay place.  Nothing here uses the library."""
import numpy as np

TOP_LEFT, TOP_RIGHT, BOTTOM_LEFT, BOTTOM_RIGHT, CENTRE = range(5)
ANCHORS = {"top-left": 0, "top-right": 1, "bottom-left": 2, "bottom-right": 3, "centre": 4, "center": 4}


def blend(dst, src, a):
    """dst under src with alpha a, all 0..255 (ints or integer arrays): (dst * (255 - a) + src * a + 127) / 255"""
    dst, src, a = (np.asarray(v, np.int64) for v in (dst, src, a))
    t = dst * (255 - a) + src * a + 128
    return ((t >> 8) + t) >> 8


def luma(r, g, b):
    """the overlay's colour on a gray base: convert("L")"""
    r, g, b = (np.asarray(v, np.int64) for v in (r, g, b))
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16


def contain_size(w, h, box):
    """ImageOps.contain's target; round is Python's: half to even, on the double"""
    bw, bh = box
    im, dest = w / h, bw / bh
    if im == dest:
        return bw, bh
    if im > dest:
        return bw, round(h / w * bw)
    return round(w / h * bh), bh


def pad_place(w, h, canvas, centering=(0.5, 0.5)):
    """where ImageOps.pad puts a w x h picture that lies inside canvas"""
    cw, ch = canvas
    return round((cw - w) * max(0, min(centering[0], 1))), round((ch - h) * max(0, min(centering[1], 1)))


def anchor_place(anchor, canvas, size, xy):
    """the top-left of an overlay of `size` on `canvas`: (x, y) the margin inward from the anchor"""
    anchor = ANCHORS.get(anchor, anchor)
    (cw, ch), (ow, oh), (x, y) = canvas, size, xy
    if anchor == CENTRE:
        return (cw - ow) // 2 + x, (ch - oh) // 2 + y
    return (cw - ow - x if anchor in (TOP_RIGHT, BOTTOM_RIGHT) else x), (ch - oh - y if anchor in (BOTTOM_LEFT, BOTTOM_RIGHT) else y)


def paste(base, overlay, at):
    """base ([h, w, 3] or [h, w] uint8) with the RGBA overlay ([oh, ow, 4] uint8) pasted with itself as mask, its
    top-left at `at`, clipped; a new array"""
    out = base.copy()
    H, W = base.shape[:2]
    oh, ow = overlay.shape[:2]
    ox, oy = at
    x0, y0, x1, y1 = max(ox, 0), max(oy, 0), min(ox + ow, W), min(oy + oh, H)
    if x0 >= x1 or y0 >= y1:
        return out
    part = overlay[y0 - oy:y1 - oy, x0 - ox:x1 - ox].astype(np.int64)
    a = part[..., 3]
    if base.ndim == 3:
        out[y0:y1, x0:x1] = blend(base[y0:y1, x0:x1], part[..., :3], a[..., None]).astype(np.uint8)
    else:
        out[y0:y1, x0:x1] = blend(base[y0:y1, x0:x1], luma(part[..., 0], part[..., 1], part[..., 2]), a).astype(np.uint8)
    return out


def compose(pic, canvas=None, at=None, centering=None, colour=(0, 0, 0), overlays=()):
    """The canvas picture: pic ([h, w, 3] or [h, w] uint8) on a canvas (cw, ch) of colour (None: its own size) at `at`
    or by the centering (neither: centred, as Compose does), then overlays [(rgba, (x, y), anchor), ...] in list order"""
    h, w = pic.shape[:2]
    cw, ch = canvas if canvas is not None else (w, h)
    if centering is not None or (at is None and canvas is not None):
        at = pad_place(w, h, (cw, ch), centering if centering is not None else (0.5, 0.5))
    px, py = at if at is not None else (0, 0)
    assert 0 <= px and 0 <= py and px + w <= cw and py + h <= ch
    if pic.ndim == 3:
        out = np.empty((ch, cw, 3), np.uint8)
        out[:] = np.asarray(colour, np.uint8)
    else:
        out = np.full((ch, cw), colour[0], np.uint8)
    out[py:py + h, px:px + w] = pic
    for rgba, xy, anchor in overlays:
        out = paste(out, rgba, anchor_place(anchor, (cw, ch), (rgba.shape[1], rgba.shape[0]), xy))
    return out
