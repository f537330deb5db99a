"""The definition of the box entries (include/sjpeg_hip.h, "THE DEFINITION of the box entries") restated in numpy integers
and Python doubles beside tests/resample_model.py: Pillow's reduce, the table of an axis from a float32 box, the five
steps of Image.resize(size, filter, box=, reducing_gap=), Image.thumbnail's size rule and ImageOps.fit's crop.  Nothing
here asks the library or Pillow for a sample.  tests/golden/resample_pillow_box.npz pins it to what Pillow 12.2.0 made;
test_resample_box_model_host.py compares the two, and an installed Pillow live."""
import math

import numpy as np

import resample_model as rm

FACTOR_MAX = 255


class Refused(ValueError):
    """a frame the box entries refuse; args[0] is one of "box", "gap", "factor", "tall" """


def f32(x):
    return float(np.float32(x))


def multiplier(n):
    """m(n): a float32 division, truncated"""
    return int(np.float32(4294967296.0) / np.float32(256 * n))


def half_up(S, n):
    """the exact half-up average of reduce_round.h -- NOT Pillow's reduce; here for the tests that tell the two apart"""
    return (2 * S + n) // (2 * n)


def reduce_sample(S, n):
    return (((S + n // 2) * multiplier(n)) & 0xFFFFFFFF) >> 24


def reduce(img, fx, fy, box=None):
    """Image.reduce((fx, fy), box=): img uint8 [h, w] or [h, w, c]"""
    h, w = img.shape[:2]
    x0, y0, x1, y1 = box if box is not None else (0, 0, w, h)
    ow, oh = -(-(x1 - x0) // fx), -(-(y1 - y0) // fy)
    out = np.empty((oh, ow) + img.shape[2:], np.uint8)
    src = img.astype(np.int64)
    for Y in range(oh):
        ys, ye = y0 + Y * fy, min(y0 + (Y + 1) * fy, y1)
        for X in range(ow):
            xs, xe = x0 + X * fx, min(x0 + (X + 1) * fx, x1)
            n = (xe - xs) * (ye - ys)
            S = src[ys:ye, xs:xe].reshape((n,) + img.shape[2:]).sum(axis=0)
            assert ((S + n // 2) * multiplier(n)).max() < 2 ** 32
            out[Y, X] = ((S + n // 2) * multiplier(n)) >> 24
    return out


def box_table(filt, n_in, n_out, b0, b1, double=False):
    """resample_model.table of an axis from its part [b0, b1): the ends and their difference in float32 (double=True:
    in doubles throughout, which is NOT Pillow -- for the test that shows the two differ)"""
    if double:
        scale = (b1 - b0) / n_out
    else:
        b0, b1 = np.float32(b0), np.float32(b1)
        scale = float(np.float32(b1 - b0)) / n_out
        b0 = float(b0)
    fs = max(scale, 1.0)
    support = rm.SUPPORT[filt] * fs
    ks = 2 * int(math.ceil(support)) + 1
    bounds = np.zeros((n_out, 2), np.int32)
    K = np.zeros((n_out, ks), np.int32)
    for xx in range(n_out):
        center = b0 + (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        n = min(n_in, int(center + support + 0.5)) - xmin
        w = [rm.filter_value(filt, (x + xmin - center + 0.5) / fs) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        bounds[xx] = (xmin, n)
        for x, v in enumerate(w):
            k = v / ww if ww != 0.0 else v
            K[xx, x] = int(k * (1 << rm.PRECISION_BITS) + 0.5) if k >= 0 else int(k * (1 << rm.PRECISION_BITS) - 0.5)
    return bounds, K


def decide(filt, W, H, size, box=None, gap=None):
    """steps 1 to 3: (fx, fy), the safe box, the reduced picture's size and the box inside it"""
    w2, h2 = size
    l, t, r, b = (0.0, 0.0, float(W), float(H)) if box is None else (float(v) for v in box)
    if not (0 <= l and 0 <= t and r <= W and b <= H and r - l > 0 and b - t > 0):
        raise Refused("box")
    if gap is not None and not gap >= 1.0:
        raise Refused("gap")
    fx = fy = 1
    if gap is not None:
        fx = int((r - l) / w2 / gap) or 1
        fy = int((b - t) / h2 / gap) or 1
    if fx > FACTOR_MAX or fy > FACTOR_MAX:
        raise Refused("factor")
    safe, inner = (0, 0, W, H), (l, t, r, b)
    if fx > 1 or fy > 1:
        s = rm.SUPPORT[filt] - 0.5
        sx, sy = (r - l) / w2, (b - t) / h2
        safe = (max(0, int(l - s * sx)), max(0, int(t - s * sy)), min(W, math.ceil(r + s * sx)), min(H, math.ceil(b + s * sy)))
        inner = ((l - safe[0]) / fx, (t - safe[1]) / fy, (r - safe[0]) / fx, (b - safe[1]) / fy)
        W, H = -(-(safe[2] - safe[0]) // fx), -(-(safe[3] - safe[1]) // fy)
    if H > 100 * W and h2 < H:
        raise Refused("tall")
    return (fx, fy), safe, (W, H), inner


def resize(img, size, filt, box=None, gap=None):
    """Image.resize(size, filt, box=box, reducing_gap=gap) of img uint8 [h, w] or [h, w, c]"""
    h, w = img.shape[:2]
    (fx, fy), safe, (W, H), inner = decide(filt, w, h, size, box, gap)
    if fx > 1 or fy > 1:
        img = reduce(img, fx, fy, safe)
    assert img.shape[:2] == (H, W)
    w2, h2 = size
    bf = [np.float32(v) for v in inner]
    out = img
    if w2 != W or bf[0] != 0 or bf[2] != W:
        out = np.swapaxes(rm.apply_axis(np.swapaxes(out, 0, 1), *box_table(filt, W, w2, bf[0], bf[2])), 0, 1)
    if h2 != H or bf[1] != 0 or bf[3] != H:
        out = rm.apply_axis(out, *box_table(filt, H, h2, bf[1], bf[3]))
    return np.ascontiguousarray(out)


def thumbnail_size(W, H, box):
    x, y = math.floor(box[0]), math.floor(box[1])
    if x >= W and y >= H:
        return W, H

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    aspect = W / H
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


def thumbnail(img, box, filt=rm.BICUBIC, gap=2.0):
    """what im.thumbnail(box, filt, reducing_gap=gap) leaves of img"""
    h, w = img.shape[:2]
    size = thumbnail_size(w, h, box)
    return img if size == (w, h) else resize(img, size, filt, None, gap)


def fit_crop(W, H, size, bleed=0.0, centering=(0.5, 0.5)):
    cx, cy = centering
    if not 0.0 <= cx <= 1.0:
        cx = 0.5
    if not 0.0 <= cy <= 1.0:
        cy = 0.5
    if not 0.0 <= bleed < 0.5:
        bleed = 0.0
    bx, by = bleed * W, bleed * H
    lw, lh = W - bx * 2, H - by * 2
    live, want = lw / lh, size[0] / size[1]
    if live == want:
        cw, ch = lw, lh
    elif live >= want:
        cw, ch = want * lh, lh
    else:
        cw, ch = lw, lw / want
    left, top = bx + (lw - cw) * cx, by + (lh - ch) * cy
    return (left, top, left + cw, top + ch)


def fit(img, size, filt=rm.BICUBIC, bleed=0.0, centering=(0.5, 0.5)):
    """ImageOps.fit(im, size, filt, bleed, centering)"""
    h, w = img.shape[:2]
    return resize(img, size, filt, fit_crop(w, h, size, bleed, centering))
