"""The definition of the resampling entries (include/sjpeg_hip.h, "resampling with Pillow's filters") restated in numpy
integers and Python doubles: the tables of one axis and a picture of bytes resampled along x, then along y, with a
uint8 intermediate.  Nothing here asks the library for a sample.  tests/golden/resample_pillow.npz pins it to what
Pillow 12.2.0 made; test_resample_model_host.py compares the two, and an installed Pillow live."""
import math

import numpy as np

BOX, BILINEAR, HAMMING, BICUBIC, LANCZOS = range(5)
FILTERS = (BOX, BILINEAR, HAMMING, BICUBIC, LANCZOS)
NAMES = ("box", "bilinear", "hamming", "bicubic", "lanczos")
SUPPORT = (0.5, 1.0, 1.0, 2.0, 3.0)
PRECISION_BITS = 22

_F054 = float(np.float32(0.54))              # (the two constants are floats promoted to double)
_F046 = float(np.float32(0.46))


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def filter_value(filt, x):
    """f(x) in IEEE double"""
    if filt == BOX:
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if filt == LANCZOS:
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    if x < 0.0:
        x = -x
    if filt == BILINEAR:
        return 1.0 - x if x < 1.0 else 0.0
    if filt == HAMMING:
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x = x * math.pi
        return math.sin(x) / x * (_F054 + _F046 * math.cos(x))
    if filt == BICUBIC:
        a = -0.5
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    raise ValueError(filt)


def ksize(filt, n_in, n_out):
    scale = n_in / n_out
    fs = max(scale, 1.0)
    return 2 * int(math.ceil(SUPPORT[filt] * fs)) + 1


def table(filt, n_in, n_out):
    """(bounds int32 [n_out, 2] -- xmin and n --, K int32 [n_out, ksize], unused entries 0)"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[filt] * fs
    ks = 2 * int(math.ceil(support)) + 1
    bounds = np.zeros((n_out, 2), np.int32)
    K = np.zeros((n_out, ks), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        n = min(n_in, int(center + support + 0.5)) - xmin
        w = [filter_value(filt, (x + xmin - center + 0.5) / fs) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        bounds[xx] = (xmin, n)
        for x, v in enumerate(w):
            k = v / ww if ww != 0.0 else v
            K[xx, x] = int(k * (1 << PRECISION_BITS) + 0.5) if k >= 0 else int(k * (1 << PRECISION_BITS) - 0.5)
    return bounds, K


def identity_table(n):
    """the table of a pass that is not run, as the plan states it: one tap of 2^22 on the sample itself"""
    bounds = np.stack([np.arange(n, dtype=np.int32), np.ones(n, np.int32)], axis=1)
    return bounds, np.full((n, 1), 1 << PRECISION_BITS, np.int32)


def apply_axis(img, bounds, K):
    """img uint8 [n_in, ...] resampled along axis 0 with a table: uint8 [n_out, ...]"""
    out = np.empty((bounds.shape[0],) + img.shape[1:], np.uint8)
    src = img.astype(np.int64)
    for xx in range(bounds.shape[0]):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        k = K[xx, :n].astype(np.int64).reshape((n,) + (1,) * (img.ndim - 1))
        ss = (1 << (PRECISION_BITS - 1)) + (k * src[xmin:xmin + n]).sum(axis=0)
        assert np.abs(ss).max() < 2 ** 31
        out[xx] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return out


_tables = {}


def _table(filt, n_in, n_out):
    key = (filt, n_in, n_out)
    if key not in _tables:
        _tables[key] = table(filt, n_in, n_out)
    return _tables[key]


def resample(img, size, filt):
    """img uint8 [h, w] or [h, w, c] to size = (w2, h2): along x, then along y; a pass whose sizes agree is not run"""
    w2, h2 = size
    h, w = img.shape[:2]
    out = img
    if w2 != w:
        out = np.swapaxes(apply_axis(np.swapaxes(out, 0, 1), *_table(filt, w, w2)), 0, 1)
    if h2 != h:
        out = apply_axis(out, *_table(filt, h, h2))
    return np.ascontiguousarray(out)


def turn(img, orientation):
    """the upright picture of a stored one (EXIF tag 0x0112, 1..8)"""
    o = orientation
    if o == 2:
        return img[:, ::-1]
    if o == 3:
        return img[::-1, ::-1]
    if o == 4:
        return img[::-1]
    if o == 5:
        return np.swapaxes(img, 0, 1)
    if o == 6:
        return np.swapaxes(img, 0, 1)[:, ::-1]
    if o == 7:
        return np.swapaxes(img, 0, 1)[::-1, ::-1]
    if o == 8:
        return np.swapaxes(img, 0, 1)[::-1]
    return img


def bound_sums(K):
    """(max |K|, max over rows of 2^21 + 255 * max(sum of positive K, sum of |negative K|))"""
    k = K.astype(np.int64)
    pos = np.where(k > 0, k, 0).sum(axis=1)
    neg = np.where(k < 0, -k, 0).sum(axis=1)
    return int(np.abs(k).max()), int((1 << 21) + 255 * np.maximum(pos, neg).max())
