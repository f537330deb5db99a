"""Pillow 12.2.0's BoxBlur, GaussianBlur and UnsharpMask on pictures of bytes, restated in numpy integers and float32
scalars -- the definition sjpeg_hip.h gives for the _filtered_ entries, written independently of the C++ that implements
it (sjpeg_amd/csrc/pillow_filter_math.h).  tests/test_pillow_filter_model_host.py holds it to Pillow's recorded and live
bytes; the other tests hold the library to it.

A picture is a uint8 array [h, w] (gray) or [h, w, 3]; every band is filtered alike."""
import math

import numpy as np

NONE, BOX, GAUSSIAN, UNSHARP = 0, 1, 2, 3
RADIUS_MAX = 63
f32 = np.float32


def box_weights(fr):
    """(r, ww, fw) of one box pass of float radius fr: the division in float32, truncated"""
    fr = f32(fr)
    r = int(fr)
    ww = int(f32(16777216.0) / (fr * f32(2.0) + f32(1.0)))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def gaussian_radius(sigma):
    """the box radius of the three passes that make a Gaussian: every operation rounded to float32 but sqrt and floor,
    which take and return double"""
    sigma = f32(sigma)
    s2 = f32(sigma * sigma) / f32(3.0)
    L = f32(math.sqrt(float(f32(f32(12.0) * s2) + f32(1.0))))
    l = f32(math.floor(float(f32(L - f32(1.0)) / f32(2.0))))
    a = f32(f32(f32(2.0) * l) + f32(1.0)) * f32(f32(l * f32(l + f32(1.0))) - f32(f32(3.0) * s2))
    a = f32(a) / f32(f32(6.0) * f32(s2 - f32(f32(l + f32(1.0)) * f32(l + f32(1.0)))))
    return f32(l + f32(a))


def gaussian_radius_double(sigma):
    """the same formula in doubles: NOT Pillow's radius for many sigmas (the test shows one)"""
    s2 = float(sigma) * float(sigma) / 3.0
    L = math.sqrt(12.0 * s2 + 1.0)
    l = math.floor((L - 1.0) / 2.0)
    a = (2 * l + 1) * (l * (l + 1) - 3 * s2)
    a /= 6 * (s2 - (l + 1) * (l + 1))
    return l + a


def axis_weights(kind, radius):
    """(r, ww, fw, passes) of an axis of a filter kind; passes 0: the axis is skipped"""
    if kind == NONE:
        return 0, 1 << 24, 0, 0
    fr = f32(radius) if kind == BOX else gaussian_radius(radius)
    if not fr > 0:
        return 0, 1 << 24, 0, 0
    return box_weights(fr) + (1 if kind == BOX else 3,)


def box_pass(a, axis, r, ww, fw):
    """one pass along `axis` of a uint8 array: the closed form, edges replicated"""
    n = a.shape[axis]
    x = np.arange(n)
    src = np.moveaxis(a, axis, 0).astype(np.uint64)
    S = np.zeros_like(src)
    for d in range(-r, r + 1):
        S += src[np.clip(x + d, 0, n - 1)]
    edge = src[np.clip(x - r - 1, 0, n - 1)] + src[np.clip(x + r + 1, 0, n - 1)]
    v = ww * S + fw * edge + (1 << 23)
    assert int(v.max()) < 1 << 32
    return np.moveaxis((v >> 24).astype(np.uint8), 0, axis)


def _pair(radius):
    return (radius, radius) if isinstance(radius, (int, float, np.integer, np.floating)) else tuple(radius)


def blur(a, kind, radius):
    """BoxBlur(radius) (kind BOX) or GaussianBlur(radius) of a picture: rows first, then columns"""
    rx, ry = _pair(radius)
    out = np.ascontiguousarray(a)
    for axis, rad in ((1, rx), (0, ry)):
        r, ww, fw, passes = axis_weights(kind, rad)
        for _ in range(passes):
            out = box_pass(out, axis, r, ww, fw)
    return out


def box_blur(a, radius):
    return blur(a, BOX, radius)


def gaussian_blur(a, radius):
    return blur(a, GAUSSIAN, radius)


def unsharp_mask(a, radius=2, percent=150, threshold=3):
    """UnsharpMask: strict comparison, C's division toward zero"""
    p = a.astype(np.int64)
    d = p - gaussian_blur(a, radius).astype(np.int64)
    scaled = d * int(percent)
    q = np.sign(scaled) * (np.abs(scaled) // 100)
    return np.where(np.abs(d) > int(threshold), np.clip(p + q, 0, 255), p).astype(np.uint8)


def apply(a, spec):
    """spec: None, ("box", radius), ("gaussian", radius) or ("unsharp", radius, percent, threshold)"""
    if spec is None or spec[0] == "none":
        return np.ascontiguousarray(a)
    if spec[0] == "box":
        return box_blur(a, spec[1])
    if spec[0] == "gaussian":
        return gaussian_blur(a, spec[1])
    if spec[0] == "unsharp":
        return unsharp_mask(a, *spec[1:])
    raise ValueError(spec)
