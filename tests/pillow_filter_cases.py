"""The cases tests/golden/pillow_filter.npz records Pillow's answers for, and their pictures -- integers of the position
alone, so that the fixture holds only what Pillow made.  Shared by tests/golden/make_pillow_filter.py and the tests."""
import numpy as np

import pillow_filter_model as pm

# (mode, (w, h), spec); spec as pillow_filter_model.apply takes it
CASES = [
    # box radii: 0.3 and 2.7 differ where the weight is divided in double (trap 1); 5 on 5 x 7 clamps at both ends at once
    ("L", (5, 7), ("box", 0.3)), ("RGB", (17, 9), ("box", 2.7)), ("L", (2, 3), ("box", 0.5)), ("RGB", (1, 1), ("box", 1)),
    ("L", (5, 7), ("box", 5)), ("RGB", (5, 7), ("box", 5)), ("L", (17, 9), ("box", 63.9)), ("RGB", (17, 9), ("box", 1)),
    ("RGB", (97, 33), ("box", (0, 2))), ("L", (97, 33), ("box", (3, 0))), ("L", (97, 33), ("box", 0.3)), ("L", (97, 33), ("box", 2.7)),
    # sigmas: 1 has r = 0
    ("L", (17, 9), ("gaussian", 1)), ("RGB", (97, 33), ("gaussian", 2)), ("L", (97, 33), ("gaussian", 3.3)),
    ("RGB", (17, 9), ("gaussian", (1.5, 4))), ("L", (5, 7), ("gaussian", (0, 3))), ("RGB", (2, 3), ("gaussian", 0)), ("L", (1, 1), ("gaussian", 2)),
    ("RGB", (5, 7), ("gaussian", 2)),
    # unsharp masks: (0.6, 500, 1) clips both ways and truncates negative differences toward zero; threshold 255: identity
    ("RGB", (97, 33), ("unsharp", 2, 150, 3)), ("L", (17, 9), ("unsharp", 1, 80, 0)), ("RGB", (17, 9), ("unsharp", 0.6, 500, 1)),
    ("L", (97, 33), ("unsharp", 0.6, 500, 1)), ("L", (5, 7), ("unsharp", 2, 150, 255)), ("RGB", (2, 3), ("unsharp", 0, 150, 0)),
    ("L", (1, 1), ("unsharp", 2, 150, 3)),
]
TRAP3_RADIUS = 1
CHAIN_BOX = (48, 48)


def _hash(h, w, c, seed):
    y, x, ch = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), np.arange(c, dtype=np.uint64), indexing="ij")
    v = (x * np.uint64(73) + y * np.uint64(151) + ch * np.uint64(31) + np.uint64(seed) * np.uint64(977) + np.uint64(12345)) * np.uint64(2654435761)
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    return (v >> np.uint64(13)) & np.uint64(255)


def picture(mode, size, seed):
    """noise over the whole range: every rounding and both clips occur"""
    w, h = size
    a = _hash(h, w, 1 if mode == "L" else 3, seed).astype(np.uint8)
    return np.ascontiguousarray(a[:, :, 0] if mode == "L" else a)


def smooth_picture(w, h, c, seed):
    """edges, ramps and a little noise: what a photograph gives an unsharp mask"""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    planes = []
    for ch in range(c):
        v = (x * (3 + ch) + y * (5 - ch)) % 256 // 2 + 60 * ((x // 23 + y // 17 + ch) % 2) + (_hash(h, w, 1, seed + ch)[:, :, 0].astype(np.int64) % 24)
        planes.append(np.clip(v, 0, 255))
    a = np.stack(planes, axis=2).astype(np.uint8)
    return np.ascontiguousarray(a[:, :, 0] if c == 1 else a)


def trap3_picture():
    a = np.full((9, 9), 100, np.uint8)
    a[4, 4] = 160
    return a


def trap3_threshold():
    """the blurred difference at the centre of trap3_picture: an unsharp mask with this threshold leaves the centre"""
    a = trap3_picture()
    return int(a[4, 4]) - int(pm.gaussian_blur(a, TRAP3_RADIUS)[4, 4])


def chain_picture():
    return smooth_picture(161, 97, 3, 7)
