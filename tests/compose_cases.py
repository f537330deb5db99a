"""The cases tests/golden/compose_pillow.npz records Pillow's answers for, and their pictures -- integers of the
position alone (pillow_filter_cases.picture), so that the fixture holds only what Pillow made.  Shared by
tests/golden/make_compose_pillow.py and the tests."""
import numpy as np

import pillow_filter_cases as pc

# (w, h, box, centering): ImageOps.contain's size and ImageOps.pad's place.  The first four are the half-to-even cases
# and the worked example; both branches of the ratio test, the equal ratio, enlarging, and centerings outside 0..1
SIZES = [(3, 2, (5, 5), (0.5, 0.5)), (2, 3, (6, 5), (0.5, 0.5)), (5, 5, (6, 1), (0.5, 0.5)), (1920, 1080, (256, 256), (0.5, 0.5)),
         (4, 2, (8, 4), (0.5, 0.5)), (90, 50, (40, 40), (0.5, 0.5)), (50, 90, (40, 40), (0.5, 0.5)), (7, 5, (50, 20), (0.25, 0.9)),
         (5, 7, (20, 50), (0.9, 0.25)), (640, 480, (100, 100), (0.0, 0.0)), (480, 640, (100, 100), (1.0, 1.0)), (33, 47, (64, 64), (-2.0, 0.5)),
         (47, 33, (64, 64), (0.5, 3.0)), (30, 100, (9, 9), (0.5, 0.5)), (100, 30, (9, 9), (0.5, 0.5)), (17, 9, (17, 9), (0.5, 0.5))]
# a target side that rounds to 0: Pillow raises
SIZES_REFUSED = [(1000, 1, (10, 10)), (3, 1000, (9, 9))]

# (mode, (w, h), [(overlay index, (ox, oy)), ...]): pastes onto picture(mode, (w, h), 100 + k), in list order, at
# top-left positions on the picture
PASTES = [("RGB", (12, 10), [(0, (2, 2)), (1, (4, 3))]), ("RGB", (12, 10), [(1, (4, 3)), (0, (2, 2))]),        # overlapping, both orders
          ("RGB", (12, 10), [(2, (-2, 3))]), ("RGB", (12, 10), [(2, (10, 3))]), ("RGB", (12, 10), [(2, (3, -1))]),   # over each edge
          ("RGB", (12, 10), [(2, (3, 8))]), ("RGB", (12, 10), [(2, (50, 50))]), ("RGB", (12, 10), [(2, (-20, 0))]),  # ... and wholly outside
          ("L", (12, 10), [(2, (1, 1))]), ("L", (12, 10), [(0, (2, 2)), (1, (4, 3))]), ("L", (12, 10), [(2, (-2, -1)), (3, (5, 5))]),
          ("RGB", (12, 10), [(4, (-3, -2))]), ("RGB", (5, 3), [(3, (1, 0))])]                                  # the whole picture covered
CHAIN_SOURCES = [(90, 50), (50, 90)]
CHAIN_BOX = (40, 40)
CHAIN_COLOUR = (250, 240, 20)
CHAIN_LOGO_AT = (27, 29)
# (mode, (w, h), size, colour, centering): ImageOps.pad(im, size, BICUBIC, color=colour, centering=centering)
PADS = [("RGB", (90, 50), (40, 40), (250, 240, 20), (0.5, 0.5)), ("RGB", (50, 90), (40, 40), (1, 2, 3), (0.5, 0.5)),
        ("RGB", (31, 17), (23, 23), (9, 99, 199), (0.2, 0.8)), ("RGB", (17, 31), (23, 23), (9, 99, 199), (0.8, 0.2)),
        ("L", (31, 17), (23, 23), (77, 77, 77), (0.5, 0.5)), ("RGB", (9, 5), (30, 31), (255, 0, 128), (0.5, 0.5)),
        ("RGB", (20, 10), (10, 5), (0, 0, 0), (0.5, 0.5))]


def overlay(k):
    """the overlays of PASTES, RGBA uint8: 0 half white, 1 half black, 2 noise in every channel, 3 noise with alpha 255 and
    0 in stripes, 4 noise larger than the pictures"""
    if k in (0, 1):
        a = np.zeros((5, 6, 4), np.uint8)
        a[..., :3] = 255 if k == 0 else 0
        a[..., 3] = 128
        return a
    size = {2: (4, 3), 3: (3, 3), 4: (20, 15)}[k]
    a = np.ascontiguousarray(np.concatenate([pc.picture("RGB", size, 200 + k), pc.picture("L", size, 300 + k)[..., None]], axis=2))
    if k == 3:
        a[:, 0, 3], a[:, 1, 3] = 0, 255
    return a


def logo():
    """the chain's logo: 10 x 8, a ramp of alpha that reaches both 0 and 255"""
    a = overlay(4)[:8, :10].copy()
    a[..., 3] = np.linspace(0, 255, 80).astype(np.uint8).reshape(8, 10)
    return a


def base(mode, size, k):
    return pc.picture(mode, size, 100 + k)


def chain_source(k):
    w, h = CHAIN_SOURCES[k]
    return pc.smooth_picture(w, h, 3, 40 + k)
