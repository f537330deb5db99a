"""The pictures and parameters that pin SJPEG_YUV_SHARP, SJPEG_YUV_AUTO, SjpegRiskiness and SjpegCompress to the real
reference: one list, walked by the CPU tests (oracle against reference, tests/test_oracle.py) and by the GPU tests
(product against reference, tests/test_reference_sharp_auto.py), so that both make byte-identical calls of the
reference and find its recorded answers (tests/golden/reference_answers.json) again.  No pytest in here.

The ref_* functions below are THE calls of the reference: positional / keyword exactly as written, because
reference_answers.call_key hashes names and order.

Sizes: one sample, one row pair, an odd last column or row, one pixel either side of an MCU -- the smallest shapes at
which the sharp sweeps and the riskiness windows can go wrong -- then random ones below 140 x 110.  Kinds: content whose
riskiness verdicts cover 4:2:0, sharp, 4:4:4 and 4:0:0 (test_live_riskiness asserts at least 10 pictures of each)."""
import collections

import numpy as np

from oracle import synth

SEED = 5
N_PICTURES = 260
FIXED_SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 17), (17, 1), (15, 15), (16, 16), (17, 17), (31, 33), (33, 31)]
QUALITIES = (30, 75, 95)
METHODS = (0, 4, 7)
KINDS = ("struct", "noise", "primaries", "gray", "near-gray", "red-blue")
# g_struct at the shapes of test_sharp_yuv_wide_and_1080p, where the sharp kernel goes in strips across the width
WIDE_SIZES = [(4099, 37), (5, 700), (1920, 1080)]
WIDE_SEED, WIDE_Q, WIDE_METHOD = 77, 80.0, 0
N_SEARCH = 80
MIN_PER_VERDICT = 10

Picture = collections.namedtuple("Picture", "img w h kind q method")
Search = collections.namedtuple("Search", "img w h q target_mode target passes tolerance trellis")


def _content(rng, w, h):
    u = rng.rand()
    if u < 0.3:
        return "struct", synth.g_struct(w, h, int(rng.randint(1 << 30)))
    if u < 0.55:
        return "noise", rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if u < 0.7:
        return "primaries", (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    if u < 0.8:
        return "gray", np.repeat(rng.randint(0, 256, (h, w, 1)), 3, 2).astype(np.uint8)
    if u < 0.9:
        g = rng.randint(0, 256, (h, w, 1)) + rng.randint(-3, 4, (h, w, 3))
        return "near-gray", np.clip(g, 0, 255).astype(np.uint8)
    img = np.zeros((h, w, 3), np.uint8)
    img[:, 0::2, 0] = 255                      # columns alternating pure red and pure blue
    img[:, 1::2, 2] = 255
    return "red-blue", img


_made = {}


def _all():
    """(pictures, search cases), every draw from ONE np.random.RandomState(SEED), in this order; made once and shared
    (the arrays are read-only)."""
    if not _made:
        rng = np.random.RandomState(SEED)
        pictures = []
        for k in range(N_PICTURES):
            w, h = FIXED_SIZES[k] if k < len(FIXED_SIZES) else (int(rng.randint(1, 140)), int(rng.randint(1, 110)))
            kind, img = _content(rng, w, h)
            img.setflags(write=False)
            pictures.append(Picture(img, w, h, kind, float(rng.choice(QUALITIES)), int(rng.choice(METHODS))))
        searches = []
        for _ in range(N_SEARCH):
            w, h = int(rng.randint(1, 150)), int(rng.randint(1, 110))
            img = synth.g_struct(w, h, int(rng.randint(1 << 30))) if rng.rand() < 0.6 else \
                rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
            img.setflags(write=False)
            q = float(rng.choice([20, 60, 85]))
            tm = int(rng.randint(1, 3))
            target = float(rng.choice([800, 2500, 7000, 20000])) if tm == 1 else float(rng.choice([28, 35, 41, 48]))
            passes = int(rng.choice([2, 3, 5, 10]))
            tol = float(rng.choice([0.1, 1.0, 5.0]))
            searches.append(Search(img, w, h, q, tm, target, passes, tol, bool(rng.randint(2))))
        _made["pictures"], _made["searches"] = pictures, searches
    return _made["pictures"], _made["searches"]


def pictures():
    """The 260 pictures: the twelve fixed sizes first."""
    return _all()[0]


def q100_pictures():
    """A fixed subset of 40 pictures -- the twelve fixed sizes and every ninth of the others -- at quality 100, method 0:
    every quantizer is 1, so a one-level difference in any Y, U or V sample of the sharp conversion shows in the bytes."""
    ps = pictures()
    idx = list(range(len(FIXED_SIZES))) + list(range(len(FIXED_SIZES), N_PICTURES, 9))
    assert len(idx) == 40
    return [ps[k]._replace(q=100.0, method=0) for k in idx]


def wide_pictures():
    if "wide" not in _made:
        out = []
        for (w, h) in WIDE_SIZES:
            img = synth.g_struct(w, h, WIDE_SEED)
            img.setflags(write=False)
            out.append(Picture(img, w, h, "struct", WIDE_Q, WIDE_METHOD))
        _made["wide"] = out
    return _made["wide"]


def search_cases():
    """80 pictures drawn like test_live_search_with_trellis (methods 4, or 7 with the trellis); each runs with
    SEARCH_YUV_MODES: sharp and auto."""
    return _all()[1]


SEARCH_YUV_MODES = (2, 0)


def even_pictures(n=10):
    """The first n pictures whose sides are both even (the 2x2 replicate of each reduces back to it exactly)."""
    out = [p for p in pictures() if p.w % 2 == 0 and p.h % 2 == 0][:n]
    assert len(out) == n
    return out


def what(p):
    return (p.w, p.h, p.kind, p.q, p.method) if isinstance(p, Picture) else tuple(p[1:])


# ---- the calls of the reference (oracle.refso.Ref's interface; tests/reference_answers.py replays them)

def ref_sharp(reference, p):
    return reference.encode(p.img, p.q, p.method, 2)


def ref_auto(reference, p):
    return reference.encode(p.img, p.q, p.method, 0)


def ref_riskiness(reference, p):
    return reference.riskiness(p.img)


def ref_compress(reference, p):
    return reference.compress(p.img, 75.0)


def ref_search(reference, s, yuv_mode):
    return reference.encode_search(s.img, s.q, yuv_mode, True, True, s.target_mode, s.target, s.passes, s.tolerance,
                                   0.0, 100.0, trellis=s.trellis)
