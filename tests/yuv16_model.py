"""The model of 10-bit video in the ragged call (sjpeg_hip.h, "10-bit video"): the contract in Python integers over numpy
uint16 planes.  The cells and weights are those of the resize model (tests/sheet_model.py: _span, _turn, places); what
follows the made 8-bit planes is tests/yuv_colour_model.py and the sheet model's placement, as they are."""
import numpy as np

import sheet_model as sm
import yuv_colour_model as cm


def own_size(words, shift):
    """the formula at the frame's own size, on an array of words: min(255, (x + 2^(s-1)) >> s)"""
    x = np.asarray(words).astype(np.int64)
    half = (1 << shift) >> 1
    return np.minimum(255, (x + half) >> shift).astype(np.uint8)


def round_deep(S, A, shift):
    """byte = min(255, floor((2 S + A 2^s) / (A 2^(s+1)))), Python integers"""
    return min(255, (2 * S + (A << shift)) // (A << (shift + 1)))


def area16(plane, w2, h2, shift):
    """the made uint8 plane [h2, w2] of a uint16 plane [H, W]: the exact weighted sum of the WORDS of every cell,
    rounded once"""
    plane = np.asarray(plane)
    assert plane.dtype == np.uint16 and plane.ndim == 2
    H, W = plane.shape
    rows = plane.tolist()
    xs, ys = [sm._span(i, W, w2) for i in range(w2)], [sm._span(j, H, h2) for j in range(h2)]
    hsum = [[sum(w * row[x] for x, w in xs[i]) for i in range(w2)] for row in rows]
    out = np.empty((h2, w2), np.uint8)
    for j in range(h2):
        for i in range(w2):
            out[j, i] = round_deep(sum(w * hsum[y][i] for y, w in ys[j]), W * H, shift)
    return out


def narrowed_then_averaged(plane, w2, h2, shift):
    """what the contract is NOT: every sample rounded to a byte first, the bytes averaged after (the torch pre-pass)"""
    return sm._area(own_size(plane, shift), w2, h2)


def chroma_size(kind, w, h):
    return (w, h) if kind == "yuv444" else ((w + 1) // 2, (h + 1) // 2)


def made_planes(yuv, kind, size, shift, o=1, colour=None):
    """the three made planes of a frame (y, u, v) of uint16 planes, kind "nv12", "nv21", "yuv420" or "yuv444": each
    resized as a picture of its own, turned, then converted from colour = (matrix, range) (None: not at all)"""
    cw, ch = chroma_size(kind, *size)
    made = [area16(yuv[0], size[0], size[1], shift), area16(yuv[1], cw, ch, shift), area16(yuv[2], cw, ch, shift)]
    made = [np.ascontiguousarray(sm._turn(p, o)) for p in made]
    if colour is not None:
        made = list(cm.convert_planes(*made, *colour))
    return made


def sheets(kind, frames, cols, rows, cell, gutter, margin, background, sizes, orientations, shift, colours=None):
    """the sheets (Y, U, V) of deep frames: the made planes above stored at the sheet model's places; the background
    stays as given"""
    half = kind in sm.YUV420_LIKE
    SW, SH = sm.sheet_size(cols, rows, cell, gutter, margin)
    where = sm.places(kind, cols, rows, cell, gutter, margin, sizes, orientations)
    dims = [(SW, SH)] + [(SW // 2, SH // 2) if half else (SW, SH)] * 2
    out = [[np.full((h, w), background[c], np.uint8) for c, (w, h) in enumerate(dims)] for _ in range(where[-1][0] + 1)]
    for f, (fr, size, o, (s, x0, y0, uw, uh)) in enumerate(zip(frames, sizes, orientations, where)):
        made = made_planes(fr, kind, size, shift, o, None if colours is None else colours[f])
        for c in range(3):
            px, py = (x0 // 2, y0 // 2) if half and c > 0 else (x0, y0)
            out[s][c][py:py + made[c].shape[0], px:px + made[c].shape[1]] = made[c]
    return [tuple(s) for s in out], where
