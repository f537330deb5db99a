"""The model of the contact sheets (sjpeg_hip.h, "contact sheets"), in Python integers and numpy indexing: _area() and
_turn() as tests/test_yuv_resize.py states them, the fit, the placement and the sheet's bytes.  tests/test_sheet_host.py
holds the formulae of the library to it without a device, tests/test_sheet.py the kernel's bytes on one."""
import numpy as np

YUV420_LIKE = ("nv12", "nv21", "yuv420")       # the kinds whose chroma is half the luma's; the others: "rgb", "gray", "yuv444"


def _span(i, n, m):
    """the source samples that output sample i of m covers among n, with their weights: sjpeg_hip.h's formula"""
    out = []
    x = i * n // m
    while x < n and x * m < (i + 1) * n:
        w = min((x + 1) * m, (i + 1) * n) - max(x * m, i * n)
        if w > 0:
            out.append((x, w))
        x += 1
    assert sum(w for _, w in out) == n
    return out


def _area(plane, w2, h2):
    """the exact area average of a uint8 plane [H, W], in Python integers: round half up"""
    H, W = plane.shape
    rows = plane.tolist()
    xs, ys = [_span(i, W, w2) for i in range(w2)], [_span(j, H, h2) for j in range(h2)]
    hsum = [[sum(w * row[x] for x, w in xs[i]) for i in range(w2)] for row in rows]
    out = np.empty((h2, w2), np.uint8)
    for j in range(h2):
        for i in range(w2):
            S = sum(w * hsum[y][i] for y, w in ys[j])
            out[j, i] = (2 * S + W * H) // (2 * W * H)
    return out


def _turn(R, o):
    """sjpeg_hip.h's table on a plane [h, w]: U(x, y) = R(sx, sy)"""
    return {1: R, 2: R[:, ::-1], 3: R[::-1, ::-1], 4: R[::-1], 5: R.T, 6: R[::-1].T, 7: R[::-1, ::-1].T, 8: R[:, ::-1].T}[o]


def fit(W, H, bw, bh):
    """sjpeg_hip_fit_size"""
    if W <= bw and H <= bh:
        return W, H
    if W * bh >= H * bw:
        return bw, max(1, (H * bw + W // 2) // W)
    return max(1, (W * bh + H // 2) // H), bh


def sheet_size(cols, rows, cell, gutter, margin):
    return (2 * margin + cols * cell[0] + (cols - 1) * gutter, 2 * margin + rows * cell[1] + (rows - 1) * gutter)


def fitted_sizes(dims, cell, orientations):
    """sizes == NULL: every frame fitted into its cell, the box turned with the frame"""
    return [fit(w, h, *((cell[1], cell[0]) if o >= 5 else cell)) for (w, h), o in zip(dims, orientations)]


def places(kind, cols, rows, cell, gutter, margin, sizes, orientations):
    """[(sheet, x0, y0, uw, uh)] of thumbnails of sizes[f] (stored orientation)"""
    out = []
    for f, ((w, h), o) in enumerate(zip(sizes, orientations)):
        uw, uh = (h, w) if o >= 5 else (w, h)
        assert uw <= cell[0] and uh <= cell[1]
        s, k = divmod(f, cols * rows)
        j, i = divmod(k, cols)
        ex, ey = (cell[0] - uw) // 2, (cell[1] - uh) // 2
        if kind in YUV420_LIKE:
            ex, ey = ex & ~1, ey & ~1
        out.append((s, margin + i * (cell[0] + gutter) + ex, margin + j * (cell[1] + gutter) + ey, uw, uh))
    return out


def rgb_sheets(pictures, cols, rows, cell, gutter, margin, background, sizes, orientations):
    """the sheets [SH, SW, C] of uint8 pictures [H, W, C] (C = 3, or 1 for gray: background[0])"""
    C = pictures[0].shape[2]
    SW, SH = sheet_size(cols, rows, cell, gutter, margin)
    where = places("rgb", cols, rows, cell, gutter, margin, sizes, orientations)
    sheets = np.empty((where[-1][0] + 1, SH, SW, C), np.uint8)
    sheets[...] = np.asarray(background[:C], np.uint8)
    for pic, (w, h), o, (s, x0, y0, uw, uh) in zip(pictures, sizes, orientations, where):
        for c in range(C):
            sheets[s, y0:y0 + uh, x0:x0 + uw, c] = _turn(_area(np.ascontiguousarray(pic[:, :, c]), w, h), o)
    return list(sheets), where


def yuv_sheets(kind, frames, cols, rows, cell, gutter, margin, background, sizes, orientations):
    """the sheets (Y, U, V) of frames (y, u, v) of uint8 planes: every plane resized and turned as a picture of its own,
    chroma at half the luma's place for the 4:2:0 kinds"""
    half = kind in YUV420_LIKE
    SW, SH = sheet_size(cols, rows, cell, gutter, margin)
    where = places(kind, cols, rows, cell, gutter, margin, sizes, orientations)
    if half:
        assert SW % 2 == 0 and SH % 2 == 0
    dims = [(SW, SH)] + [(SW // 2, SH // 2) if half else (SW, SH)] * 2
    sheets = [[np.full((h, w), background[c], np.uint8) for c, (w, h) in enumerate(dims)] for _ in range(where[-1][0] + 1)]
    for fr, (w, h), o, (s, x0, y0, uw, uh) in zip(frames, sizes, orientations, where):
        for c in range(3):
            pw, ph = ((w + 1) // 2, (h + 1) // 2) if half and c > 0 else (w, h)
            made = _turn(_area(fr[c], pw, ph), o)
            px, py = (x0 // 2, y0 // 2) if half and c > 0 else (x0, y0)
            assert px + made.shape[1] <= dims[c][0] and py + made.shape[0] <= dims[c][1]
            sheets[s][c][py:py + made.shape[0], px:px + made.shape[1]] = made
    return [tuple(s) for s in sheets], where
