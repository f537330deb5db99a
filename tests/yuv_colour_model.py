"""The model of the video colour conversion (sjpeg_hip.h, "video colour converted inside the ragged call"): the contract
restated in numpy integers, used by every test of the feature.  The tables are written out as the header writes them;
derive_matrix() is the float64 chain behind them, for the test that holds the tables to it."""
import numpy as np

BT601, BT709 = 0, 1
FULL, LIMITED = 0, 1
SOURCES = [(BT601, FULL), (BT601, LIMITED), (BT709, LIMITED), (BT709, FULL)]
NAMES = {(BT601, FULL): "bt601-full", (BT601, LIMITED): "bt601-limited", (BT709, LIMITED): "bt709-limited", (BT709, FULL): "bt709-full"}

# (y0, k): Q14, rows Y, U, V of the output, columns Y, U, V of the source
TABLES = {
    (BT601, FULL): (0, ((16384, 0, 0), (0, 16384, 0), (0, 0, 16384))),
    (BT601, LIMITED): (16, ((19077, 0, 0), (0, 18651, 0), (0, 0, 18651))),
    (BT709, LIMITED): (16, ((19077, 1895, 3657), (0, 18462, -2064), (0, -1351, 18342))),
    (BT709, FULL): (0, ((16384, 1664, 3213), (0, 16218, -1813), (0, -1187, 16112))),
}
KR_KB = {BT601: (0.299, 0.114), BT709: (0.2126, 0.0722)}


def _to_rgb(kr, kb):
    """Y'CbCr (Cb, Cr centred, full range) -> R'G'B' with the given Kr, Kb"""
    kg = 1.0 - kr - kb
    return np.array([[1.0, 0.0, 2.0 * (1.0 - kr)],
                     [1.0, -2.0 * kb * (1.0 - kb) / kg, -2.0 * kr * (1.0 - kr) / kg],
                     [1.0, 2.0 * (1.0 - kb), 0.0]], np.float64)


def _from_rgb(kr, kb):
    """R'G'B' -> Y'CbCr (full range) with the given Kr, Kb"""
    kg = 1.0 - kr - kb
    y = np.array([kr, kg, kb], np.float64)
    return np.stack([y, (np.array([0.0, 0.0, 1.0]) - y) / (2.0 * (1.0 - kb)), (np.array([1.0, 0.0, 0.0]) - y) / (2.0 * (1.0 - kr))])


def derive_matrix(matrix, rng):
    """M of the header: source Y'CbCr -> R'G'B' by the source's Kr, Kb, R'G'B' -> full-range BT.601 YCbCr, the columns
    scaled by 255/219 (Y) and 255/224 (chroma) for a limited-range source; float64"""
    m = _from_rgb(*KR_KB[BT601]) @ _to_rgb(*KR_KB[matrix])
    if rng == LIMITED:
        m = m * np.array([255.0 / 219.0, 255.0 / 224.0, 255.0 / 224.0])[None, :]
    return m


def convert_samples(y, u, v, matrix, rng):
    """The contract on arrays of samples that belong together (y's chroma is u, v): integer arrays of one shape in,
    (Y', U', V') uint8 out.  floor is numpy's >> on int64: a true floor."""
    y0, k = TABLES[(matrix, rng)]
    y = np.asarray(y, np.int64)
    uu = np.asarray(u, np.int64) - 128
    vv = np.asarray(v, np.int64) - 128
    yo = np.clip((k[0][0] * (y - y0) + k[0][1] * uu + k[0][2] * vv + 8192) >> 14, 0, 255)
    uo = np.clip(128 + ((k[1][1] * uu + k[1][2] * vv + 8192) >> 14), 0, 255)
    vo = np.clip(128 + ((k[2][1] * uu + k[2][2] * vv + 8192) >> 14), 0, 255)
    return yo.astype(np.uint8), uo.astype(np.uint8), vo.astype(np.uint8)


def convert_planes(y, u, v, matrix, rng):
    """P' of the upright planar picture P = (y [uh, uw], u and v [ch, cw]): luma (x, y) takes the UNCONVERTED chroma at
    (x / s, y / s), s = 2 where the chroma planes are the halved ones and 1 where they have the luma's size"""
    y, u, v = (np.asarray(p, np.uint8) for p in (y, u, v))
    if (matrix, rng) == (BT601, FULL):
        return y.copy(), u.copy(), v.copy()
    uh, uw = y.shape
    s = 1 if u.shape == y.shape else 2
    assert u.shape == v.shape == ((uh + s - 1) // s, (uw + s - 1) // s), (y.shape, u.shape, v.shape)
    yi, xi = np.arange(uh)[:, None] // s, np.arange(uw)[None, :] // s
    yo, _, _ = convert_samples(y, u[yi, xi], v[yi, xi], matrix, rng)
    _, uo, vo = convert_samples(np.zeros_like(u), u, v, matrix, rng)
    return yo, uo, vo
