"""Every source format through the uniform and the ragged entry, on the GPU: for each SJPEG_HIP_SRC_* value 0..20 a
picture of 17 x 9 and one of 40 x 24 (clipped MCUs in both directions, the chroma-width rounding), rows stored top-down
and bottom-up (a negative row stride), at every sampling the format takes, method 0.  The samples are whole numbers
0..255 -- exact in half and bfloat16 -- and the float formats go through scale 1, bias 0, so no rounding is involved: the
JPEG must be, byte for byte, the CPU oracle's for the equivalent uint8 picture (RGB for the RGB-like formats, the plane
set for the YUV and gray ones).  The RGB-like formats also go through the ragged riskiness, whose sums must be those of
the uint8 SRC_RGB picture."""
import os

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import synth

pytestmark = pytest.mark.gpu

SIZES = [(17, 9), (40, 24)]
FLOATS = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
# format -> (what it is made of, element dtype or None for bytes); written out here, not read from the binding's table
KINDS = {sj.SRC_RGB: ("rgb", None), sj.SRC_BGRA: ("bgra", None), sj.SRC_RGBA: ("rgba", None), sj.SRC_GRAY: ("gray", None),
         sj.SRC_YUV444: ("yuv444", None), sj.SRC_YUV420: ("yuv420", None), sj.SRC_NV12: ("nv12", None),
         sj.SRC_NV21: ("nv21", None), sj.SRC_RGB_PLANAR: ("planar", None),
         sj.SRC_RGB_PLANAR_F32: ("planar", "float32"), sj.SRC_RGB_PLANAR_F16: ("planar", "float16"),
         sj.SRC_RGB_PLANAR_BF16: ("planar", "bfloat16"),
         sj.SRC_RGB_F32: ("rgb", "float32"), sj.SRC_RGB_F16: ("rgb", "float16"), sj.SRC_RGB_BF16: ("rgb", "bfloat16"),
         sj.SRC_RGBA_F32: ("rgba", "float32"), sj.SRC_RGBA_F16: ("rgba", "float16"), sj.SRC_RGBA_BF16: ("rgba", "bfloat16"),
         sj.SRC_GRAY_F32: ("gray", "float32"), sj.SRC_GRAY_F16: ("gray", "float16"), sj.SRC_GRAY_BF16: ("gray", "bfloat16")}
RGB_LIKE = ("rgb", "bgra", "rgba", "planar")
IMPLIED = {"gray": sj.YUV_400, "yuv444": sj.YUV_444, "yuv420": sj.YUV_420, "nv12": sj.YUV_420, "nv21": sj.YUV_420}


@pytest.fixture(scope="module")
def engine():
    eng = sj.Engine(0)
    eng.set_pixel_transform(1.0, 0.0)
    return eng


@pytest.fixture(scope="module")
def pictures():
    """Per size two uint8 pictures [H, W, 3] (the two frames of the uniform call; the first of each size makes the ragged
    batch) and two chroma planes [ch, cw] each for the 4:2:0 layouts; never written to."""
    out = []
    for k, (w, h) in enumerate(SIZES):
        cw, ch = (w + 1) // 2, (h + 1) // 2
        rgb = [synth.g_struct(w, h, 8100 + k), synth.g_noise(w, h, 8200 + k)]
        sub = [[synth.g_noise(cw, ch, 8300 + 2 * k + j)[:, :, c].copy() for c in (0, 1)] for j in range(2)]
        out.append((rgb, sub))
    return out


_wanted = {}


def _want(oracle, kind, pic, sub, mode, quant):
    """the oracle's JPEG of the uint8 picture a layout stands for; computed once for all formats and signs"""
    key = (kind if kind not in RGB_LIKE else "rgb", pic.tobytes(), pic.shape, mode)
    if key not in _wanted:
        h, w = pic.shape[:2]
        if kind in RGB_LIKE:
            fmt, planes = sj.SRC_RGB, [pic.reshape(h, -1)]
        else:
            fmt = {"gray": sj.SRC_GRAY, "yuv444": sj.SRC_YUV444, "yuv420": sj.SRC_YUV420, "nv12": sj.SRC_NV12, "nv21": sj.SRC_NV21}[kind]
            planes = _planes(kind, pic, sub)
        _wanted[key] = oracle.encode_src(fmt, planes, w, h, quant, yuv_mode=mode, method=0)
    return _wanted[key]


def _planes(kind, pic, sub):
    """the host planes [rows, elements] of a layout, as uint8 values"""
    h, w = pic.shape[:2]
    r, g, b = (np.ascontiguousarray(pic[:, :, c]) for c in range(3))
    a = np.full((h, w), 0x5a, np.uint8)
    if kind == "rgb":
        return [pic.reshape(h, 3 * w)]
    if kind == "bgra":
        return [np.stack([b, g, r, a], 2).reshape(h, 4 * w)]
    if kind == "rgba":
        return [np.stack([r, g, b, a], 2).reshape(h, 4 * w)]
    if kind == "gray":
        return [g]
    if kind in ("planar", "yuv444"):
        return [r, g, b]
    if kind == "yuv420":
        return [r, sub[0], sub[1]]
    uv = sub if kind == "nv12" else sub[::-1]
    return [r, np.stack(uv, 2).reshape(sub[0].shape[0], -1)]


def _device(kind, dtype, frames, sign):
    """The planes of `frames` (one uniform batch: [(pic, sub), ...] of one size) in device memory, rows padded and, with
    sign -1, stored bottom-up.  Returns (keep-alive tensors, per plane (address of row 0 of frame 0, row stride, frame
    stride) in bytes).  The fourth element of a float RGBA pixel and all padding are NaN (0xEE for bytes)."""
    host = [_planes(kind, pic, sub) for pic, sub in frames]
    keep, where = [], []
    for i in range(len(host[0])):
        rows, elems = host[0][i].shape
        tdt = torch.uint8 if dtype is None else FLOATS[dtype]
        buf = torch.full((len(frames), rows + 1, elems + 5), 0xEE if dtype is None else float("nan"), dtype=tdt)
        for f, planes in enumerate(host):
            p = torch.from_numpy(planes[i][::-1].copy() if sign < 0 else planes[i]).to(tdt)
            if dtype is not None and kind == "rgba":
                p.view(rows, -1, 4)[:, :, 3] = float("nan")
            buf[f, :rows, :elems] = p
        dev = buf.cuda()
        esz = dev.element_size()
        pitch = dev.stride(1) * esz
        keep.append(dev)
        where.append((dev.data_ptr() + (rows - 1) * pitch, -pitch, dev.stride(0) * esz) if sign < 0 else
                     (dev.data_ptr(), pitch, dev.stride(0) * esz))
    return keep, where


def _modes(kind):
    return (IMPLIED[kind],) if kind in IMPLIED else (sj.YUV_420, sj.YUV_444, sj.YUV_400)


@pytest.mark.parametrize("sign", [1, -1], ids=["top-down", "bottom-up"])
@pytest.mark.parametrize("fmt", sorted(KINDS), ids=lambda f: "fmt%d" % f)
def test_uniform_and_ragged_entries(engine, oracle, pictures, fmt, sign):
    kind, dtype = KINDS[fmt]
    tables, qm = sj.make_tables(quality=75.0)
    placed = [_device(kind, dtype, list(zip(rgb, sub)), sign) for rgb, sub in pictures]
    for mode in _modes(kind):
        # the uniform entry: the two frames of each size
        for (w, h), (rgb, sub), (_, where) in zip(SIZES, pictures, placed):
            src = sj.Source()
            src.format = fmt
            for i, (at, row, frame) in enumerate(where):
                src.plane[i], src.row_stride[i], src.frame_stride[i] = at, row, frame
            out, sizes = engine.encode_source(src, 2, w, h, tables, sj.make_header(w, h, mode, qm), mode)
            torch.cuda.synchronize()
            host, sz = out.cpu().numpy(), sizes.cpu().numpy()
            for f in range(2):
                assert host[f, :int(sz[f])].tobytes() == _want(oracle, kind, rgb[f], sub[f], mode, qm), ("uniform", mode, (w, h), f)
        # the ragged entry: the first picture of each size in one call
        planes = [[(at, row) for at, row, _ in where] for _, where in placed]
        out, sizes, offs = engine.encode_ragged(fmt, planes, SIZES, mode, tables, [sj.make_header(w, h, mode, qm) for w, h in SIZES])
        torch.cuda.synchronize()
        host, sz = out.cpu().numpy(), sizes.cpu().numpy()
        for k, (rgb, sub) in enumerate(pictures):
            assert host[offs[k]:offs[k] + int(sz[k])].tobytes() == _want(oracle, kind, rgb[0], sub[0], mode, qm), ("ragged", mode, SIZES[k])


@pytest.fixture(scope="module")
def risk_table():
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def rgb_sums(engine, pictures, risk_table):
    """the riskiness sums of the uint8 SRC_RGB pictures (the first of each size), once"""
    devs = [torch.from_numpy(rgb[0].reshape(rgb[0].shape[0], -1)).cuda() for rgb, _ in pictures]
    sums = engine.riskiness_ragged(sj.SRC_RGB, [[d] for d in devs], SIZES, table=risk_table)
    torch.cuda.synchronize()
    return sums.cpu().numpy()


@pytest.mark.parametrize("sign", [1, -1], ids=["top-down", "bottom-up"])
@pytest.mark.parametrize("fmt", sorted(f for f, (kind, _) in KINDS.items() if kind in RGB_LIKE), ids=lambda f: "fmt%d" % f)
def test_riskiness_sums_are_those_of_the_rgb_picture(engine, pictures, risk_table, rgb_sums, fmt, sign):
    kind, dtype = KINDS[fmt]
    placed = [_device(kind, dtype, [(rgb[0], sub[0])], sign) for rgb, sub in pictures]
    planes = [[(at, row) for at, row, _ in where] for _, where in placed]
    sums = engine.riskiness_ragged(fmt, planes, SIZES, table=risk_table)
    torch.cuda.synchronize()
    assert (sums.cpu().numpy() == rgb_sums).all()
