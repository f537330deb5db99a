"""The float pixel transform on the GPU, bit for bit against the exact model of tests/float_contract.py:
    t  = fmaf((float)x, scale[c], bias[c])           ONE fp32 rounding
    u8 = isnan(t) ? 0 : rint(min(max(t, 0), 255))    half to even; +-inf saturate
on every bit pattern of float16 and bfloat16 and 65 536 chosen ones of float32, under transforms made so that each near
miss of the contract -- two roundings, flushed subnormals, ties away, truncation, a NaN that is not 0 -- changes bytes
(tests/test_float_contract_host.py asserts how many).  Part A reads the scalar helper's bytes back (elem_load_u8 through
the reduce kernel at factor 1); part B sees the scan kernels' three loaders (elem_load8, elem_load8x3<3>, <4>) through
JPEGs in which every byte shows; part C takes the other kernels that convert: riskiness, sharp YUV, box sums.
Every comparison is exact.  A failure names the competing model that explains it, if one does."""
import os

import numpy as np
import pytest
import torch

import float_contract as fc
import sjpeg_amd as sj
from test_reduce import _box

pytestmark = pytest.mark.gpu

DT = list(fc.DTYPES)
NAMES = [n for n, _ in fc.transforms(fc.F16)]
LAYOUTS = ("planar", "rgb", "rgba")


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.fixture(scope="module")
def risk_table():
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        tab = f.read()
    sj.set_riskiness_table(tab)
    return tab


def _device(t, layout, off=1, pad=2):
    """The CUDA copy of a host [3, H, W] (gray: [1, H, W]) tensor in `layout`, as the logical channel-first view the
    layout="chw" calls take: cut out of rows off + W + pad pixels wide at pixel `off`, so that addresses are aligned to
    the element only; the padding and the fourth element of an "rgba" pixel are NaN."""
    c, h, w = t.shape
    nan = float("nan")
    if layout in ("planar", "gray"):
        buf = torch.full((c, h, off + w + pad), nan, dtype=t.dtype)
        buf[:, :, off:off + w] = t
        return buf.cuda()[:, :, off:off + w]
    step = 3 if layout == "rgb" else 4
    buf = torch.full((h, off + w + pad, step), nan, dtype=t.dtype)
    buf[:, off:off + w, :3] = t.permute(1, 2, 0)
    return buf.cuda()[:, off:off + w, :3].permute(2, 0, 1)


def _verdict(dtype, name, channels, t, got, want):
    """the message of a failed comparison of bytes: per channel, through float_contract.explain"""
    scale, bias = fc.transform(dtype, name)
    lines = [fc.explain(dtype, scale[c], bias[c], t.reshape(-1), got[k].reshape(-1), want[k].reshape(-1))
             for k, c in enumerate(channels) if not np.array_equal(got[k], want[k])]
    return f"transform {name!r}: " + " | ".join(lines)


def _who(check):
    """the competing models under which check(model name) holds: what explains a failure that has no bytes to show"""
    named = [m for m in fc.MODELS if check(m)]
    return "explained by: " + (", ".join(named) if named else "no competing model")


# ---- A. the scalar helper, byte for byte: reduce at factor 1 returns what elem_load_u8 makes of every sample

def _read_back(engine, dtype, name, layout):
    v = fc.values(dtype).reshape(1, 256, 256)
    scale, bias = fc.transform(dtype, name)
    channels = [0] if layout == "gray" else [0, 1, 2]
    dev = _device(v if layout == "gray" else v.expand(3, 256, 256), layout)
    got = sj.reduce_images(sj.FloatPixels([dev], scale, bias), 1, engine=engine, layout="chw")[0]
    torch.cuda.synchronize()
    got = got.cpu().numpy().reshape(len(channels), 256, 256)
    want = fc.bytes3(dtype, name)[channels].reshape(len(channels), 256, 256)
    assert np.array_equal(got, want), _verdict(dtype, name, channels, v, got, want)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", DT, ids=fc.NAMES.get)
def test_scalar_helper_planar(engine, dtype, name):
    _read_back(engine, dtype, name, "planar")


@pytest.mark.parametrize("name", ["cancelling", "lift"])
@pytest.mark.parametrize("layout", ["rgb", "rgba", "gray"])
@pytest.mark.parametrize("dtype", DT, ids=fc.NAMES.get)
def test_scalar_helper_other_layouts(engine, dtype, layout, name):
    _read_back(engine, dtype, name, layout)


# ---- B. the scan kernels' loaders through the stream: a value fills an 8 x 8 block of a 4:4:4 picture at quality 100

_stream_cache = {}


def _gray_rgb(b):
    return np.ascontiguousarray(np.repeat(b[:, :, None], 3, axis=2))


def _block_index(idx, bw, bh, w, h):
    """[h, w] indices: idx (bw * bh of them) laid out one per 8 x 8 block, cut to w x h"""
    return np.repeat(np.repeat(np.asarray(idx).reshape(bh, bw), 8, axis=0), 8, axis=1)[:h, :w]


def _quadrants():
    """the 65 536 values as 256 x 256 blocks, in four pictures of 1024 x 1024: their [1024, 1024] index arrays"""
    grid = _block_index(np.arange(65536), 256, 256, 2048, 2048)
    return [grid[y:y + 1024, x:x + 1024] for y in (0, 1024) for x in (0, 1024)]


def _stream_wants(oracle, dtype, name, c, model=None):
    """the oracle's four streams of the pictures the contract (or a model) makes of the quadrants; cached"""
    key = (dtype, name, c, model)
    if key not in _stream_cache:
        b = fc.bytes3(dtype, name, model)[c]
        _stream_cache[key] = [oracle.encode(_gray_rgb(b[q]), 100.0, sj.YUV_444) for q in _quadrants()]
    return _stream_cache[key]


@pytest.mark.parametrize("name,c", fc.STREAM_TRANSFORMS, ids=[n for n, _ in fc.STREAM_TRANSFORMS])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DT, ids=fc.NAMES.get)
def test_loaders_through_the_stream(engine, oracle, dtype, layout, name, c):
    scale, bias = fc.transform(dtype, name)
    v = fc.values(dtype)
    dev = [_device(v[torch.from_numpy(q)].unsqueeze(0).expand(3, 1024, 1024), layout, k % 2, k) for k, q in enumerate(_quadrants())]
    got = sj.encode_images(sj.FloatPixels(dev, scale[c], bias[c]), 100.0, sj.YUV_444, engine=engine, layout="chw")
    want = _stream_wants(oracle, dtype, name, c)
    assert got == want, (f"{fc.NAMES[dtype]} {layout} transform {name!r} channel {c} (scale {scale[c]!r}, bias {bias[c]!r}): quadrants "
                         f"{[k for k in range(4) if got[k] != want[k]]} differ; " +
                         _who(lambda m: got == _stream_wants(oracle, dtype, name, c, m)))


@pytest.mark.parametrize("dtype,layout", [(fc.F16, "planar"), (fc.BF16, "rgb"), (fc.F32, "rgba")],
                         ids=["f16-planar", "bf16-rgb", "f32-rgba"])
def test_loaders_edge_path_beside_the_inside_path(engine, oracle, dtype, layout):
    """width 8 * 16 + 5, height 8 * 8 + 3: the last block column and row are cut, and the encoder replicates them"""
    name, c = "cancelling", 1
    w, h, bw, bh = 133, 67, 17, 9
    scale, bias = fc.transform(dtype, name)
    grid = _block_index(fc.probe(dtype, name, bw * bh), bw, bh, w, h)
    dev = _device(fc.values(dtype)[torch.from_numpy(grid)].unsqueeze(0).expand(3, h, w), layout, 3, 1)
    got = sj.encode_images(sj.FloatPixels([dev], scale[c], bias[c]), 100.0, sj.YUV_444, engine=engine, layout="chw")[0]

    def want(model=None):
        return oracle.encode(_gray_rgb(fc.bytes3(dtype, name, model)[c][grid]), 100.0, sj.YUV_444)
    assert got == want(), f"{fc.NAMES[dtype]} {layout} {w} x {h}: " + _who(lambda m: got == want(m))


def test_loaders_through_the_uniform_batch(engine, oracle):
    """the same pictures through make_source and Engine.encode_source: two frames of 32 x 32 blocks"""
    dtype, name, c = fc.F16, "cancelling", 1
    n, w, h = 2, 256, 256
    scale, bias = fc.transform(dtype, name)
    grids = [_block_index(idx, 32, 32, w, h) for idx in fc.probe(dtype, name, 2048).reshape(2, 1024)]
    big = torch.full((n, 3, h, w + 5), float("nan"), dtype=dtype)
    for k, g in enumerate(grids):
        big[k, :, :, 3:3 + w] = fc.values(dtype)[torch.from_numpy(g)]
    x = big.cuda()[:, :, :, 3:3 + w]
    src, nf = sj.make_source(sj.SRC_RGB_PLANAR_F16, (x[:, 0], x[:, 1], x[:, 2]))
    assert nf == n
    engine.set_pixel_transform(scale[c], bias[c])
    tables, qm = sj.make_tables(quality=100.0)
    out, sizes = engine.encode_source(src, n, w, h, tables, sj.make_header(w, h, sj.YUV_444, qm), sj.YUV_444)
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    got = [host[k, :int(sz[k])].tobytes() for k in range(n)]

    def want(model=None):
        return [oracle.encode(_gray_rgb(fc.bytes3(dtype, name, model)[c][g]), 100.0, sj.YUV_444) for g in grids]
    assert got == want(), _who(lambda m: got == want(m))


# ---- C. the other kernels that convert, on small pictures tiled from the discriminating samples, per-channel transform

SMALL = [(64, 48), (17, 13)]
BIG = [(96, 80), (200, 36)]              # past the 32 x 32 of sharp_small: the import, strips and export kernels
C_NAME = "cancelling"
C_LAYOUT = {fc.F32: "planar", fc.F16: "rgb", fc.BF16: "rgba"}
_small_cache = {}


def _pictures(dtype):
    """(device pictures, index arrays [H, W]) of the four part-C pictures of a dtype, made once"""
    if dtype not in _small_cache:
        grids = [fc.probe(dtype, C_NAME, w * h).reshape(h, w) for (w, h) in SMALL + BIG]
        dev = [_device(fc.values(dtype)[torch.from_numpy(g)].unsqueeze(0).expand(3, *g.shape), C_LAYOUT[dtype], 1 + k, k)
               for k, g in enumerate(grids)]
        _small_cache[dtype] = (dev, grids)
    return _small_cache[dtype]


def _model_pictures(dtype, model=None):
    """the uint8 pictures [H, W, 3] the contract (or a model) makes of the part-C pictures"""
    b = fc.bytes3(dtype, C_NAME, model)
    return [np.ascontiguousarray(np.stack([b[c][g] for c in range(3)], axis=2)) for g in _pictures(dtype)[1]]


def _fp(dtype):
    return sj.FloatPixels(_pictures(dtype)[0], *fc.transform(dtype, C_NAME))


@pytest.mark.parametrize("dtype", DT, ids=fc.NAMES.get)
def test_riskiness(engine, oracle, risk_table, dtype):
    got = sj.riskiness_images(_fp(dtype), engine=engine, layout="chw")

    def want(model=None):
        return [oracle.riskiness(im, risk_table) for im in _model_pictures(dtype, model)]
    assert got == want(), _who(lambda m: got == want(m))
    # and the three sums themselves: those of the uint8 call on the model's pictures
    planes, dims, _, fmt = sj._chw_planes("test", _pictures(dtype)[0], _fp(dtype))
    a = engine.riskiness_ragged(fmt, planes, dims).cpu().numpy()

    def sums(model=None):
        u8 = [torch.from_numpy(im).cuda() for im in _model_pictures(dtype, model)]
        return engine.riskiness_ragged(sj.SRC_RGB, [[t.reshape(t.shape[0], -1)] for t in u8], dims).cpu().numpy()
    assert np.array_equal(a, sums()), _who(lambda m: np.array_equal(a, sums(m)))


@pytest.mark.parametrize("dtype", DT, ids=fc.NAMES.get)
def test_sharp_yuv_ragged(engine, oracle, dtype):
    planes, dims, _, fmt = sj._chw_planes("test", _pictures(dtype)[0], _fp(dtype))
    engine.set_pixel_transform(*fc.transform(dtype, C_NAME))
    got = engine.sharp_yuv_ragged(fmt, planes, dims)
    torch.cuda.synchronize()
    got = [[p.cpu().numpy() for p in frame] for frame in got]

    def same(model=None):
        return all(np.array_equal(a, np.asarray(b)) for frame, im in zip(got, _model_pictures(dtype, model))
                   for a, b in zip(frame, oracle.sharp_yuv(im)))
    assert same(), _who(same)


@pytest.mark.parametrize("factor", [2, 3])
@pytest.mark.parametrize("dtype", DT, ids=fc.NAMES.get)
def test_box_sums_of_converted_samples(engine, dtype, factor):
    got = sj.reduce_images(_fp(dtype), factor, engine=engine, layout="chw")
    torch.cuda.synchronize()
    got = [p.permute(1, 2, 0).cpu().numpy() for p in got]

    def same(model=None):
        return all(np.array_equal(a, _box(im, factor)) for a, im in zip(got, _model_pictures(dtype, model)))
    assert same(), _who(same)
