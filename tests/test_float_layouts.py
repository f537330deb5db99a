"""Channels-last, RGBA and gray float pictures (SJPEG_HIP_SRC_RGB_F* / _RGBA_F* / _GRAY_F*) and the per-channel pixel
transform on the GPU.  The contract is sjpeg_hip.h's: a sample x of channel c becomes the byte
rint(clamp(fmaf(x, scale[c], bias[c]), 0, 255)) -- ties to even, NaN -> 0, +-inf saturate --, the fourth element of a
4-element pixel is never read, and the JPEG is that of the uint8 picture so defined.  Every expected value is the
oracle's for the uint8 picture the test derives itself on the CPU."""
import os

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import orc, synth

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
IDS = {F32: "f32", F16: "f16", BF16: "bf16"}
DT = {F32: 0, F16: 1, BF16: 2}
# away from ties, per channel: fp32 takes values around -1..1, half values in 0..1 and -1..1, bfloat16 (8 significant
# bits) exact small multiples
XFORM3 = {F32: ((127.5, 255.0, 63.75), (127.5, 0.0, 10.0)), F16: ((255.0, 127.5, 255.0), (0.0, 127.5, 0.0)),
          BF16: ((1.0, 2.0, 4.0), (0.0, 1.0, 2.0))}
DMAX = {F32: 0.4, F16: 0.25, BF16: 0.0}
SHAPES = [(1, 1), (7, 5), (8, 8), (9, 17), (33, 17), (64, 48)]
RAGGED = [(1, 1), (17, 13), (64, 48), (215, 279), (700, 24)]


def _fmt(dtype, step):
    return {1: sj.SRC_GRAY_F32, 3: sj.SRC_RGB_F32, 4: sj.SRC_RGBA_F32, 0: sj.SRC_RGB_PLANAR_F32}[step] + DT[dtype]


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.fixture(scope="module")
def risk_table():
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        tab = f.read()
    sj.set_riskiness_table(tab)
    return tab


@pytest.fixture(scope="module")
def ragged():
    """The five pictures of the ragged float tests (host [H, W, 3] uint8); never written to."""
    return [synth.g_struct(w, h, 5200 + k) if k % 2 == 0 else synth.g_noise(w, h, 5200 + k) for k, (w, h) in enumerate(RAGGED)]


@pytest.fixture(scope="module")
def shapes():
    """The pictures of the shape tests (host [H, W, 3] uint8); never written to."""
    return [synth.g_noise(w, h, 6100 + k) if k % 2 else synth.g_struct(w, h, 6100 + k) for k, (w, h) in enumerate(SHAPES)]


def _floats(im, dtype, scale=None, bias=None, dmax=None, seed=1):
    """A host [C, H, W] tensor of `dtype` (C = 3 for an [H, W, 3] picture, 1 for an [H, W] one) whose samples land AWAY
    from ties under the per-channel transform, and the uint8 picture it must be coded as.  Sample of channel c =
    fp32((k + d - bias[c]) / scale[c]) cast to dtype, d uniform in [-dmax, dmax] (0 for bfloat16, whose transform is
    exact).  The condition -- the float64 value of x * scale[c] + bias[c] within 0.45 of the byte, so that the last ulp
    of the fused multiply-add cannot change it -- is asserted here."""
    if scale is None:
        scale, bias = XFORM3[dtype]
    if dmax is None:
        dmax = DMAX[dtype]
    k = (im.transpose(2, 0, 1) if im.ndim == 3 else im[None]).astype(np.float64)
    s = np.asarray(scale, np.float64)[:k.shape[0], None, None]
    b = np.asarray(bias, np.float64)[:k.shape[0], None, None]
    d = np.random.RandomState(seed).uniform(-dmax, dmax, k.shape) if dmax > 0 else 0.0
    t = torch.from_numpy(((k + d - b) / s).astype(np.float32)).to(dtype)
    back = t.to(torch.float64).numpy() * s + b
    assert (np.abs(back - k) <= 0.45).all()
    u8 = np.empty(im.shape, np.uint8)
    u8[...] = k.astype(np.uint8).transpose(1, 2, 0) if im.ndim == 3 else k[0].astype(np.uint8)
    return t, u8


def _inter(t, step, off=0, pad=0, flip=False):
    """The CUDA copy of a host [3, H, W] tensor as interleaved pixels of `step` elements, cut out of a row of
    off + W + pad pixels at pixel `off`; the fourth element of every pixel (step 4) and the padding are NaN.  Returns the
    LOGICAL [3, H, W] view (strides 1, row, step).  flip: the rows are stored bottom-up (the view is then top-down again
    through a negative row stride the caller builds from it)."""
    c, h, w = t.shape
    buf = torch.full((h, off + w + pad, step), float("nan"), dtype=t.dtype)
    buf[:, off:off + w, :3] = (torch.flip(t, (1,)) if flip else t).permute(1, 2, 0)
    return buf.cuda()[:, off:off + w, :3].permute(2, 0, 1)


def _gray_dev(t, off=0, pad=0, squeeze=False):
    """The CUDA copy of a host [1, H, W] tensor as a crop of a wider one; [H, W] with squeeze."""
    _, h, w = t.shape
    buf = torch.full((1, h, off + w + pad), float("nan"), dtype=t.dtype)
    buf[:, :, off:off + w] = t
    v = buf.cuda()[:, :, off:off + w]
    return v[0] if squeeze else v


def _quant(q=75.0):
    m = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(float(q), m.ctypes.data)
    return m


def _rgb2d(im):
    return [im.reshape(im.shape[0], -1)]


def _gray_want(oracle, img, q=75.0, method=0):
    """the oracle's bytes of a uint8 gray picture [H, W], as the gray tests of test_gpu_parity.py obtain them"""
    return oracle.encode_src(sj.SRC_GRAY, [img], img.shape[1], img.shape[0], _quant(q), yuv_mode=4, method=method)


def _ragged_bytes(engine, fmt, planes, dims, mode, q=75.0):
    tables, qm = sj.make_tables(quality=q)
    headers = [sj.make_header(w, h, mode, qm) for (w, h) in dims]
    out, sizes, offs = engine.encode_ragged(fmt, planes, dims, mode, tables, headers)
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    return [host[offs[k]:offs[k] + int(sz[k])].tobytes() for k in range(len(dims))]


def _bytes_of(t, scale, bias):
    """The contract on the CPU for EXACT transforms (x * scale + bias without rounding in float64 and in fp32 alike)."""
    v = t.to(torch.float64).numpy() * scale + bias
    out = np.rint(np.clip(np.nan_to_num(v, nan=0.0, posinf=1e9, neginf=-1e9), 0, 255))
    out[np.isnan(v)] = 0
    return out.astype(np.uint8)


# ---- 1. shapes: the edge path alone, one block, clipped MCUs in both directions, inside rows next to clipped ones

@pytest.mark.parametrize("step", [3, 4])
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=IDS.get)
def test_shapes(engine, oracle, shapes, dtype, step):
    esz = torch.zeros((), dtype=dtype).element_size()
    keep, planes, want = [], [], []
    for k, im in enumerate(shapes):
        t, u8 = _floats(im, dtype, seed=20 + k)
        want.append(u8)
        h = im.shape[0]
        if im.shape[1] == 9:          # a crop of a wider tensor at an odd column
            v = _inter(t, step, 3, 2)
        elif im.shape[1] == 33:       # rows stored bottom-up
            v = _inter(t, step, 0, 1, flip=True)
        else:
            v = _inter(t, step, 0, k % 2)
        keep.append(v)
        rs = (v.stride(1) if h > 1 else v.shape[2] * step) * esz
        assert v.stride(0) == 1 and (v.shape[2] == 1 or v.stride(2) == step)
        planes.append([(v.data_ptr() + (h - 1) * rs, -rs)] if im.shape[1] == 33 else [(v.data_ptr(), rs)])
    dims = [(im.shape[1], im.shape[0]) for im in shapes]
    engine.set_pixel_transform(*XFORM3[dtype])
    for mode in (sj.YUV_420, sj.YUV_444, sj.YUV_400):
        got = _ragged_bytes(engine, _fmt(dtype, step), planes, dims, mode)
        for k, im in enumerate(want):
            assert got[k] == oracle.encode(im, 75.0, mode), (mode, k, im.shape)


# ---- 2. gray

@pytest.mark.parametrize("squeeze", [False, True], ids=["1hw", "hw"])
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=IDS.get)
def test_gray(engine, oracle, shapes, dtype, squeeze):
    dev, want = [], []
    for k, im in enumerate(shapes):
        t, u8 = _floats(im[:, :, 1], dtype, seed=40 + k)
        want.append(u8)
        dev.append(_gray_dev(t, 3 if im.shape[1] == 9 else 0, k % 2, squeeze))
    got = sj.encode_images(sj.FloatPixels(dev, *XFORM3[dtype]), 75.0, sj.YUV_400, engine=engine, layout="chw")
    for k, img in enumerate(want):
        assert got[k] == _gray_want(oracle, img), (k, img.shape)


# ---- 3. channel mapping

@pytest.mark.parametrize("step", [0, 3, 4], ids=["planar", "step3", "step4"])
@pytest.mark.parametrize("dtype", [F32, F16], ids=IDS.get)
def test_channel_mapping_exact(engine, oracle, dtype, step):
    """scale (1, 2, 4), bias (0, 1, 2) on exact inputs: a swapped or shared channel changes the bytes"""
    scale, bias = (1.0, 2.0, 4.0), (0.0, 1.0, 2.0)
    im = synth.g_noise(33, 17, 311)
    t, u8 = _floats(im, dtype, scale, bias, dmax=0.0)
    assert (_bytes_of(t, np.array(scale)[:, None, None], np.array(bias)[:, None, None]).transpose(1, 2, 0) == u8).all()
    wrong = _bytes_of(t, np.array(scale[::-1])[:, None, None], np.array(bias[::-1])[:, None, None])
    assert (wrong.transpose(1, 2, 0) != u8).any()
    dev = t.cuda() if step == 0 else _inter(t, step, 1, 1)
    got = sj.encode_images(sj.FloatPixels([dev], scale, bias), 90.0, sj.YUV_444, engine=engine, layout="chw")[0]
    assert got == oracle.encode(u8, 90.0, sj.YUV_444)
    assert engine.pixel_transform3() == (scale, bias)


@pytest.mark.parametrize("dtype,step", [(F32, 0), (F32, 4), (F16, 3)], ids=["f32-planar", "f32-step4", "f16-step3"])
def test_normalized(engine, oracle, dtype, step):
    im = synth.g_struct(33, 17, 312)
    fp0 = sj.FloatPixels.normalized([], (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    t, u8 = _floats(im, dtype, fp0.scale3, fp0.bias3, dmax=0.25)
    dev = t.cuda() if step == 0 else _inter(t, step, 0, 3)
    fp = sj.FloatPixels.normalized([dev], (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    got = sj.encode_images(fp, 75.0, sj.YUV_420, engine=engine, layout="chw")[0]
    assert got == oracle.encode(u8, 75.0, sj.YUV_420)


# ---- 4. exact rounding on the new load path

def _tie_values(dtype, shape):
    ties = [k + 0.5 for k in range(256 if dtype != BF16 else 128)]           # even and odd k
    special = [-0.0, -0.5, -3.0, 254.5, 255.5, 300.0, float("inf"), float("-inf"), float("nan"),
               float(np.float32(1e-45)), float(torch.finfo(dtype).smallest_normal) * float(torch.finfo(dtype).eps)]
    vals = np.array(ties + special * 4, np.float64)
    pick = np.random.RandomState(3).randint(0, len(vals), shape)
    pick.reshape(-1)[:len(vals)] = np.arange(len(vals))                     # every value at least once
    return torch.from_numpy(vals[pick]).to(torch.float32).to(dtype)


@pytest.mark.parametrize("dtype,step", [(F32, 3), (F16, 4), (BF16, 3), (F32, 4), (F16, 3), (BF16, 4)],
                         ids=lambda v: IDS.get(v, str(v)))
def test_exact_rounding_interleaved(engine, oracle, dtype, step):
    w, h = 64, 48
    t = _tie_values(dtype, (3, h, w))
    want = _bytes_of(t, 1.0, 0.0)
    print("scale 1: distinct expected bytes", len(np.unique(want)), "NaN samples", int(torch.isnan(t).sum()))
    got = sj.encode_images(sj.FloatPixels([_inter(t, step)], 1.0, 0.0), 90.0, sj.YUV_444, engine=engine, layout="chw")[0]
    assert got == oracle.encode(np.ascontiguousarray(want.transpose(1, 2, 0)), 90.0, sj.YUV_444), "scale 1, bias 0"
    # scale 256, bias 0.5, inputs j / 256: still exact, and now every sample is a tie
    j = np.random.RandomState(4).randint(0, 256, (3, h, w))
    j.reshape(-1)[:256] = np.arange(256)
    t = torch.from_numpy(j / 256.0).to(torch.float32).to(dtype)
    assert (t.to(torch.float64).numpy() * 256 == j).all()
    want = _bytes_of(t, 256.0, 0.5)
    assert (want[j < 255] % 2 == 0).all() and (want[j == 255] == 255).all()     # (ties go to the even byte; 255.5 is clamped first)
    got = sj.encode_images(sj.FloatPixels([_inter(t, step)], 256.0, 0.5), 90.0, sj.YUV_444, engine=engine, layout="chw")[0]
    assert got == oracle.encode(np.ascontiguousarray(want.transpose(1, 2, 0)), 90.0, sj.YUV_444), "scale 256, bias 0.5"


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=IDS.get)
def test_exact_rounding_gray(engine, oracle, dtype):
    w, h = 64, 48
    t = _tie_values(dtype, (1, h, w))
    want = _bytes_of(t, 1.0, 0.0)[0]
    got = sj.encode_images(sj.FloatPixels([_gray_dev(t)], 1.0, 0.0), 90.0, sj.YUV_400, engine=engine, layout="chw")[0]
    assert got == _gray_want(oracle, np.ascontiguousarray(want), 90.0)


# ---- 5. channels-last end to end

def test_channels_last_end_to_end(engine, oracle):
    n, h, w = 2, 17, 33
    pairs = [_floats(synth.g_struct(w, h, 700 + k), F16, (255.0,) * 3, (0.0,) * 3, 0.25, seed=k) for k in range(n)]
    x = torch.stack([p[0] for p in pairs]).cuda().to(memory_format=torch.channels_last)
    assert x.shape == (n, 3, h, w) and x[1].stride() == (1, 3 * w, 3)
    got = sj.encode_images(sj.FloatPixels([x[0], x[1]]), 75.0, sj.YUV_420, engine=engine, layout="chw")
    xc = x.contiguous()
    assert xc[1].stride() == (h * w, w, 1)
    planar = sj.encode_images(sj.FloatPixels([xc[0], xc[1]]), 75.0, sj.YUV_420, engine=engine, layout="chw")
    for k in range(n):
        assert got[k] == planar[k] == oracle.encode(pairs[k][1], 75.0, sj.YUV_420), k
    # the same for bytes: a uint8 channels_last batch against layout="chw" on its contiguous copy
    u = torch.stack([torch.from_numpy(np.ascontiguousarray(p[1].transpose(2, 0, 1))) for p in pairs]).cuda()
    ul = u.to(memory_format=torch.channels_last)
    assert ul[1].stride() == (1, 3 * w, 3)
    got = sj.encode_images([ul[0], ul[1]], 75.0, sj.YUV_420, engine=engine, layout="chw")
    planar = sj.encode_images([u[0], u[1]], 75.0, sj.YUV_420, engine=engine, layout="chw")
    for k in range(n):
        assert got[k] == planar[k] == oracle.encode(pairs[k][1], 75.0, sj.YUV_420), k


# ---- 6. flows: the five-picture ragged set, one interleaved dtype per flow, steps alternating

def _ragged_dev(ragged, dtype, step):
    """(CUDA interleaved float pictures as logical [3, H, W] views, the uint8 pictures they stand for); the 17 x 13 one
    cut out of a wider row at pixel 3, every other one with padded rows."""
    dev, want = [], []
    for k, im in enumerate(ragged):
        t, u8 = _floats(im, dtype, seed=10 + k)
        dev.append(_inter(t, step, 3, 4) if im.shape[1] == 17 else _inter(t, step, 0, 2 if k % 2 else 0))
        want.append(u8)
    return dev, want


def _fp(dev, dtype):
    return sj.FloatPixels(dev, *XFORM3[dtype])


def test_flow_method_4(engine, oracle, ragged):
    dev, want = _ragged_dev(ragged, F32, 3)
    got = sj.encode_images(_fp(dev, F32), 75.0, sj.YUV_420, engine=engine, method=4, layout="chw")
    for k, im in enumerate(want):
        assert got[k] == oracle.encode_method(im, 75.0, sj.YUV_420, 4), (k, im.shape)


def test_flow_trellis(engine, oracle, ragged):
    dev, want = _ragged_dev(ragged, F16, 4)
    got = sj.encode_images(_fp(dev, F16), 75.0, sj.YUV_420, engine=engine, method=4, use_trellis=True, layout="chw")
    for k, im in enumerate(want):
        assert got[k] == oracle.encode_method(im, 75.0, sj.YUV_420, 7), (k, im.shape)


def test_flow_target_size(engine, oracle, ragged):
    dev, want = _ragged_dev(ragged, BF16, 3)
    sizes = [max(int(0.7 * len(oracle.encode_method(im, 75.0, sj.YUV_420, 4))), 200) for im in want]
    got = sj.encode_images(_fp(dev, BF16), 75.0, sj.YUV_420, engine=engine, method=4, target_size=sizes, passes=5,
                           layout="chw")
    for k, im in enumerate(want):
        ref = oracle.encode_search(orc.SRC_RGB, _rgb2d(im), im.shape[1], im.shape[0], _quant(75.0), yuv_mode=sj.YUV_420,
                                   target_mode=1, target_value=float(sizes[k]), passes=5)
        assert got[k] == ref, (k, im.shape)


def test_flow_packed(engine, oracle, ragged):
    dev, want = _ragged_dev(ragged, F32, 4)
    qs = [60.0, 75.0, 90.0, 75.0, 40.0]
    got = sj.encode_images(_fp(dev, F32), qs, sj.YUV_420, engine=engine, packed=True, layout="chw")
    for k, (im, q) in enumerate(zip(want, qs)):
        assert got[k] == oracle.encode(im, q, sj.YUV_420), k


def _auto_want(oracle, im, verdict, sp=None):
    """What sjpeg::Encode() makes of the picture with the mode SJPEG_YUV_AUTO gave it (the sharp frames as planar 4:2:0)."""
    if verdict == sj.YUV_SHARP:
        fmt, planes, mode = orc.SRC_YUV420, list(oracle.sharp_yuv(im)), sj.YUV_420
    else:
        fmt, planes, mode = orc.SRC_RGB, _rgb2d(im), verdict
    if sp is None:
        return oracle.encode_src(fmt, planes, im.shape[1], im.shape[0], _quant(75.0), yuv_mode=mode, method=4)
    return oracle.encode_search(fmt, planes, im.shape[1], im.shape[0], _quant(75.0), yuv_mode=mode, target_mode=1,
                                target_value=float(sp), passes=4)


def test_flow_compress_and_riskiness(engine, oracle, ragged, risk_table):
    dev, want = _ragged_dev(ragged, F16, 3)
    verdicts = [oracle.riskiness(im, risk_table)[0] for im in want]
    assert [m for m, _ in sj.riskiness_images(_fp(dev, F16), engine=engine, layout="chw")] == verdicts
    got = sj.compress_images(_fp(dev, F16), 75.0, engine=engine, layout="chw")
    for k, im in enumerate(want):
        assert got[k] == _auto_want(oracle, im, verdicts[k]), (k, im.shape, verdicts[k])


def test_flow_sharp_yuv_ragged(engine, oracle, ragged):
    dtype, step = BF16, 4
    dev, want = _ragged_dev(ragged, dtype, step)
    engine.set_pixel_transform(*XFORM3[dtype])
    planes = [[(v.data_ptr(), (v.stride(1) if v.shape[1] > 1 else v.shape[2] * step) * 2)] for v in dev]
    got = engine.sharp_yuv_ragged(_fmt(dtype, step), planes, [(im.shape[1], im.shape[0]) for im in want])
    torch.cuda.synchronize()
    for k, im in enumerate(want):
        for a, b in zip(got[k], oracle.sharp_yuv(im)):
            assert (a.cpu().numpy() == np.asarray(b)).all(), (k, im.shape)


def test_flow_full_call_with_a_target(engine, oracle, ragged, risk_table):
    dev, want = _ragged_dev(ragged, F32, 3)
    verdicts = [oracle.riskiness(im, risk_table)[0] for im in want]
    targets = [max(int(0.7 * len(_auto_want(oracle, im, verdicts[k]))), 200) for k, im in enumerate(want)]
    got = sj.encode_images_full_chw(_fp(dev, F32), 75.0, sj.YUV_AUTO, method=4, target_size=targets, passes=4, engine=engine)
    for k, im in enumerate(want):
        assert got[k] == _auto_want(oracle, im, verdicts[k], sp=targets[k]), (k, im.shape, verdicts[k])


def test_flow_gray(engine, oracle, ragged):
    dtype = F16
    dev, want = [], []
    for k, im in enumerate(ragged):
        t, u8 = _floats(im[:, :, 0], dtype, seed=60 + k)
        dev.append(_gray_dev(t, 3 if im.shape[1] == 17 else 0, 2, squeeze=bool(k % 2)))
        want.append(u8)
    got = sj.encode_images(_fp(dev, dtype), 75.0, sj.YUV_400, engine=engine, method=4, layout="chw")
    for k, img in enumerate(want):
        assert got[k] == _gray_want(oracle, img, method=4), (k, img.shape)
    sizes = [max(int(0.7 * len(_gray_want(oracle, img, method=4))), 200) for img in want]
    got = sj.encode_images(_fp(dev, dtype), 75.0, sj.YUV_400, engine=engine, method=4, target_size=sizes, passes=5,
                           layout="chw")
    for k, img in enumerate(want):
        ref = oracle.encode_search(orc.SRC_GRAY, [img], img.shape[1], img.shape[0], _quant(75.0), yuv_mode=sj.YUV_400,
                                   target_mode=1, target_value=float(sizes[k]), passes=5)
        assert got[k] == ref, (k, img.shape)


# ---- 7. the uniform batch: make_source, Engine.encode_source and Engine.encode_batch (the lanes path)

@pytest.mark.parametrize("dtype,step", [(F16, 3), (BF16, 1)], ids=["f16-step3", "bf16-gray"])
def test_uniform_batch(engine, oracle, dtype, step):
    n, w, h = 3, 33, 17
    mode = sj.YUV_400 if step == 1 else sj.YUV_420
    imgs = [synth.g_struct(w, h, 900 + k) if k != 1 else synth.g_noise(w, h, 900 + k) for k in range(n)]
    pairs = [_floats(im if step == 3 else im[:, :, 2], dtype, seed=k) for k, im in enumerate(imgs)]
    # a frame stride larger than the frame: two spare rows and five spare elements a row
    big = torch.full((n, h + 2, w * step + 5), float("nan"), dtype=dtype)
    for k in range(n):
        big[k, :h, :w * step] = pairs[k][0].permute(1, 2, 0).reshape(h, w * step)
    x = big.cuda()[:, :h, :w * step]
    assert x.stride(0) > h * x.stride(1) and x.stride(2) == 1
    src, nf = sj.make_source(_fmt(dtype, step), [x])
    assert nf == n and src.row_stride[0] == x.stride(1) * x.element_size()
    engine.set_pixel_transform(*XFORM3[dtype])

    def want(k, method):
        if step == 1:
            return _gray_want(oracle, pairs[k][1], 80.0, method)
        return oracle.encode_method(pairs[k][1], 80.0, mode, method)

    tables, qm = sj.make_tables(quality=80.0)
    out, sizes = engine.encode_source(src, n, w, h, tables, sj.make_header(w, h, mode, qm), mode)
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    for k in range(n):
        assert host[k, :int(sz[k])].tobytes() == want(k, 0), k
    out, sizes = engine.encode_batch(src, n, w, h, mode, _quant(80.0), method=4)
    engine.wait()
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    for k in range(n):
        assert host[k, :int(sz[k])].tobytes() == want(k, 4), k


# ---- 8. the transform stays sticky and byte sources ignore it

def test_the_transform_is_sticky_and_bytes_ignore_it(oracle, ragged):
    eng = sj.Engine(0)
    assert eng.pixel_transform3() == ((255.0,) * 3, (0.0,) * 3)
    dev, want = _ragged_dev(ragged, BF16, 3)
    scale, bias = XFORM3[BF16]
    got = sj.encode_images(sj.FloatPixels(dev, scale, bias), 75.0, sj.YUV_420, engine=eng, layout="chw")
    assert eng.pixel_transform3() == (scale, bias)
    assert eng.pixel_transform() == (scale[0], bias[0])
    u8 = [torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1))).cuda() for im in want]
    again = sj.encode_images(u8, 75.0, sj.YUV_420, engine=eng, layout="chw")
    hwc = sj.encode_images([torch.from_numpy(im).cuda() for im in want], 75.0, sj.YUV_420, engine=eng)
    for k, im in enumerate(want):
        assert got[k] == again[k] == hwc[k] == oracle.encode(im, 75.0, sj.YUV_420), k
    assert eng.pixel_transform3() == (scale, bias)
    # a bare float tensor keeps the refusal it always had, and a refused transform changes nothing
    with pytest.raises(sj.SjpegError, match="is torch.float32, not torch.uint8"):
        sj.encode_images([dev[2].float()], engine=eng, layout="chw")
    with pytest.raises(sj.SjpegError, match="scale and bias must be finite"):
        eng.set_pixel_transform((1.0, float("inf"), 1.0), 0.0)
    assert eng.pixel_transform3() == (scale, bias)
    # the one-value setter fills three
    eng.set_pixel_transform(127.5, 127.5)
    assert eng.pixel_transform3() == ((127.5,) * 3, (127.5,) * 3)
