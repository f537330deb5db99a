"""Float channel-first pictures (SJPEG_HIP_SRC_RGB_PLANAR_F32 / _F16 / _BF16, sj.FloatPixels): the loader's conversion
held to the contract of sjpeg_hip.h -- byte = rint(clamp(fmaf(x, scale, bias), 0, 255)), ties to even, NaN -> 0, +-inf
saturate -- on exact ties and away from them, the shapes of the planar tests, and every path that takes the formats.
Every expected value is the oracle's for the uint8 picture the test derives itself on the CPU."""
import os

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import orc, synth

pytestmark = pytest.mark.gpu

FMT = {torch.float32: sj.SRC_RGB_PLANAR_F32, torch.float16: sj.SRC_RGB_PLANAR_F16, torch.bfloat16: sj.SRC_RGB_PLANAR_BF16}
# the transform each dtype is tested with away from ties: values in -1..1, in 0..1, and bytes as they are
XFORM = {torch.float32: (127.5, 127.5), torch.float16: (255.0, 0.0), torch.bfloat16: (1.0, 0.0)}
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
RAGGED = [(1, 1), (17, 13), (64, 48), (215, 279), (700, 24)]
IDS = {F32: "f32", F16: "f16", BF16: "bf16"}


def _id(v):
    return IDS.get(v, None)


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
    """The five pictures of the ragged tests (host [H, W, 3] uint8); never written to."""
    return [synth.g_struct(w, h, 5200 + k) if k % 2 == 0 else synth.g_noise(w, h, 5200 + k) for k, (w, h) in enumerate(RAGGED)]


def _floats(im, dtype, scale=None, bias=None, dmax=0.25, seed=1):
    """A host [3, H, W] tensor of `dtype` whose samples land AWAY from ties, and the uint8 picture [H, W, 3] it must be
    coded as.  Sample = fp32((k + d - bias) / scale) cast to dtype, d uniform in [-dmax, dmax]; bfloat16 (8 significant
    bits) takes bytes that are multiples of 4 at scale 1, d = 0.  The condition -- the float64 value of x * scale + bias
    within 0.45 of k, so that the last ulp of the fused multiply-add cannot change the byte -- is checked here."""
    if scale is None:
        scale, bias = XFORM[dtype]
    k = im.transpose(2, 0, 1).astype(np.float64)
    if dtype == BF16:
        assert (scale, bias) == (1.0, 0.0)
        k = np.floor(k / 4) * 4
        d = 0.0
    else:
        d = np.random.RandomState(seed).uniform(-dmax, dmax, k.shape)
    t = torch.from_numpy(((k + d - bias) / scale).astype(np.float32)).to(dtype)
    back = t.to(torch.float64).numpy() * scale + bias
    assert (np.abs(back - k) <= 0.45).all()
    u8 = np.empty(im.shape, np.uint8)             # (a fresh array: a transposed 1 x 1 view reports strides of its own)
    u8[...] = k.astype(np.uint8).transpose(1, 2, 0)
    return t, u8


def _dev(t, off=0, pad=0):
    """The CUDA copy of a host [3, H, W] tensor as a crop of a [3, H, off + W + pad] tensor at column `off`: rows of the
    parent's pitch, addresses aligned to the element only."""
    c, h, w = t.shape
    big = torch.full((c, h, off + w + pad), 77.0, dtype=t.dtype)
    big[:, :, off:off + w] = t
    return big.cuda()[:, :, off:off + w]


def _ragged_dev(ragged, dtype):
    """(CUDA float pictures, the uint8 pictures they stand for); the 17 x 13 one cut out of a [3, 13, 24] tensor at
    column 3, every other one with padded rows."""
    dev, want = [], []
    for k, im in enumerate(ragged):
        t, u8 = _floats(im, dtype, seed=10 + k)
        dev.append(_dev(t, 3, 4) if im.shape[1] == 17 else _dev(t, 0, 8 if k % 2 else 0))
        want.append(u8)
    return dev, want


def _fp(dev, dtype):
    return sj.FloatPixels(dev, *XFORM[dtype])


def _quant(q=75.0):
    m = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(float(q), m.ctypes.data)
    return m


def _streams(out, sizes):
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    return [host[k, :int(sz[k])].tobytes() for k in range(len(sz))]


def _rgb2d(im):
    return [im.reshape(im.shape[0], -1)]


def _bytes_of(t, scale, bias):
    """The contract on the CPU for EXACT transforms (x * scale + bias without rounding in float64 and in fp32 alike)."""
    v = t.to(torch.float64).numpy() * scale + bias
    out = np.rint(np.clip(np.nan_to_num(v, nan=0.0, posinf=1e9, neginf=-1e9), 0, 255))
    out[np.isnan(v)] = 0
    return out.astype(np.uint8)


# ---- exact rounding: the test that decides whether the convert instruction alone rounds as the contract says

@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=_id)
def test_exact_rounding(engine, oracle, dtype):
    w, h = 64, 48
    ties = [k + 0.5 for k in range(256 if dtype != BF16 else 128)]           # even and odd k
    special = [-0.0, -0.5, -3.0, 254.5, 255.5, 300.0, float("inf"), float("-inf"), float("nan"),
               float(np.float32(1e-45)), float(torch.finfo(dtype).smallest_normal) * float(torch.finfo(dtype).eps)]
    vals = np.array(ties + special * 4, np.float64)
    pick = np.random.RandomState(3).randint(0, len(vals), (3, h, w))
    pick.reshape(-1)[:len(vals)] = np.arange(len(vals))                     # every value at least once
    t = torch.from_numpy(vals[pick]).to(torch.float32).to(dtype)
    want = _bytes_of(t, 1.0, 0.0)
    print("scale 1: distinct expected bytes", len(np.unique(want)), "NaN samples", int(torch.isnan(t).sum()))
    got = sj.encode_images(sj.FloatPixels([_dev(t)], 1.0, 0.0), 90.0, sj.YUV_444, engine=engine, layout="chw")[0]
    assert got == oracle.encode(np.ascontiguousarray(want.transpose(1, 2, 0)), 90.0, sj.YUV_444), "scale 1, bias 0"
    # scale 256, bias 0.5, inputs j / 256: still exact, and now every sample is a tie
    j = np.random.RandomState(4).randint(0, 256, (3, h, w))
    j.reshape(-1)[:256] = np.arange(256)
    t = torch.from_numpy(j / 256.0).to(torch.float32).to(dtype)
    assert (t.to(torch.float64).numpy() * 256 == j).all()
    want = _bytes_of(t, 256.0, 0.5)
    assert (want[j < 255] % 2 == 0).all() and (want[j == 255] == 255).all()     # (ties go to the even byte; 255.5 is clamped first)
    got = sj.encode_images(sj.FloatPixels([_dev(t)], 256.0, 0.5), 90.0, sj.YUV_444, engine=engine, layout="chw")[0]
    assert got == oracle.encode(np.ascontiguousarray(want.transpose(1, 2, 0)), 90.0, sj.YUV_444), "scale 256, bias 0.5"


# ---- away from ties: the byte is k whatever the rounding of the fma's last ulp

@pytest.mark.parametrize("dtype,scale,bias,dmax", [(F32, 255.0, 0.0, 0.4), (F32, 127.5, 127.5, 0.4), (F16, 255.0, 0.0, 0.25),
                                                   (F16, 127.5, 127.5, 0.25), (BF16, 1.0, 0.0, 0.0)],
                         ids=["f32-255", "f32-127.5", "f16-255", "f16-127.5", "bf16-1"])
def test_away_from_ties(engine, oracle, dtype, scale, bias, dmax):
    im = synth.g_noise(64, 48, 77)
    im[0, :, 0] = np.arange(64) * 4                                         # the low and the high end too
    im[1, :, 1] = 255 - np.arange(64)
    t, u8 = _floats(im, dtype, scale, bias, dmax)
    got = sj.encode_images(sj.FloatPixels([_dev(t)], scale, bias), 75.0, sj.YUV_420, engine=engine, layout="chw")[0]
    assert got == oracle.encode(u8, 75.0, sj.YUV_420)


# ---- shapes, through the uniform batch in the three samplings

@pytest.mark.parametrize("w,h,mode,dtype", [
    (64, 48, sj.YUV_420, F32),      # interior segments only
    (17, 13, sj.YUV_420, F16),      # clipped in x and y; cut out at column 3: element-aligned addresses only
    (17, 13, sj.YUV_400, F32),
    (1, 1, sj.YUV_444, BF16),
    (1, 1, sj.YUV_420, F32),
    (700, 24, sj.YUV_420, BF16),    # more than 42 MCUs wide: a segment wraps to the next MCU row
    (700, 24, sj.YUV_444, F16),
    (330, 50, sj.YUV_400, F16),     # several segments, clipped
    (330, 50, sj.YUV_444, F32),
    (330, 50, sj.YUV_420, BF16)], ids=lambda v: IDS.get(v, str(v)))
def test_uniform_batch(engine, oracle, w, h, mode, dtype):
    n = 3
    imgs = [synth.g_struct(w, h, 900 + k) if k != 1 else synth.g_noise(w, h, 900 + k) for k in range(n)]
    pairs = [_floats(im, dtype, seed=k) for k, im in enumerate(imgs)]
    off = 3 if w == 17 else 0
    big = torch.full((n, 3, h, off + w + 4), 5.0, dtype=dtype)
    for k in range(n):
        big[k, :, :, off:off + w] = pairs[k][0]
    x = big.cuda()[:, :, :, off:off + w]
    src, nf = sj.make_source(FMT[dtype], (x[:, 0], x[:, 1], x[:, 2]))
    assert nf == n
    engine.set_pixel_transform(*XFORM[dtype])
    assert engine.pixel_transform() == XFORM[dtype]
    tables, qm = sj.make_tables(quality=75.0)
    out, sizes = engine.encode_source(src, n, w, h, tables, sj.make_header(w, h, mode, qm), mode)
    got = _streams(out, sizes)
    for k in range(n):
        assert got[k] == oracle.encode(pairs[k][1], 75.0, mode), (k, w, h, mode)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=_id)
def test_uniform_batch_method_4(engine, oracle, dtype):
    w, h, n = 330, 50, 3
    pairs = [_floats(synth.g_struct(w, h, 950 + k), dtype, seed=k) for k in range(n)]
    x = torch.stack([p[0] for p in pairs]).cuda()
    src, _ = sj.make_source(FMT[dtype], (x[:, 0], x[:, 1], x[:, 2]))
    engine.set_pixel_transform(*XFORM[dtype])
    out, sizes = engine.encode_batch(src, n, w, h, sj.YUV_420, _quant(80.0), method=4)
    engine.wait()
    got = _streams(out, sizes)
    for k in range(n):
        assert got[k] == oracle.encode_method(pairs[k][1], 80.0, sj.YUV_420, 4), k


def test_bottom_up_rows(engine, oracle):
    dtype = F32
    imgs = [synth.g_struct(101, 67, 77), synth.g_noise(64, 48, 78)]
    keep, planes, want = [], [], []
    for im in imgs:
        h = im.shape[0]
        t, u8 = _floats(im, dtype)
        want.append(u8)
        d = _dev(torch.flip(t, (1,)), 1, 4)             # stored bottom-up
        keep.append(d)
        rs = d.stride(1) * 4
        planes.append([(d[c].data_ptr() + (h - 1) * rs, -rs) for c in range(3)])
    engine.set_pixel_transform(*XFORM[dtype])
    tables, qm = sj.make_tables(quality=75.0)
    headers = [sj.make_header(im.shape[1], im.shape[0], sj.YUV_420, qm) for im in imgs]
    out, sizes, offs = engine.encode_ragged(FMT[dtype], planes, [(im.shape[1], im.shape[0]) for im in imgs], sj.YUV_420,
                                            tables, headers)
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    for k in range(len(imgs)):
        assert host[offs[k]:offs[k] + int(sz[k])].tobytes() == oracle.encode(want[k], 75.0, sj.YUV_420), k


# ---- the ragged list through the torch-facing calls

@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=_id)
def test_ragged_method_0(engine, oracle, ragged, dtype):
    dev, want = _ragged_dev(ragged, dtype)
    for mode in (sj.YUV_420, sj.YUV_444, sj.YUV_400):
        got = sj.encode_images(_fp(dev, dtype), 75.0, mode, engine=engine, layout="chw")
        for k, im in enumerate(want):
            assert got[k] == oracle.encode(im, 75.0, mode), (mode, k, im.shape)


@pytest.mark.parametrize("dtype", [F32, F16], ids=_id)
def test_ragged_method_4(engine, oracle, ragged, dtype):
    dev, want = _ragged_dev(ragged, dtype)
    got = sj.encode_images(_fp(dev, dtype), 75.0, sj.YUV_420, engine=engine, method=4, layout="chw")
    for k, im in enumerate(want):
        assert got[k] == oracle.encode_method(im, 75.0, sj.YUV_420, 4), (k, im.shape)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_id)
def test_ragged_trellis(engine, oracle, ragged, dtype):
    dev, want = _ragged_dev(ragged, dtype)
    got = sj.encode_images(_fp(dev, dtype), 75.0, sj.YUV_420, engine=engine, method=4, use_trellis=True, layout="chw")
    for k, im in enumerate(want):
        assert got[k] == oracle.encode_method(im, 75.0, sj.YUV_420, 7), (k, im.shape)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=_id)
def test_ragged_target_size(engine, oracle, ragged, dtype):
    dev, want = _ragged_dev(ragged, dtype)
    sizes = [max(int(0.7 * len(oracle.encode_method(im, 75.0, sj.YUV_420, 4))), 200) for im in want]
    got = sj.encode_images(_fp(dev, dtype), 75.0, sj.YUV_420, engine=engine, method=4, target_size=sizes, passes=5,
                           layout="chw")
    for k, im in enumerate(want):
        ref = oracle.encode_search(orc.SRC_RGB, _rgb2d(im), im.shape[1], im.shape[0], _quant(75.0), yuv_mode=sj.YUV_420,
                                   target_mode=1, target_value=float(sizes[k]), passes=5)
        assert got[k] == ref, (k, im.shape)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_id)
def test_ragged_packed(engine, oracle, ragged, dtype):
    dev, want = _ragged_dev(ragged, dtype)
    qs = [60.0, 75.0, 90.0, 75.0, 40.0]
    got = sj.encode_images(_fp(dev, dtype), qs, sj.YUV_420, engine=engine, packed=True, layout="chw")
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


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=_id)
def test_riskiness_and_compress_images(engine, oracle, ragged, risk_table, dtype):
    dev, want = _ragged_dev(ragged, dtype)
    # the riskiness: the sums of the uint8 call, exactly
    u8 = [torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1))).cuda() for im in want]
    dims = [(im.shape[1], im.shape[0]) for im in want]
    engine.set_pixel_transform(*XFORM[dtype])
    a = engine.riskiness_ragged(FMT[dtype], [[(d[c].data_ptr(), (d.stride(1) if d.shape[1] > 1 else d.shape[2]) * d.element_size())
                                             for c in range(3)] for d in dev], dims).cpu().numpy()
    b = engine.riskiness_ragged(sj.SRC_RGB_PLANAR, [[t[0], t[1], t[2]] for t in u8], dims).cpu().numpy()
    assert (a == b).all()
    verdicts = [oracle.riskiness(im, risk_table)[0] for im in want]
    assert [m for m, _ in sj.riskiness_images(_fp(dev, dtype), engine=engine, layout="chw")] == verdicts
    got = sj.compress_images(_fp(dev, dtype), 75.0, engine=engine, layout="chw")
    for k, im in enumerate(want):
        assert got[k] == _auto_want(oracle, im, verdicts[k]), (k, im.shape, verdicts[k])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_id)
def test_sharp_yuv(engine, oracle, ragged, dtype):
    dev, want = _ragged_dev(ragged, dtype)
    got = sj.encode_images(_fp(dev, dtype), 75.0, sj.YUV_SHARP, engine=engine, method=4, layout="chw")
    for k, im in enumerate(want):
        assert got[k] == _auto_want(oracle, im, sj.YUV_SHARP), (k, im.shape)


@pytest.mark.parametrize("dtype", [F16, F32], ids=_id)
def test_full_call_with_a_target(engine, oracle, ragged, risk_table, dtype):
    dev, want = _ragged_dev(ragged, dtype)
    verdicts = [oracle.riskiness(im, risk_table)[0] for im in want]
    targets = [max(int(0.7 * len(_auto_want(oracle, im, verdicts[k]))), 200) for k, im in enumerate(want)]
    got = sj.encode_images_full_chw(_fp(dev, dtype), 75.0, sj.YUV_AUTO, method=4, target_size=targets, passes=4, engine=engine)
    for k, im in enumerate(want):
        assert got[k] == _auto_want(oracle, im, verdicts[k], sp=targets[k]), (k, im.shape, verdicts[k])


def test_the_transform_is_sticky_and_bytes_ignore_it(oracle, ragged):
    eng = sj.Engine(0)
    assert eng.pixel_transform() == (255.0, 0.0)
    dev, want = _ragged_dev(ragged, BF16)
    got = sj.encode_images(sj.FloatPixels(dev, 1.0, 0.0), 75.0, sj.YUV_420, engine=eng, layout="chw")
    assert eng.pixel_transform() == (1.0, 0.0)
    u8 = [torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1))).cuda() for im in want]
    again = sj.encode_images(u8, 75.0, sj.YUV_420, engine=eng, layout="chw")
    for k, im in enumerate(want):
        assert got[k] == again[k] == oracle.encode(im, 75.0, sj.YUV_420), k
    # a bare float tensor keeps the refusal it always had
    with pytest.raises(sj.SjpegError, match="is torch.float32, not torch.uint8"):
        sj.encode_images([dev[2].float()], engine=eng, layout="chw")
    with pytest.raises(sj.SjpegError, match="scale and bias must be finite"):
        eng.set_pixel_transform(float("inf"), 0.0)
    assert eng.pixel_transform() == (1.0, 0.0)
