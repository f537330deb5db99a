"""tests/float_contract.py held to itself on the CPU: the exact rounding routine, the fast form against the slow one,
the existing float tests' _bytes_of where the transform is exact, and the CONDITIONS on the inputs the GPU tests
(tests/test_float_contract.py) stand on -- enough samples on which every near miss of the contract gives another byte,
and a picture in which every such byte reaches the JPEG."""
import fractions

import numpy as np
import pytest
import torch

import float_contract as fc
import sjpeg_amd as sj
from test_float_pixels import _bytes_of

DT = list(fc.DTYPES)


# ---- 1. one rounding to fp32

def test_round_to_f32_against_numpy_casts():
    """a float64 cast to float32 is ONE rounding of a known rational: normal, subnormal, overflowing, ties included"""
    rs = np.random.RandomState(1)
    v = np.concatenate([
        rs.uniform(-300, 300, 3000),
        np.ldexp(rs.uniform(0.5, 1, 3000), rs.randint(-160, 130, 3000)) * rs.choice([-1, 1], 3000),
        # exact midpoints of neighbouring fp32s, even and odd below: normal, subnormal and the one below 2^128
        np.ldexp(rs.randint(1 << 23, 1 << 24, 2000) + 0.5, rs.randint(-149, 104, 2000)),
        np.ldexp(rs.randint(0, 1 << 23, 500) + 0.5, -149),
        [2.0 ** 128 - 2.0 ** 103, 2.0 ** 128 - 2.0 ** 103 - 2.0 ** 80, 2.0 ** 128, 2.0 ** -150, 2.0 ** -150 * 1.0000001,
         2.0 ** -149, 0.0, 3.4028234663852886e38, 1e-46, -2.0 ** -150, -2.0 ** 128]])
    with np.errstate(all="ignore"):
        want = v.astype(np.float32).astype(np.float64)
    got = np.array([fc.round_to_f32(fractions.Fraction(float(x))) for x in v])
    assert np.array_equal(got, want)
    # rationals that are no float64: a third, and a hair either side of a midpoint
    mid = fractions.Fraction((1 << 23) + 1) + fractions.Fraction(1, 2)
    assert fc.round_to_f32(fractions.Fraction(1, 3)) == float(np.float32(1 / 3))
    assert fc.round_to_f32(mid) == float((1 << 23) + 2) and fc.round_to_f32(mid - 1) == float(1 << 23)
    assert fc.round_to_f32(mid + fractions.Fraction(1, 10 ** 30)) == float((1 << 23) + 2)
    assert fc.round_to_f32(mid - fractions.Fraction(1, 10 ** 30)) == float((1 << 23) + 1)


def test_one_rounding_differs_from_two_where_it_must():
    """x = 1 + 2^-12, scale = 1 + 2^-12: the product 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 (tie to even), and with
    bias 0.5 - (1 + 2^-11) two roundings give the tie 0.5 -> 0, one rounding 0.5 + 2^-24 -> 1"""
    x = torch.tensor([1.0 + 2.0 ** -12], dtype=torch.float32)
    s, b = 1.0 + 2.0 ** -12, 0.5 - (1.0 + 2.0 ** -11)
    assert fc.contract_bytes(x, s, b)[0] == 1 == fc.contract_bytes_slow(x, s, b)[0]
    assert fc.two_roundings(x, s, b)[0] == 0
    # inf * 0 is NaN and so 0; a NaN stays one whatever the transform; -inf saturates at 0, +inf at 255
    sp = torch.tensor([float("inf"), float("-inf"), float("nan")], dtype=torch.float32)
    assert fc.contract_bytes(sp, 0.0, 200.0).tolist() == [0, 0, 0] == fc.contract_bytes_slow(sp, 0.0, 200.0).tolist()
    assert fc.contract_bytes(sp, 2.0, 1.0).tolist() == [255, 0, 0] == fc.contract_bytes_slow(sp, 2.0, 1.0).tolist()
    assert fc.contract_bytes(sp, -2.0, 1.0).tolist() == [0, 255, 0]
    assert fc.nan_is_255(sp, 0.0, 1.0).tolist() == [255, 255, 255] and fc.nan_is_garbage(sp, 1.0, 0.0).tolist() == [255, 0, 128]


# ---- 2. the value sets

@pytest.mark.parametrize("dtype", DT, ids=fc.NAMES.get)
def test_value_sets(dtype):
    v = fc.values(dtype)
    bits = fc.to_bits(v)
    assert v.dtype == dtype and len(np.unique(bits)) == 65536
    x = fc.exact64(v)
    with np.errstate(all="ignore"):
        sub = (np.abs(x) < fc.MIN_NORMAL[dtype]) & (x != 0)
    assert int(sub.sum()) >= {fc.F32: 2048, fc.F16: 2046, fc.BF16: 254}[dtype]
    assert np.isinf(x).sum() == 2 and (x == 0).sum() == 2 and np.isnan(x).sum() >= 16
    if dtype == fc.F32:
        b = bits.astype(np.int64)
        for m in (0, 1, 0x400000, 0x7fffff):
            for sign in (0, 1 << 31):
                assert np.isin((np.arange(256) << 23) | m | sign, b).all()
        assert np.isin([0x7f800001, 0x7fa00000, 0xff800100], b).all()                       # signalling NaNs
        assert (np.abs(x[np.isfinite(x)]) * 255.0 > 3.5e38).sum() >= 256                       # the product overflows


# ---- 3. the fast form is the slow form; both are _bytes_of where that is exact

def test_fast_form_is_the_slow_form_on_every_half():
    v = fc.values(fc.F16)
    for name, (scale, bias) in fc.transforms(fc.F16):
        for c in range(3):
            assert np.array_equal(fc.bytes3(fc.F16, name)[c], fc.contract_bytes_slow(v, scale[c], bias[c])), (name, c)


@pytest.mark.parametrize("dtype", [fc.F32, fc.BF16], ids=fc.NAMES.get)
def test_fast_form_is_the_slow_form_on_an_eighth_of_the_others(dtype):
    v = fc.values(dtype)
    for name, (scale, bias) in fc.transforms(dtype):
        for c in range(3):
            k = (3 * fc.transforms(dtype).index((name, (scale, bias))) + c) % 8
            assert np.array_equal(fc.bytes3(dtype, name)[c][k::8], fc.contract_bytes_slow(v[k::8], scale[c], bias[c])), (name, c)


@pytest.mark.parametrize("dtype", DT, ids=fc.NAMES.get)
def test_contract_is_bytes_of_on_exact_transforms(dtype):
    v = fc.values(dtype)
    assert np.array_equal(fc.contract_bytes(v, 1.0, 0.0), _bytes_of(v, 1.0, 0.0))
    j = torch.from_numpy(np.arange(256) / 256.0).to(torch.float32).to(dtype)
    assert (fc.exact64(j) * 256 == np.arange(256)).all()
    assert np.array_equal(fc.contract_bytes(j, 256.0, 0.5), _bytes_of(j, 256.0, 0.5))
    ties = torch.from_numpy(np.arange(128) + 0.5).to(torch.float32).to(dtype)
    assert np.array_equal(fc.contract_bytes(ties, 1.0, 0.0), _bytes_of(ties, 1.0, 0.0))
    assert (fc.contract_bytes(ties, 1.0, 0.0) % 2 == 0).all()


# ---- 4. the conditions: every near miss changes enough bytes

@pytest.mark.parametrize("dtype", DT, ids=fc.NAMES.get)
def test_every_competing_model_differs_on_enough_samples(dtype):
    counts = {m: 0 for m in fc.MODELS}
    per = {}
    for name, _ in fc.transforms(dtype):
        want = fc.bytes3(dtype, name)
        for m in fc.MODELS:
            n = int((fc.bytes3(dtype, name, m) != want).sum())
            counts[m] += n
            per[(name, m)] = n
    print(fc.NAMES[dtype], counts)
    for m, least in fc.MINIMUM.items():
        assert counts[m] >= least, (m, counts[m], least)
    # the transforms made to separate do: one rounding from two, and a flushed subnormal from a kept one
    assert per[("cancelling", "two_roundings")] >= 100 and per[("drawn", "two_roundings")] >= 3
    assert per[("lift", "flush_inputs")] >= 100
    # and the one-channel transforms of the stream tests carry every model between them
    for m in fc.MODELS:
        n = sum(int((fc.bytes3(dtype, name, m)[c] != fc.bytes3(dtype, name)[c]).sum()) for name, c in fc.STREAM_TRANSFORMS)
        print("stream blocks", m, n)
        assert n >= fc.STREAM_MINIMUM, (m, n)


@pytest.mark.parametrize("dtype", DT, ids=fc.NAMES.get)
def test_transforms_are_what_the_entry_keeps(dtype):
    names = [n for n, _ in fc.transforms(dtype)]
    assert names[:7] == ["default", "signed", "bytes", "imagenet", "inverted", "scale0", "lift"]
    fp = sj.FloatPixels.normalized([], (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    assert fc.transform(dtype, "imagenet") == (fp.scale3, fp.bias3)
    for name, (scale, bias) in fc.transforms(dtype):
        fp = sj.FloatPixels([], scale, bias)
        assert fp.scale3 == tuple(scale) and fp.bias3 == tuple(bias)
        assert all(fc.f32(x) == x for x in scale + bias), name


@pytest.mark.parametrize("dtype", DT, ids=fc.NAMES.get)
def test_small_pictures_carry_the_discriminating_samples(dtype):
    """the 17 x 13 picture of the GPU tests' part 3c: every model that the transform separates at all shows in it"""
    idx = fc.probe(dtype, "cancelling", 17 * 13)
    want = fc.bytes3(dtype, "cancelling")[:, idx]
    for m in ("two_roundings", "half_away", "truncate", "nan_is_255", "nan_is_garbage"):
        assert (fc.bytes3(dtype, "cancelling", m)[:, idx] != want).sum() >= 3, m
    assert np.array_equal(idx, fc.probe(dtype, "cancelling", 17 * 13))


# ---- 5. observability: in a 4:4:4 picture of quality 100 a constant block of every gray level has its own stream

def test_every_byte_of_a_constant_block_reaches_the_stream(oracle):
    """The stream tests fill an 8 x 8 block with ONE value in the three channels under ONE transform, so the block is
    gray whatever the model: R = G = B = v.  256 levels, 256 different streams: whichever byte a model puts in place
    of the contract's, the JPEG differs.  (With a different transform per channel that does not hold: a step of 1 in
    B alone moves Y by 0.114 and is lost in its rounding more often than not -- shown here too.)"""
    streams = [oracle.encode(np.full((8, 8, 3), v, np.uint8), 100.0, sj.YUV_444) for v in range(256)]
    assert len(set(streams)) == 256
    blue = [oracle.encode(np.dstack([np.full((8, 8, 2), 100, np.uint8), np.full((8, 8, 1), v, np.uint8)]), 100.0, sj.YUV_444)
            for v in range(100, 108)]
    assert len(set(blue)) < 8
    # and for every model and every block of the stream pictures where it differs, by the above: the bytes differ
    for dtype in DT:
        for name, c in fc.STREAM_TRANSFORMS:
            want = fc.bytes3(dtype, name)[c]
            for m in fc.MODELS:
                got = fc.bytes3(dtype, name, m)[c]
                bad = np.flatnonzero(got != want)
                assert all(streams[int(got[i])] != streams[int(want[i])] for i in bad)
