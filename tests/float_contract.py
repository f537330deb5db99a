"""The float pixel transform of sjpeg_hip.h as an exact model, the ways a kernel can miss it by a hair, and the inputs
that tell them apart: shared by the CPU tests (tests/test_float_contract_host.py: the model against itself and the
conditions on the inputs) and the GPU tests (tests/test_float_contract.py: the kernels against the model).  No pytest
in here.

The contract, scale and bias being fp32 and those of the sample's channel:
    t  = fmaf((float)x, scale, bias)                 ONE fp32 rounding; (float)x is exact for half and bfloat16
    u8 = isnan(t) ? 0 : rint(min(max(t, 0), 255))    half to even; +-inf saturate
contract_bytes() computes x * scale + bias WITHOUT rounding, rounds it once to fp32 (nearest even, subnormals, overflow
to +-inf) and makes the byte.  Values travel as CPU torch tensors of torch.float32 / float16 / bfloat16 (numpy has no
bfloat16); all arithmetic is float64 where that is exact and integers where it is not."""
import fractions
import math

import numpy as np
import torch

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = (F32, F16, BF16)
NAMES = {F32: "f32", F16: "f16", BF16: "bf16"}
# below this magnitude a value of the dtype is subnormal
MIN_NORMAL = {F32: 2.0 ** -126, F16: 2.0 ** -14, BF16: 2.0 ** -126}
BITS = {F32: (torch.int32, np.uint32), F16: (torch.int16, np.uint16), BF16: (torch.int16, np.uint16)}


# ---- values

def from_bits(bits, dtype):
    """the tensor of `dtype` with these bit patterns (any integer array)"""
    tint, nint = BITS[dtype]
    a = np.ascontiguousarray(np.asarray(bits).astype(nint))
    return torch.from_numpy(a.view(np.int32 if nint is np.uint32 else np.int16)).view(dtype)


def to_bits(t):
    """the bit patterns of a tensor, as unsigned numpy integers"""
    tint, nint = BITS[t.dtype]
    return t.contiguous().view(tint).numpy().view(nint)


def exact64(t):
    """the values as float64: exact for the three dtypes"""
    return t.to(torch.float64).numpy()


def f32(v):
    """a Python float that is an fp32 value: what the engine keeps of a scale or bias"""
    return float(np.float32(v))


# ---- one rounding to fp32, exactly

def _round_ratio(num, den):
    """The fp32 nearest to num / den (integers, den > 0), ties to even, with fp32 subnormals and overflow to +-inf, as
    a Python float.  Integer arithmetic only."""
    if num == 0:
        return 0.0
    a = abs(num)
    e = a.bit_length() - den.bit_length()                             # 2^(e-1) < a / den < 2^(e+1)
    if (a << max(-e, 0)) < (den << max(e, 0)):
        e -= 1                                                        # now 2^e <= a / den < 2^(e+1)
    qe = max(e, -126) - 23                                            # the quantum is 2^qe; subnormals share 2^-149
    n, rem = divmod(a << max(-qe, 0), den << max(qe, 0))
    if 2 * rem > (den << max(qe, 0)) or (2 * rem == (den << max(qe, 0)) and (n & 1)):
        n += 1
    if n.bit_length() + qe > 128:                                     # n * 2^qe >= 2^128
        return float("inf") if num > 0 else float("-inf")
    r = math.ldexp(n, qe)                                             # (n <= 2^24: exact)
    return r if num > 0 else -r


def round_to_f32(q):
    """round-to-nearest-even of a rational (fractions.Fraction, int or float) to fp32, as a Python float"""
    q = fractions.Fraction(q)
    return _round_ratio(q.numerator, q.denominator)


def _fma_slow(x, scale, bias):
    """fmaf(x, scale, bias) of float64 values that are exact, element by element in integers; float64 array of fp32s"""
    sn, sd = float(scale).as_integer_ratio()
    bn, bd = float(bias).as_integer_ratio()
    out = np.empty(x.shape, np.float64)
    flat = out.reshape(-1)
    for i, v in enumerate(x.reshape(-1).tolist()):
        if v != v:
            flat[i] = np.nan
        elif v in (float("inf"), float("-inf")):
            flat[i] = np.nan if scale == 0 else (v if scale > 0 else -v)
        else:
            xn, xd = v.as_integer_ratio()
            flat[i] = _round_ratio(xn * sn * bd + bn * xd * sd, xd * sd * bd)
    return out


def _round_sum(p, bias):
    """fl32(p + bias) for a float64 array p of exact values: ONE rounding of the exact sum.  The sum is made in float64
    with its error term (TwoSum).  Where the error is 0 the float64 sum is exact and numpy's cast to float32 is the one
    rounding.  Where it is not, the exact sum lies strictly between the float64 sum and a float64 neighbour; every fp32
    and every midpoint of two fp32s is a float64, so the cast of the float64 sum is still right unless that sum IS such
    a midpoint (or the cast overflowed within reach of the midpoint below 2^128): only those elements go through exact
    integers."""
    with np.errstate(all="ignore"):
        s = p + bias
        bb = s - p
        err = (p - (s - bb)) + (bias - bb)
        r = s.astype(np.float32)
        r64 = r.astype(np.float64)
        d = s - r64
        toward = np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        gap = np.nextafter(r, toward).astype(np.float64) - r64
        unsure = np.isfinite(s) & (err != 0) & ((2 * d == gap) | (~np.isfinite(r64) & (np.abs(s) <= 2.0 ** 128)))
    out = r64
    if unsure.any():
        fb = fractions.Fraction(bias)
        idx = np.flatnonzero(unsure)
        flat, pf = out.reshape(-1), p.reshape(-1)
        for i in idx.tolist():
            flat[i] = round_to_f32(fractions.Fraction(float(pf[i])) + fb)
    return out


def _product(x, scale):
    """x * scale in float64: exact, both having at most 24 significant bits and the exponents room (NaN where inf * 0)"""
    with np.errstate(all="ignore"):
        return x * np.float64(scale)


def _check_transform(scale, bias):
    assert f32(scale) == scale and f32(bias) == bias and np.isfinite(scale) and np.isfinite(bias), (scale, bias)


def fma32(t, scale, bias):
    """fmaf((float)x, scale, bias) for every element of the tensor: a float64 array holding fp32 values"""
    _check_transform(scale, bias)
    return _round_sum(_product(exact64(t), scale), np.float64(bias))


def to_byte(v, nan=0):
    """the contract's second line on fp32 values held in float64"""
    isnan = np.isnan(v)
    out = np.rint(np.clip(np.where(isnan, 0.0, v), 0.0, 255.0)).astype(np.uint8)
    out[isnan] = nan
    return out


# ---- the contract and its near misses: (tensor, scale, bias) -> uint8 array of the tensor's shape

def contract_bytes(t, scale, bias):
    return to_byte(fma32(t, scale, bias))


def contract_bytes_slow(t, scale, bias):
    """the same, every element in rationals: the definition the fast form is held to"""
    _check_transform(scale, bias)
    return to_byte(_fma_slow(exact64(t), scale, bias))


def two_roundings(t, scale, bias):
    """fl32(fl32(x * scale) + bias): a multiply and an add in place of the fused one"""
    _check_transform(scale, bias)
    with np.errstate(all="ignore"):
        p = _product(exact64(t), scale).astype(np.float32).astype(np.float64)
    return to_byte(_round_sum(p, np.float64(bias)))


def flush_inputs(t, scale, bias):
    """subnormal x taken as +-0 before the multiply"""
    x = exact64(t)
    x = np.where(np.abs(x) < MIN_NORMAL[t.dtype], 0.0, x)
    _check_transform(scale, bias)
    return to_byte(_round_sum(_product(x, scale), np.float64(bias)))


def half_away(t, scale, bias):
    """ties away from zero instead of to even"""
    v = fma32(t, scale, bias)
    isnan = np.isnan(v)
    out = np.floor(np.clip(np.where(isnan, 0.0, v), 0.0, 255.0) + 0.5).astype(np.uint8)       # (exact in float64)
    out[isnan] = 0
    return out


def truncate(t, scale, bias):
    """(uint8)t without rounding"""
    v = fma32(t, scale, bias)
    isnan = np.isnan(v)
    out = np.floor(np.clip(np.where(isnan, 0.0, v), 0.0, 255.0)).astype(np.uint8)
    out[isnan] = 0
    return out


def nan_is_255(t, scale, bias):
    return to_byte(fma32(t, scale, bias), nan=255)


def nan_is_garbage(t, scale, bias):
    return to_byte(fma32(t, scale, bias), nan=128)


MODELS = {"two_roundings": two_roundings, "flush_inputs": flush_inputs, "half_away": half_away, "truncate": truncate,
          "nan_is_255": nan_is_255, "nan_is_garbage": nan_is_garbage}
# the least number of (value, channel of a transform) samples per dtype on which a model's byte must differ from the
# contract's, asserted in tests/test_float_contract_host.py
MINIMUM = {"two_roundings": 100, "flush_inputs": 100, "half_away": 120, "truncate": 1000, "nan_is_255": 16,
           "nan_is_garbage": 16}


# ---- transforms: (name, (scale[3], bias[3])), every number an fp32

def _imagenet():
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    return tuple(f32(255.0 * s) for s in std), tuple(f32(255.0 * m) for m in mean)


def _cancelling(j):
    """A transform under which MANY samples separate one rounding from two.  scale = 2^j * (1 + 2^-23): the product
    of a sample x = M * 2^e (M an integer below 2^23, 2^(e+j) the unit) is x * 2^j plus between one and two ulps, and
    rounds to x * 2^j + 1 ulp while M * 2^-23 has a fraction below one half.  For the binade B <= x * 2^j < 1.5 * B the
    bias 0.5 - B - ulp(B) cancels all of that but the rounding error: two roundings land ON the tie (x * 2^j - B) + 0.5,
    one rounding lands the error above it, and the error, (x * 2^j - B) * 2^-23, is at least an ulp of the tie."""
    big = 128.0 * 2.0 ** j if j <= 2 else 128.0
    scale = f32(2.0 ** j * (1.0 + 2.0 ** -23))
    bias = f32(0.5 - big - big * 2.0 ** -23)
    assert bias == 0.5 - big - big * 2.0 ** -23
    return scale, bias


def _drawn(values, seed, tries=400):
    """The construction one sample at a time: draw x0 from `values`, a scale s in 50..250 and a small k; if the exact
    product p = x0 * s is no fp32, r = fl32(p) and bias = k + 0.5 - r is one, then two roundings land on the tie
    k + 0.5 and one rounding beside it.  Returns the three (scale, bias) of the draws on which the two bytes differ for
    the most samples of `values`."""
    rs = np.random.RandomState(seed)
    x = exact64(values)
    ok = np.flatnonzero(np.isfinite(x) & (np.abs(x) > 2.0 ** -8) & (np.abs(x) < 4.0))
    found = []
    for _ in range(tries):
        x0 = float(x[ok[rs.randint(len(ok))]])
        s = f32(rs.uniform(50.0, 250.0) * (1 if x0 > 0 else -1))
        k = int(rs.randint(0, 8))
        p = x0 * s
        r = float(np.float32(p))
        b = k + 0.5 - r
        if r == p or f32(b) != b:
            continue
        one = contract_bytes(values, s, b)
        n = int((two_roundings(values, s, b) != one).sum())
        if n:
            found.append((n, len(found), s, b))
        if len(found) >= 12:
            break
    found.sort(reverse=True)
    assert len(found) >= 3
    return tuple(f[2] for f in found[:3]), tuple(f[3] for f in found[:3])


_transforms = {}


def transforms(dtype):
    """The per-channel transforms a dtype is tested with, in a fixed order; made once."""
    if dtype not in _transforms:
        lift = 2.0 ** 22 if dtype == F16 else 1.5 * 2.0 ** 127
        c = [_cancelling(j) for j in (1, 2, 0)]
        out = [("default", ((255.0,) * 3, (0.0,) * 3)),
               ("signed", ((127.5,) * 3, (127.5,) * 3)),
               ("bytes", ((1.0,) * 3, (0.0,) * 3)),
               ("imagenet", _imagenet()),
               ("inverted", ((-255.0, -127.5, -1.0), (255.0, 255.0, 255.0))),
               ("scale0", ((0.0, 0.0, 0.0), (7.5, 300.0, -1.0))),
               ("lift", ((lift, lift, -lift), (0.0, 2.0, 2.0))),
               ("ties256", ((256.0, 128.0, 512.0), (0.5, 0.5, 0.5))),
               ("cancelling", (tuple(s for s, _ in c), tuple(b for _, b in c))),
               ("drawn", _drawn(values(dtype), 11 + DTYPES.index(dtype)))]
        _transforms[dtype] = out
    return _transforms[dtype]


# The transforms of the stream tests, as (name, channel): there ONE (scale, bias) serves the three channels, so that a
# block is gray and every byte reaches the stream (tests/test_float_contract_host.py shows why): the default, two
# constructed ones and the one that lifts subnormals, with bias 2.
STREAM_TRANSFORMS = (("default", 0), ("cancelling", 1), ("drawn", 0), ("lift", 1))
# the least number of blocks of the stream pictures on which every model differs, per dtype (the smallest count is
# bfloat16's half_away: 44)
STREAM_MINIMUM = 40


def transform(dtype, name):
    return dict(transforms(dtype))[name]


# ---- the value sets: 65 536 bit patterns per dtype

def _f32_bits():
    rs = np.random.RandomState(20)
    parts = []
    # every exponent with mantissas 0, 1, 0x400000, 0x7fffff, both signs: +-0, +-inf, quiet and signalling NaNs among them
    e = np.arange(256, dtype=np.uint64)[:, None, None] << 23
    m = np.array([0, 1, 0x400000, 0x7fffff], np.uint64)[None, :, None]
    sg = np.array([0, 1 << 31], np.uint64)[None, None, :]
    parts.append((e | m | sg).reshape(-1))
    # more NaN payloads, signalling (quiet bit clear) and quiet
    parts.append(np.array([0x7f800002, 0x7fa00000, 0x7f8fffff, 0xff800100, 0x7fc00001, 0xffc12345, 0x7fffffff, 0xffffffff],
                          np.uint64))
    # 2 048 subnormals across the whole mantissa range, every eighth negative
    sub = np.linspace(1, 0x7fffff, 2048).astype(np.uint64)
    sub[7::8] |= 1 << 31
    parts.append(sub)
    # values whose product with 255 or 127.5 overflows, and ones around the largest finite
    parts.append((np.uint64(0x7e800000) + rs.randint(0, 0x00ffffff, 256).astype(np.uint64)) | (rs.randint(0, 2, 256).astype(np.uint64) << 31))
    # constructed near-ties: the fp32 nearest to (k + 0.5 - bias) / scale and its neighbours two ulps either side
    near = []
    for scale, bias in ((255.0, 0.0), (127.5, 127.5), (1.0, 0.0), (-255.0, 255.0), (256.0, 0.5)) + \
            tuple(zip(*_imagenet())):
        k = np.arange(256, dtype=np.float64)
        x = ((k + 0.5 - bias) / scale).astype(np.float32)
        for d in range(-2, 3):
            near.append((x.view(np.uint32).astype(np.int64) + d).astype(np.uint64) & 0xffffffff)
    parts.append(np.concatenate(near))
    # the binade in which the three cancelling transforms separate one rounding from two (x in 128 .. 192), on the
    # quarter integers and off them
    x = np.concatenate([np.arange(128, 192, 0.25), 128 + rs.randint(0, 1 << 22, 512) * 2.0 ** -16])
    parts.append(x.astype(np.float32).view(np.uint32).astype(np.uint64))
    # samples in and around the usual input ranges
    x = np.concatenate([rs.uniform(-0.25, 1.25, 12000), rs.uniform(-1.5, 1.5, 6000), rs.uniform(-8, 300, 6000),
                        rs.uniform(-3, 3, 2000)])
    parts.append(x.astype(np.float32).view(np.uint32).astype(np.uint64))
    have = np.unique(np.concatenate(parts))
    # the rest: raw bits
    while len(have) < 65536:
        more = rs.randint(0, 1 << 32, 65536 - len(have), dtype=np.uint64)
        have = np.unique(np.concatenate([have, more]))
    assert len(have) == 65536
    return rs.permutation(have).astype(np.uint32)


_values = {}


def values(dtype):
    """The 65 536 values a dtype is tested on (a CPU tensor, never written to): every bit pattern of float16 and of
    bfloat16; for float32 the patterns of _f32_bits()."""
    if dtype not in _values:
        _values[dtype] = from_bits(np.arange(65536) if dtype != F32 else _f32_bits(), dtype)
    return _values[dtype]


# ---- expected bytes of a whole value set, cached

_cache = {}


def bytes3(dtype, name, model=None):
    """[3, 65536] uint8: what the contract (or a competing model, by name) makes of values(dtype) under the three
    channels of the transform `name`.  Cached; never written to."""
    key = (dtype, name, model)
    if key not in _cache:
        fn = contract_bytes if model is None else MODELS[model]
        scale, bias = transform(dtype, name)
        out = np.stack([fn(values(dtype), scale[c], bias[c]) for c in range(3)])
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def probe(dtype, name, n):
    """Indices into values(dtype) of n samples for a small picture under the transform `name`: first those on which a
    competing model's byte differs from the contract's in some channel (up to n // 8 a model), then infinities, NaNs,
    zeros and subnormals, then samples with a byte inside 1..254.  Fixed for a given (dtype, name, n)."""
    want = bytes3(dtype, name)
    picked = []
    for m in MODELS:
        picked.append(np.flatnonzero((bytes3(dtype, name, m) != want).any(axis=0))[:max(n // 8, 1)])
    x = exact64(values(dtype))
    with np.errstate(all="ignore"):
        special = ~np.isfinite(x) | (np.abs(x) < MIN_NORMAL[dtype])
    picked.append(np.flatnonzero(special)[::max(int(special.sum()) // max(n // 8, 1), 1)][:n // 8])
    inside = np.flatnonzero(((want > 0) & (want < 255)).any(axis=0))
    picked.append(np.random.RandomState(n).permutation(inside))
    idx = np.concatenate(picked)
    _, first = np.unique(idx, return_index=True)
    return np.resize(idx[np.sort(first)], n)                  # (repeated from the start where the set has fewer)


def explain(dtype, scale, bias, t, got, want):
    """What a failing comparison says: the first differing bit pattern, the bytes got and wanted, and which competing
    model, if any, explains ALL differences.  t, got and want are flat and of one channel."""
    bad = np.flatnonzero(got != want)
    if len(bad) == 0:
        return "equal"
    i = int(bad[0])
    width = 8 if dtype == F32 else 4
    named = [name for name, fn in MODELS.items() if np.array_equal(fn(t, scale, bias), got)]
    return (f"{NAMES[dtype]} scale {scale!r} bias {bias!r}: {len(bad)} of {len(got)} samples differ; first at bits "
            f"0x{int(to_bits(t)[i]):0{width}x} (value {float(exact64(t)[i])!r}): got {int(got[i])}, want {int(want[i])}; "
            f"explained by: {', '.join(named) if named else 'no competing model'}")
