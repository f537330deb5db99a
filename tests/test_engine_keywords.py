"""Where the keywords of the Engine's full-style methods go (GPU).  The other GPU tests call most of these methods with
their defaults; here every keyword is given explicitly -- capacities (twice the default), offsets (the frames in
reversed order, 16-aligned), out (a slice of a larger tensor of sentinels), sizes / sizes_out, packed_capacity,
out_stride, a search per picture and metadata per picture -- and the call must write where it was told: the returned
tensors are the ones given, the frames lie at the given offsets, and every frame's bytes are those of the call that takes
the same search and metadata and leaves the rest to the defaults.  The same for out= of the six picture-making methods.

Two pictures, 17 x 9 (an odd width with a partial MCU) and 8 x 8 (a single block); for the YUV-plane formats NV12 frames
of 18 x 10 and 8 x 8."""
import numpy as np
import pytest
import torch

import sjpeg_amd as sj

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 64
MODE = sj.YUV_420
DIMS = [(17, 9), (8, 8)]
YUV_DIMS = [(18, 10), (8, 8)]
SIZES = [(9, 5), (8, 8)]                 # (stored orientation)
YUV_SIZES = [(10, 6), (8, 8)]
ORIENTS = [6, 1]
FACTORS = [2, 1]
SHEET = sj.Sheet(1, 1, (8, 8), background=(0x11, 0x7E, 0xEF))       # one picture a sheet: two sheets
EXIF = b"Exif\0\0II*\0\x08\0\0\0\0\0\0\0\0\0"
METADATA = [sj.PictureMetadata(exif=EXIF), None]
SEARCH = [dict(target_mode=sj.TARGET_PSNR, target_value=36.0, passes=4),
          sj.SearchParams(sj.TARGET_SIZE, 700.0, 3, 1.0, 0.0, 100.0)]


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


def _quant(q=75.0):
    m = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(float(q), m.ctypes.data)
    return m


def _upright(sizes, orientations):
    return [(h, w) if o >= 5 else (w, h) for (w, h), o in zip(sizes, orientations)]


@pytest.fixture(scope="module")
def families():
    """name -> (fmt, planes, dims, what stands between dims and yuv_mode, the sizes the pictures are coded at, whether the
    sizes tensor goes by `sizes_out`)"""
    rs = np.random.RandomState(20)
    rgb = [torch.from_numpy(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).cuda() for w, h in DIMS]
    rgba = [torch.from_numpy(rs.randint(0, 256, (h, w, 4)).astype(np.uint8)).cuda() for w, h in DIMS]
    planes = [[d.as_strided((d.shape[0], d.shape[1] * 3), (d.stride(0), 1))] for d in rgb]
    planes4 = [[d.as_strided((d.shape[0], d.shape[1] * 4), (d.stride(0), 1))] for d in rgba]
    nv12 = [[torch.from_numpy(rs.randint(0, 256, (h, w)).astype(np.uint8)).cuda(),
             torch.from_numpy(rs.randint(0, 256, ((h + 1) // 2, 2 * ((w + 1) // 2))).astype(np.uint8)).cuda()] for w, h in YUV_DIMS]
    flatten = sj.Flatten((200, 100, 50))
    sw, sh = sj.sheet_size(SHEET)
    return {
        "full": (sj.SRC_RGB, planes, DIMS, (), DIMS, False),
        "reduced": (sj.SRC_RGB, planes, DIMS, (FACTORS,), [sj.reduced_size(w, h, f) for (w, h), f in zip(DIMS, FACTORS)], False),
        "resized": (sj.SRC_RGB, planes, DIMS, (SIZES,), SIZES, True),
        "oriented": (sj.SRC_RGB, planes, DIMS, (SIZES, ORIENTS), _upright(SIZES, ORIENTS), True),
        "flattened": (sj.SRC_RGBA, planes4, DIMS, (flatten, SIZES, ORIENTS), _upright(SIZES, ORIENTS), True),
        "yuv_resized": (sj.SRC_NV12, nv12, YUV_DIMS, (YUV_SIZES, ORIENTS), _upright(YUV_SIZES, ORIENTS), True),
        "sheet": (sj.SRC_RGB, planes, DIMS, (SHEET, None, ORIENTS), [(sw, sh)] * 2, None),
    }


NAMES = ["full", "reduced", "resized", "oriented", "flattened", "yuv_resized", "sheet"]


def _bounds(coded, one_for_all=False):
    """the default capacities: the bound of every coded picture with room for its metadata"""
    msizes = [0 if m is None else m.size() for m in METADATA]
    if one_for_all:
        msizes = [max(msizes)] * len(msizes)
    return [sj.frame_bound(w, h, MODE, 2048 + ms) for (w, h), ms in zip(coded, msizes)]


def _host_frames(out, sizes, offsets):
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), [int(s) for s in sizes.cpu().numpy()]
    offs = [int(o) for o in (offsets.cpu().numpy() if hasattr(offsets, "cpu") else offsets)]
    assert all(s > 0 for s in sz), sz
    return [host[offs[k]:offs[k] + sz[k]].tobytes() for k in range(len(sz))], sz, offs


def _is_jpeg(frame):
    return frame[:2] == b"\xff\xd8" and frame[-2:] == b"\xff\xd9"


def _carries_the_routed_metadata(frames):
    assert EXIF in frames[0] and EXIF not in frames[1]


def _sentinels(nbytes):
    """a slice of nbytes at a multiple of 16 in the middle of a tensor of sentinels, and that tensor"""
    whole = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (whole.data_ptr() + GUARD) % 16 == 0
    return whole[GUARD:GUARD + nbytes], whole


def _guards_survive(whole, nbytes):
    host = whole.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + nbytes:] == SENTINEL).all()


@pytest.mark.parametrize("name", NAMES)
def test_unpacked_keywords(engine, families, name):
    fmt, planes, dims, special, coded, sizes_out = families[name]
    method = getattr(engine, f"encode_ragged_{name}")
    args = (fmt, planes, dims, *special, MODE, _quant())
    plain, _, _ = _host_frames(*method(*args)[:3])
    assert all(_is_jpeg(f) for f in plain)
    res = method(*args, search=SEARCH, metadata=METADATA)
    want, _, default_offsets = _host_frames(*res[:3])
    assert all(_is_jpeg(f) for f in want) and want != plain
    _carries_the_routed_metadata(want)
    n = len(want)
    if name == "sheet":
        stride = (_bounds(coded, True)[0] + 15) & ~15
        assert default_offsets == [0, stride]
        out, whole = _sentinels(n * (stride + 64))
        got = method(*args, search=SEARCH, metadata=METADATA, out_stride=stride + 64, out=out)
        offsets = [0, stride + 64]
    else:
        defaults = _bounds(coded)
        assert default_offsets == [0, (defaults[0] + 15) & ~15]
        capacities = [2 * c for c in defaults]
        offsets = [(capacities[1] + 15) & ~15, 0]                  # (the frames in reversed order)
        out, whole = _sentinels(offsets[0] + capacities[0])
        given_sizes = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        got = method(*args, search=SEARCH, metadata=METADATA, capacities=capacities, offsets=offsets, out=out,
                     **{"sizes_out" if sizes_out else "sizes": given_sizes})
        assert got[1] is given_sizes
    assert got[0] is out and list(got[2]) == offsets
    frames, sz, _ = _host_frames(*got[:3])
    assert frames == want
    assert got[3:] == res[3:]                                       # (modes, q and value of the search)
    _guards_survive(whole, out.numel())


@pytest.mark.parametrize("name", NAMES)
def test_packed_keywords(engine, families, name):
    fmt, planes, dims, special, coded, _ = families[name]
    method = getattr(engine, f"encode_ragged_{name}_packed")
    args = (fmt, planes, dims, *special, MODE, _quant())
    plain, _, _ = _host_frames(*method(*args)[:3])
    assert all(_is_jpeg(f) for f in plain)
    res = method(*args, search=SEARCH, metadata=METADATA)
    want, _, _ = _host_frames(res[0], res[1], res[2][:-1])
    assert all(_is_jpeg(f) for f in want) and want != plain
    _carries_the_routed_metadata(want)
    n = len(want)
    defaults = _bounds(coded, name == "sheet")
    packed_capacity = sum((2 * c + 15) & ~15 for c in defaults)
    out, whole = _sentinels(packed_capacity + 256)                  # (len(out) is NOT the capacity: the keyword is)
    keywords = dict(packed_capacity=packed_capacity, out=out)
    if name != "sheet":
        keywords["capacities"] = [2 * c for c in defaults]
    got = method(*args, search=SEARCH, metadata=METADATA, **keywords)
    assert got[0] is out
    frames, sz, offs = _host_frames(got[0], got[1], got[2])
    assert frames == want and got[3:] == res[3:]
    # back to back in the caller's order, each at a multiple of 16; offsets[n]: the bytes used
    at = 0
    for k in range(n):
        assert offs[k] == at
        at += (sz[k] + 15) & ~15
    assert offs[n] == at <= packed_capacity
    host = out.cpu().numpy()
    assert (host[packed_capacity:] == SENTINEL).all()
    _guards_survive(whole, out.numel())


def _same_pictures(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, tuple):
            assert all(torch.equal(a, b) for a, b in zip(g, w)) and len(g) == len(w)
        else:
            assert g.shape == w.shape and torch.equal(g, w)


@pytest.mark.parametrize("name", ["reduce_ragged", "resize_ragged", "orient_ragged", "flatten_ragged", "resize_ragged_yuv",
                                  "sheet_ragged"])
def test_picture_makers_out(engine, families, name):
    family, special = {"reduce_ragged": ("reduced", (FACTORS,)), "resize_ragged": ("resized", (SIZES,)),
                       "orient_ragged": ("oriented", (SIZES, ORIENTS)), "resize_ragged_yuv": ("yuv_resized", (YUV_SIZES, ORIENTS)),
                       "flatten_ragged": ("flattened", None), "sheet_ragged": ("sheet", None)}[name]
    fmt, planes, dims = families[family][:3]
    special = families[family][3] if special is None else special
    method = getattr(engine, name)
    rfmt, want, buf = method(fmt, planes, dims, *special)
    torch.cuda.synchronize()
    assert len(want) == 2
    out, whole = _sentinels(buf.numel() + 32)                       # (more than the bytes needed)
    got_fmt, got, got_buf = method(fmt, planes, dims, *special, out=out)
    torch.cuda.synchronize()
    assert got_fmt == rfmt and got_buf is out
    _same_pictures(got, want)
    lo, hi = out.data_ptr(), out.data_ptr() + buf.numel()
    for g in got:
        for p in (g if isinstance(g, tuple) else (g,)):
            assert lo <= p.data_ptr() < hi and p.data_ptr() % 16 == 0
    assert (out.cpu().numpy()[buf.numel():] == SENTINEL).all()
    _guards_survive(whole, out.numel())
