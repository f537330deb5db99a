"""10-bit video in the ragged call on the GPU (sjpeg_hip_convert_ragged_yuv16_src and the other _yuv16 entries;
sjpeg_amd.video's *_deep_* functions).  The contract is sjpeg_hip.h's: a made sample is the exact area average of the
16-bit WORDS of its cell, divided by 2^shift, rounded half up once and clamped to 255; everything behind the made planes
is the 8-bit contract.  The planes are compared to tests/yuv16_model.py (Python integers), the JPEGs to what the existing
8-bit entry makes of the model's planes.  Every comparison is byte equality.  The shapes are the smallest at which the
kernel's deep path can go wrong: odd sizes and chroma of (w + 1) / 2, trailing elements and dword tails, segments at
and above the stage's capacity in samples (8192) and in pairs (4096), every orientation, rows that run backwards."""
import numpy as np
import pytest
import torch

import sjpeg_amd as sj
import sjpeg_amd.video as sv
import sheet_model as sm
import yuv16_model as dm
import yuv_colour_model as cm

pytestmark = pytest.mark.gpu

FORMATS = {"yuv444": sj.SRC_YUV444, "yuv420": sj.SRC_YUV420, "nv12": sj.SRC_NV12, "nv21": sj.SRC_NV21}
DEPTHS = {2: sv.VideoDepth.YUV10, 8: sv.VideoDepth.P010}
BT709 = (cm.BT709, cm.LIMITED)
SENTINEL = 0x5A5A
# (source size, made size): own size and about 2 / 3
TAILS = [((1, 1), (1, 1)), ((2, 2), (2, 2)), ((3, 5), (3, 5)), ((17, 9), (17, 9)),
         ((1, 1), (1, 1)), ((2, 2), (1, 1)), ((3, 5), (2, 3)), ((17, 9), (11, 6))]


def _out_fmt(fmt):
    return sj.SRC_YUV444 if fmt == sj.SRC_YUV444 else sj.SRC_YUV420


def _source(kind, w, h, seed, shift, top=None):
    """(y, u, v) uint16 planes of a w x h frame: noise over the depth's whole scale (top: up to this word instead)"""
    rs = np.random.RandomState(seed)
    cw, ch = dm.chroma_size(kind, w, h)
    hi = (256 << shift) if top is None else top + 1
    return [rs.randint(0, hi, (h, w)).astype(np.uint16), rs.randint(0, hi, (ch, cw)).astype(np.uint16),
            rs.randint(0, hi, (ch, cw)).astype(np.uint16)]


def _tensor(a, unsigned=False):
    """a uint16 array on the device: int16 bits, or torch's own uint16"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if unsigned else a.view(np.int16)).cuda()


def _device(kind, yuv, pairs3=False, unsigned=False):
    """the caller's planes of a frame: (y, uv) for the semi-planar kinds (nv21: V first; pairs3: [rows, pairs, 2]),
    else (y, u, v)"""
    y, u, v = yuv
    if kind in ("nv12", "nv21"):
        first, second = (u, v) if kind == "nv12" else (v, u)
        uv = np.stack([first, second], axis=-1)
        return (_tensor(y, unsigned), _tensor(uv if pairs3 else uv.reshape(u.shape[0], 2 * u.shape[1]), unsigned))
    return tuple(_tensor(p, unsigned) for p in yuv)


def _host(pics):
    torch.cuda.synchronize()
    return [[p.cpu().numpy().copy() for p in pic] for pic in pics]


def _planar(planes):
    return [tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pic) for pic in planes]


def _check(pics, wants):
    got = _host(pics)
    assert len(got) == len(wants)
    for k, (g, w) in enumerate(zip(got, wants)):
        for c in range(3):
            assert g[c].shape == w[c].shape, (k, c, g[c].shape, w[c].shape)
            assert np.array_equal(g[c], w[c]), (k, c, w[c].shape, np.argwhere(g[c] != w[c])[:4])


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


# ---- 1. tails: every format, low- and high-aligned samples, one ragged call each

@pytest.mark.parametrize("shift", [2, 8])
@pytest.mark.parametrize("kind", list(FORMATS))
def test_tails_planes_and_jpegs_against_the_model(engine, kind, shift):
    fmt, depth = FORMATS[kind], DEPTHS[shift]
    dims, sizes = [c[0] for c in TAILS], [c[1] for c in TAILS]
    # (the last frame: bits above the nominal depth take part as they are, the clamp bounds the result)
    srcs = [_source(kind, w, h, 6100 + 13 * k + shift, shift, top=0xffff if k == len(dims) - 1 else None) for k, (w, h) in enumerate(dims)]
    frames = [_device(kind, s, pairs3=k % 2 == 1, unsigned=k == 3 and hasattr(torch, "uint16")) for k, s in enumerate(srcs)]
    wants = [dm.made_planes(s, kind, size, shift) for s, size in zip(srcs, sizes)]
    assert any((w[0] == 255).any() for w in wants) and any((w[0] < 255).all() for w in wants)
    before = _host(frames)
    out_fmt, pics, _ = sv.convert_deep_frames(frames, fmt, None, sizes=sizes, engine=engine, depth=depth)
    assert out_fmt == _out_fmt(fmt)
    _check(pics, wants)
    for b, a in zip(before, _host(frames)):          # the caller's planes were read, not written
        assert all(np.array_equal(x, y) for x, y in zip(b, a))
    got = sv.encode_deep_video_frames(frames, fmt, None, sizes=sizes, quality=80.0, engine=engine, depth=depth)
    want = sj.encode_yuv_frames(_planar(wants), _out_fmt(fmt), quality=80.0, engine=engine)
    assert all(len(w) > 0 for w in want) and got == want
    # ... and with the colour put right behind the made planes
    wants = [dm.made_planes(s, kind, size, shift, colour=BT709) for s, size in zip(srcs, sizes)]
    _, pics, _ = sv.convert_deep_frames(frames, fmt, sizes=sizes, engine=engine, depth=depth)
    _check(pics, wants)
    # own sizes without sizes: no pass-through, the same kernel
    _, pics, _ = sv.convert_deep_frames(frames[:4], fmt, None, engine=engine, depth=depth)
    _check(pics, [[dm.own_size(p, shift) for p in s] for s in srcs[:4]])


# ---- 2. constant planes at full scale: the clamp

@pytest.mark.parametrize("shift,word", [(8, 0xffff), (2, 1023)])
def test_full_scale_planes_meet_the_clamp(engine, shift, word):
    yuv = [np.full((9, 17), word, np.uint16), np.full((5, 9), word, np.uint16), np.full((5, 9), word, np.uint16)]
    assert (2 * word * 4 + (4 << shift)) // (4 << (shift + 1)) == 256          # 256 before the clamp
    frames = [_device("nv12", yuv)] * 2
    sizes = [(17, 9), (11, 6)]
    wants = [dm.made_planes(yuv, "nv12", s, shift) for s in sizes]
    assert all((p == 255).all() for w in wants for p in w)
    _, pics, _ = sv.convert_deep_frames(frames, sj.SRC_NV12, None, sizes=sizes, engine=engine, depth=DEPTHS[shift])
    _check(pics, wants)


# ---- 3. rounding once, not per sample

def test_rounding_happens_once_behind_the_average(engine):
    rs = np.random.RandomState(77)
    vals = np.array([0x7f, 0x80, 0x17f, 0x180], np.uint16)
    y = vals[rs.randint(0, 4, (8, 8))]
    y[0:2, 0:2] = [[0x7f, 0x80], [0x7f, 0x80]]       # a cell that averages to 0x7f.8: 0, but 1 where each sample is rounded first
    yuv = [y, vals[rs.randint(0, 4, (8, 8))], vals[rs.randint(0, 4, (8, 8))]]
    want = dm.made_planes(yuv, "yuv444", (4, 4), 8)
    cheap = [dm.narrowed_then_averaged(p, 4, 4, 8) for p in yuv]
    assert want[0][0, 0] == 0 and cheap[0][0, 0] == 1
    assert any((w != c).any() for w, c in zip(want, cheap))
    _, pics, _ = sv.convert_deep_frames([_device("yuv444", yuv)], sj.SRC_YUV444, None, sizes=[(4, 4)], engine=engine)
    _check(pics, [want])


# ---- 4. segments longer than the stage: chunks of one row, from half the width of the 8-bit path

@pytest.fixture(scope="module")
def wide():
    """frames whose tiles' segments lie at and above the stage's capacity: 8192 samples of a one-channel plane, 4096
    pairs of a UV plane.  (width, height, made size); the model is computed once"""
    cases = [(20000, 3, (3, 2)), (8192, 2, (1, 1)), (8194, 2, (1, 1))]
    srcs = [_source("nv12", w, h, 6400 + k, 8) for k, (w, h, _) in enumerate(cases)]
    wants = [dm.made_planes(s, "nv12", size, 8) for s, (_, _, size) in zip(srcs, cases)]
    return cases, srcs, wants


@pytest.mark.parametrize("kind", ["nv12", "nv21", "yuv420"])
def test_the_chunked_path_of_luma_and_of_the_pair_plane(engine, wide, kind):
    cases, srcs, wants = wide
    # (20000 x 3 -> 3 x 2: one tile of the Y plane spans 20000 samples, one of the UV plane 10000 pairs -> 2 columns;
    #  8192 wide: 8192 samples and 4096 pairs, exactly the capacities; 8194 wide: 8194 and 4097, one chunk more)
    frames = [_device(kind, s) for s in srcs]
    _, pics, _ = sv.convert_deep_frames(frames, FORMATS[kind], None, sizes=[c[2] for c in cases], engine=engine)
    _check(pics, wants)                              # (U and V are the same planes under all three kinds)


# ---- 5. the eight orientations

@pytest.mark.parametrize("kind", ["nv12", "yuv444"])
def test_one_frame_under_each_orientation(engine, kind):
    fmt = FORMATS[kind]
    src = _source(kind, 37, 23, 6500, 8)
    frames = [_device(kind, src)] * 8
    orients = list(range(1, 9))
    upright = dm.made_planes(src, kind, (19, 11), 8)
    wants = [[np.ascontiguousarray(sm._turn(p, o)) for p in upright] for o in orients]
    _, pics, _ = sv.convert_deep_frames(frames, fmt, None, sizes=[(19, 11)] * 8, orientations=orients, engine=engine)
    _check(pics, wants)
    for k, g in enumerate(pics):
        assert (g[0].shape[1], g[0].shape[0]) == sj.oriented_size(19, 11, orients[k])
    jpegs = sv.encode_deep_video_frames(frames, fmt, None, sizes=[(19, 11)] * 8, orientations=orients, engine=engine)
    assert jpegs == sj.encode_yuv_frames(_planar(wants), _out_fmt(fmt), engine=engine)


# ---- 6. rows that run backwards, rows with padding

def _bottom_up(t):
    """a plane stored bottom-up inside a larger tensor of sentinels: (address of row 0, negative stride in bytes), the tensor"""
    rows, n = t.shape
    big = torch.full((rows + 2, n + 7), SENTINEL, dtype=torch.int16, device="cuda")
    big[1:rows + 1, 3:3 + n] = t.flip(0)
    return (big.data_ptr() + 2 * (rows * big.stride(0) + 3), -2 * big.stride(0)), big


def _padded(t):
    rows, n = t.shape
    big = torch.full((rows + 2, n + 13), SENTINEL, dtype=torch.int16, device="cuda")
    big[1:rows + 1, 5:5 + n] = t
    return big[1:rows + 1, 5:5 + n], big


@pytest.mark.parametrize("kind", ["nv12", "yuv420"])
def test_negative_and_padded_row_strides(engine, kind):
    fmt = FORMATS[kind]
    src = _source(kind, 17, 9, 6600, 8)
    want = dm.made_planes(src, kind, (11, 6), 8)
    tight = _device(kind, src)
    up = [_bottom_up(p) for p in tight]
    pad = [_padded(p) for p in tight]
    assert all(addr % 2 == 0 and stride % 2 == 0 and stride < 0 for (addr, stride), _ in up)
    # (the binding's reader takes tensors: frames of (address, stride) planes go to the C entry by the engine's own helpers)
    for planes in ([p for p, _ in pad],):
        _, pics, _ = sv.convert_deep_frames([tuple(planes)], fmt, None, sizes=[(11, 6)], engine=engine)
        _check(pics, [want])
    planes, dims = [[a for a, _ in up]], [(17, 9)]
    cframes, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
    arr = np.asarray([(11, 6)], np.int32)
    L = sv._lib()
    need = L.sjpeg_hip_resize_ragged_yuv_bytes(fmt, 1, cframes, arr.ctypes.data, None)
    out = torch.zeros(need, dtype=torch.uint8, device="cuda")
    made, rfmt = (sj.RaggedFrame * 1)(), sj.C.c_int(-1)
    st = sv.VideoDepth.P010._struct()
    engine._chk(L.sjpeg_hip_convert_ragged_yuv16_src(engine._h, fmt, 1, cframes, arr.ctypes.data, None, None, 0, sj.C.addressof(st),
                                                     out.data_ptr(), need, made, sj.C.byref(rfmt), engine._stream()), "convert")
    _check(sj._frame_views(out, made, rfmt.value), [want])
    for (_, big), t in zip(up + pad, list(tight) * 2):        # the sentinels around the planes stand
        host = big.cpu().numpy().view(np.uint16)
        assert (host == SENTINEL).sum() >= host.size - t.numel()


# ---- 7. contact sheets: the rectangles are the model's, the background stays

@pytest.mark.parametrize("colour", [None, BT709], ids=["as-is", "bt709-limited"])
def test_sheets_of_p010_frames(engine, colour):
    sheet = sj.Sheet(2, 2, (20, 14), gutter=2, margin=2, background=(90, 40, 200))
    dims, orients = [(40, 24)] * 4, [1, 6, 3, 8]
    srcs = [_source("nv12", 40, 24, 6700 + k, 8) for k in range(4)]
    frames = [_device("nv12", s, pairs3=k % 2 == 0) for k, s in enumerate(srcs)]
    sizes = sm.fitted_sizes(dims, (20, 14), orients)
    want, where = dm.sheets("nv12", srcs, 2, 2, (20, 14), 2, 2, (90, 40, 200), sizes, orients, 8, None if colour is None else [colour] * 4)
    assert len(want) == 1 and (want[0][0] == 90).any() and (want[0][1] == 40).any()
    vc = None if colour is None else sv.VideoColour("bt709", "limited")
    out_fmt, got, _ = sv.make_deep_video_sheets(frames, sj.SRC_NV12, sheet, vc, orientations=orients, engine=engine)
    assert out_fmt == sj.SRC_YUV420
    _check(got, want)
    jpegs, places = sv.encode_deep_video_sheets(frames, sj.SRC_NV12, sheet, vc, orientations=orients, quality=85.0, engine=engine)
    assert [tuple(p) for p in places] == [tuple(p) for p in where]
    assert jpegs == sj.encode_yuv_frames(_planar(want), sj.SRC_YUV420, quality=85.0, engine=engine)
    packed, _ = sv.encode_deep_video_sheets(frames, sj.SRC_NV12, sheet, vc, orientations=orients, quality=85.0, packed=True, engine=engine)
    assert packed == jpegs


# ---- 8. ragged batches: mixed sizes, per-frame colour, packed and unpacked, a per-frame target size

@pytest.mark.parametrize("kind,shift", [("nv12", 8), ("yuv420", 2)])
def test_mixed_batches_packed_and_searched(engine, kind, shift):
    fmt, depth = FORMATS[kind], DEPTHS[shift]
    dims = [(64, 48), (33, 21), (8, 8), (120, 30), (17, 9)]
    sizes = [(32, 24), (33, 21), (5, 7), (40, 10), (9, 5)]
    orients = [1, 6, 1, 3, 8]
    per = [cm.SOURCES[k % 4] for k in range(len(dims))]
    srcs = [_source(kind, w, h, 6800 + k, shift) for k, (w, h) in enumerate(dims)]
    frames = [_device(kind, s) for s in srcs]
    wants = [dm.made_planes(s, kind, size, shift, o, c) for s, size, o, c in zip(srcs, sizes, orients, per)]
    colours = [sv.VideoColour(*c) for c in per]
    _, pics, _ = sv.convert_deep_frames(frames, fmt, colours, sizes=sizes, orientations=orients, engine=engine, depth=depth)
    _check(pics, wants)
    planar = _planar(wants)
    targets = [300 + 10 * (k % 5) for k in range(len(dims))]
    for kw in (dict(), dict(target_size=targets)):
        want = sj.encode_yuv_frames(planar, _out_fmt(fmt), **kw, engine=engine)
        for packed in (False, True):
            got = sv.encode_deep_video_frames(frames, fmt, colours, sizes=sizes, orientations=orients, packed=packed, **kw, engine=engine,
                                              depth=depth)
            assert got == want, (kw.keys(), packed)


# ---- 9. the 8-bit path beside it, on one engine

def test_an_8_bit_call_is_the_same_before_and_after_a_deep_call():
    eng = sj.Engine(0)
    rs = np.random.RandomState(6900)
    y8, uv8 = rs.randint(0, 256, (24, 40)).astype(np.uint8), rs.randint(0, 256, (12, 40)).astype(np.uint8)
    frames8 = [(torch.from_numpy(y8).cuda(), torch.from_numpy(uv8).cuda())] * 2
    kw = dict(sizes=[(20, 12), (13, 9)], orientations=[1, 6], engine=eng)
    before = sv.encode_video_frames(frames8, sj.SRC_NV12, **kw)
    _, planes_before, _ = sv.convert_yuv_frames(frames8, sj.SRC_NV12, **kw)
    planes_before = _host(planes_before)
    src = _source("nv12", 40, 24, 6901, 8)
    deep = sv.encode_deep_video_frames([_device("nv12", src)] * 3, sj.SRC_NV12, sizes=[(20, 12), (40, 24), (7, 5)], engine=eng)
    assert len(deep) == 3 and all(deep)
    assert sv.encode_video_frames(frames8, sj.SRC_NV12, **kw) == before
    _, planes_after, _ = sv.convert_yuv_frames(frames8, sj.SRC_NV12, **kw)
    _check(planes_after, planes_before)
    # ... and the deep call of the bytes shifted up is the 8-bit call's answer: (b << 8) / 256 = b, exactly
    y16, uv16 = (y8.astype(np.uint16) << 8), (uv8.astype(np.uint16) << 8)
    frames16 = [(_tensor(y16), _tensor(uv16))] * 2
    assert sv.encode_deep_video_frames(frames16, sj.SRC_NV12, **kw) == before
    eng.close()
