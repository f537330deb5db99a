"""Video colour converted inside the ragged call on the GPU (sjpeg_hip_convert_ragged_yuv_src,
sjpeg_hip_encode_ragged_yuv_converted_src, the _yuv_colour sheet entries; sjpeg_amd.video).  The contract is
sjpeg_hip.h's: with P the planes sjpeg_hip_resize_ragged_yuv_src makes of a frame, the converted planes are
tests/yuv_colour_model.py's P' bit for bit, and a JPEG is what the existing calls make of P' handed over as planar
frames at their own size (the _full_meta_ call on them)."""
import numpy as np
import pytest
import torch

import sjpeg_amd as sj
import sjpeg_amd.video as sv
import yuv_colour_model as cm
from test_yuv_resize import _device_planes, _source

pytestmark = pytest.mark.gpu

FORMATS = {"yuv444": sj.SRC_YUV444, "yuv420": sj.SRC_YUV420, "nv12": sj.SRC_NV12, "nv21": sj.SRC_NV21}
CONVERTING = [s for s in cm.SOURCES if s != (cm.BT601, cm.FULL)]
# (source size, made size or None for its own, orientation): a turn with a resize; ratio 1; odd luma over cw = 5, ch = 3;
# one sample; the luma widths 9..16 at their own size -- cw mod 4 in {1, 2, 3, 0}, and for 9..12 a last luma dword that
# begins at the stride and must not be touched
CASES = [((18, 10), (10, 6), 6), ((8, 8), None, 1), ((17, 9), (9, 5), 1), ((1, 1), None, 1)] + [((w, 5), None, 1) for w in range(9, 17)]
SENTINEL = 0xA5


def _out_fmt(fmt):
    return sj.SRC_YUV444 if fmt == sj.SRC_YUV444 else sj.SRC_YUV420


def _colour(src):
    return sv.VideoColour(*src)


def _host(pics):
    torch.cuda.synchronize()
    return [[p.cpu().numpy().copy() for p in pic] for pic in pics]


def _frames_of(fmt, srcs):
    return [tuple(_device_planes(fmt, s)) for s in srcs]


def _planar(planes):
    """model planes as frames of the planar output format, on the device"""
    return [tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pic) for pic in planes]


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.fixture(scope="module")
def cases(engine):
    """per format: the frames of CASES on the device, their dims, sizes and orientations, and P -- what the resize entry
    makes of them today.  Computed once, never written to."""
    out = {}
    for name, fmt in FORMATS.items():
        dims = [c[0] for c in CASES]
        sizes = [c[1] if c[1] is not None else c[0] for c in CASES]
        orients = [c[2] for c in CASES]
        srcs = [_source(fmt, w, h, 5100 + 7 * k) for k, (w, h) in enumerate(dims)]
        frames = _frames_of(fmt, srcs)
        _, pics, _ = engine.resize_ragged_yuv(fmt, [list(f) for f in frames], dims, sizes, orients)
        out[name] = (frames, dims, sizes, orients, _host(pics))
    return out


def _check(pics, wants):
    got = _host(pics)
    assert len(got) == len(wants)
    for k, (g, w) in enumerate(zip(got, wants)):
        for c in range(3):
            assert g[c].shape == w[c].shape, (k, c, g[c].shape, w[c].shape)
            assert np.array_equal(g[c], w[c]), (k, c, w[c].shape, np.argwhere(g[c] != w[c])[:4])


# ---- 1. the planes and the JPEGs: every format, every converting source, one ragged call each

@pytest.mark.parametrize("src", CONVERTING, ids=[cm.NAMES[s] for s in CONVERTING])
@pytest.mark.parametrize("name", list(FORMATS))
def test_planes_and_jpegs_against_the_model(engine, cases, name, src):
    fmt = FORMATS[name]
    frames, dims, sizes, orients, P = cases[name]
    wants = [cm.convert_planes(*p, *src) for p in P]
    n = len(dims)
    cframes, _, _, _ = sj._ragged_frames([list(f) for f in frames], dims, None, None, None, None)
    arr = np.ascontiguousarray(np.asarray(sizes, np.int32))
    oarr = np.ascontiguousarray(np.asarray(orients, np.uint8))
    need = sj.lib().sjpeg_hip_resize_ragged_yuv_bytes(fmt, n, cframes, arr.ctypes.data, oarr.ctypes.data)
    guard = 256
    whole = torch.full((need + 2 * guard,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert need > 0 and (whole.data_ptr() + guard) % 16 == 0
    before = _host(frames)
    out_fmt, pics, _ = sv.convert_yuv_frames(frames, fmt, _colour(src), sizes=sizes, orientations=orients, engine=engine,
                                             out=whole[guard:guard + need])
    assert out_fmt == _out_fmt(fmt)
    _check(pics, wants)
    host = whole.cpu().numpy()
    assert (host[:guard] == SENTINEL).all() and (host[guard + need:] == SENTINEL).all()
    # the bytes between the planes' last rows and the next plane (plane padding) stay; row padding may be written
    for pic in pics:
        for p in pic:
            end = p.data_ptr() - whole.data_ptr() + p.stride(0) * p.shape[0]
            assert (host[end:(end + 15) & ~15] == SENTINEL).all()
    # the caller's planes were read, not written: the frames at ratio 1 too
    for b, a in zip(before, _host(frames)):
        assert all(np.array_equal(x, y) for x, y in zip(b, a))
    # one byte short is refused before anything runs
    with pytest.raises(sj.SjpegError, match="bytes"):
        sv.convert_yuv_frames(frames, fmt, _colour(src), sizes=sizes, orientations=orients, engine=engine, out=whole[guard:guard + need - 1])
    # the JPEGs: those of the model's planes
    got = sv.encode_video_frames(frames, fmt, _colour(src), sizes=sizes, orientations=orients, quality=80.0, engine=engine)
    want = sj.encode_yuv_frames(_planar(wants), _out_fmt(fmt), quality=80.0, engine=engine)
    assert all(len(w) > 0 for w in want) and got == want


# ---- 2. the eight orientations

@pytest.mark.parametrize("name", ["nv12", "yuv444"])
def test_one_frame_under_each_orientation(engine, name):
    fmt = FORMATS[name]
    src = _source(fmt, 11, 7, 5300)
    frames = _frames_of(fmt, [src] * 8)
    orients = list(range(1, 9))
    _, pics, _ = engine.resize_ragged_yuv(fmt, [list(f) for f in frames], [(11, 7)] * 8, None, orients)
    P = _host(pics)
    for s in CONVERTING:
        wants = [cm.convert_planes(*p, *s) for p in P]
        _, got, _ = sv.convert_yuv_frames(frames, fmt, _colour(s), orientations=orients, engine=engine)
        _check(got, wants)
        for k, g in enumerate(got):
            assert (g[0].shape[1], g[0].shape[0]) == sj.oriented_size(11, 7, orients[k])


# ---- 3. a designed frame: every luma value against the chroma extremes, so that both clamps and Y < 16 are met

@pytest.mark.parametrize("name", ["nv12", "yuv444"])
def test_designed_frame_hits_both_clamps(engine, name):
    fmt = FORMATS[name]
    vals = np.array([0, 16, 128, 240, 255], np.uint8)
    s = 1 if fmt == sj.SRC_YUV444 else 2
    crows, cw = 25, 256 // s
    y = np.tile(np.arange(256, dtype=np.uint8), (crows * s, 1))                    # a ramp of all 256 values
    u = np.repeat(vals[np.arange(crows) // 5][:, None], cw, axis=1)                # chroma rows at the five values,
    v = np.repeat(vals[np.arange(crows) % 5][:, None], cw, axis=1)                 # every pair of them
    frames = _frames_of(fmt, [[y, np.ascontiguousarray(u), np.ascontiguousarray(v)]])
    for src in CONVERTING:
        want = cm.convert_planes(y, u, v, *src)
        y0, k = cm.TABLES[src]
        raw = (k[0][0] * (y.astype(np.int64) - y0) + 8192) >> 14
        assert (raw < 0).any() == (y0 > 0) and (want[0] == 0).any() and (want[0] == 255).any()      # (Y < 16, both ends)
        assert (want[1] == 0).any() and (want[1] == 255).any() and (want[2] == 0).any() and (want[2] == 255).any()
        _, got, _ = sv.convert_yuv_frames(frames, fmt, _colour(src), engine=engine)
        _check(got, [want])


# ---- 4. a batch that mixes all four sources, per frame

@pytest.mark.parametrize("name", list(FORMATS))
def test_a_batch_mixing_all_four_sources(engine, cases, name):
    fmt = FORMATS[name]
    frames, dims, sizes, orients, P = cases[name]
    per = [cm.SOURCES[k % 4] for k in range(len(dims))]
    wants = [cm.convert_planes(*p, *s) for p, s in zip(P, per)]
    _, got, _ = sv.convert_yuv_frames(frames, fmt, [_colour(s) for s in per], sizes=sizes, orientations=orients, engine=engine)
    _check(got, wants)
    for k, s in enumerate(per):                      # (the identity frames: the resize entry's bytes)
        if s == (cm.BT601, cm.FULL):
            assert all(np.array_equal(w, p) for w, p in zip(wants[k], P[k]))
    jpegs = sv.encode_video_frames(frames, fmt, [_colour(s) for s in per], sizes=sizes, orientations=orients, engine=engine)
    assert jpegs == sj.encode_yuv_frames(_planar(wants), _out_fmt(fmt), engine=engine)
    plain = sj.encode_yuv_frames(frames, fmt, sizes=sizes, orientations=orients, engine=engine)
    for k, s in enumerate(per):                      # (the identity frames: the streams of the _yuv_resized_ entry)
        if s == (cm.BT601, cm.FULL):
            assert jpegs[k] == plain[k], k


# ---- 5. nothing to convert: the existing entries, byte for byte, and no memory of the engine's for it

@pytest.mark.parametrize("packed", [False, True])
def test_null_and_identity_are_the_existing_entries(cases, packed):
    frames, dims, sizes, orients, P = cases["nv12"]
    eng = sj.Engine(0)
    ident = sv.VideoColour("bt601", "full")
    assert ident.identity and not sv.VideoColour().identity
    want = sj.encode_yuv_frames(frames, sj.SRC_NV12, sizes=sizes, orientations=orients, packed=packed, engine=eng)
    own = sj.encode_yuv_frames(frames, sj.SRC_NV12, packed=packed, engine=eng)
    before = eng.scratch_bytes()
    for colour in (None, ident, [ident] * len(dims)):
        assert sv.encode_video_frames(frames, sj.SRC_NV12, colour, sizes=sizes, orientations=orients, packed=packed, engine=eng) == want
        # (at their own size and upright: the pass-through of the existing entry, no kernel at all)
        assert sv.encode_video_frames(frames, sj.SRC_NV12, colour, packed=packed, engine=eng) == own
    assert eng.scratch_bytes() == before
    _, got, _ = sv.convert_yuv_frames(frames, sj.SRC_NV12, None, sizes=sizes, orientations=orients, engine=eng)
    _check(got, P)
    _, got, _ = sv.convert_yuv_frames(frames, sj.SRC_NV12, [ident] * len(dims), sizes=sizes, orientations=orients, engine=eng)
    _check(got, P)
    assert eng.scratch_bytes() == before
    # ... and a converting call's descriptors are the engine's: counted, released by trim
    sv.encode_video_frames(frames, sj.SRC_NV12, sizes=sizes, orientations=orients, packed=packed, engine=eng)
    assert eng.scratch_bytes() > before
    eng.trim()
    assert eng.scratch_bytes() < before
    eng.close()


# ---- 6. sheets: only the thumbnails' rectangles are converted

def _sheet_case(fmt):
    """thumbnails of odd sizes whose chroma rectangles start at every phase of a dword, with gutter and margin"""
    if fmt == sj.SRC_YUV444:
        return sj.Sheet(4, 1, (11, 7), gutter=1, margin=3, background=(90, 40, 200)), [(5, 3), (9, 5), (7, 7), (3, 1), (11, 7), (1, 1)]
    return sj.Sheet(4, 1, (10, 6), gutter=2, margin=2, background=(90, 40, 200)), [(5, 3), (9, 5), (7, 5), (3, 1), (10, 6), (1, 1)]


@pytest.mark.parametrize("name", ["nv12", "yuv444"])
def test_sheets_convert_the_rectangles_alone(engine, name):
    fmt = FORMATS[name]
    sheet, sizes = _sheet_case(fmt)
    dims = [(2 * w + 1, 2 * h + 3) for (w, h) in sizes]
    orients = [1, 6, 3, 8, 1, 5]
    sizes = [(h, w) if o >= 5 else (w, h) for (w, h), o in zip(sizes, orients)]     # (sizes are in the STORED orientation)
    srcs = [_source(fmt, w, h, 5500 + k) for k, (w, h) in enumerate(dims)]
    frames = _frames_of(fmt, srcs)
    per = [CONVERTING[k % 3] for k in range(len(dims) - 1)] + [(cm.BT601, cm.FULL)]
    out_fmt, plain, _ = engine.sheet_ragged(fmt, [list(f) for f in frames], dims, sheet, sizes, orients)
    S = _host(plain)
    places = sj.sheet_places(sheet, dims, fmt, sizes, orients)
    s = 1 if fmt == sj.SRC_YUV444 else 2
    want = [[p.copy() for p in sh] for sh in S]
    leads = set()
    for (k, x0, y0, uw, uh), src in zip(places, per):
        cx, cy, cw, ch = x0 // s, y0 // s, (uw + s - 1) // s, (uh + s - 1) // s
        leads.add(cx % 4)
        rect = (S[k][0][y0:y0 + uh, x0:x0 + uw], S[k][1][cy:cy + ch, cx:cx + cw], S[k][2][cy:cy + ch, cx:cx + cw])
        yo, uo, vo = cm.convert_planes(*rect, *src)
        want[k][0][y0:y0 + uh, x0:x0 + uw] = yo
        want[k][1][cy:cy + ch, cx:cx + cw] = uo
        want[k][2][cy:cy + ch, cx:cx + cw] = vo
    assert leads == {0, 1, 2, 3} and len(S) == 2
    colours = [_colour(src) for src in per]
    fmt2, got, _ = sv.make_video_sheets(frames, fmt, sheet, colours, sizes=sizes, orientations=orients, engine=engine)
    assert fmt2 == out_fmt
    _check(got, want)                                # (inside the rectangles the model, outside them the existing entry's bytes)
    jpegs, where = sv.encode_video_sheets(frames, fmt, sheet, colours, sizes=sizes, orientations=orients, quality=85.0, engine=engine)
    assert where == places
    assert jpegs == sj.encode_yuv_frames(_planar(want), out_fmt, quality=85.0, engine=engine)
    packed, _ = sv.encode_video_sheets(frames, fmt, sheet, colours, sizes=sizes, orientations=orients, quality=85.0, packed=True, engine=engine)
    assert packed == jpegs
    # nothing to convert: the existing sheet call
    same, _ = sv.encode_video_sheets(frames, fmt, sheet, None, sizes=sizes, orientations=orients, quality=85.0, engine=engine)
    assert same == sj.encode_yuv_sheets(frames, fmt, sheet, sizes=sizes, orientations=orients, quality=85.0, engine=engine)[0]


# ---- 7. packed output and a per-frame target size through the new encode entries

@pytest.mark.parametrize("name", ["nv12", "yuv444"])
def test_packed_output_and_target_sizes(engine, cases, name):
    fmt = FORMATS[name]
    frames, dims, sizes, orients, P = cases[name]
    src = (cm.BT709, cm.LIMITED)
    wants = _planar([cm.convert_planes(*p, *src) for p in P])
    targets = [300 + 10 * (k % 5) for k in range(len(dims))]
    for kw in (dict(), dict(target_size=targets)):
        want = sj.encode_yuv_frames(wants, _out_fmt(fmt), **kw, engine=engine)
        assert sv.encode_video_frames(frames, fmt, _colour(src), sizes=sizes, orientations=orients, packed=True, **kw, engine=engine) == want
        assert sv.encode_video_frames(frames, fmt, _colour(src), sizes=sizes, orientations=orients, **kw, engine=engine) == want
