"""Contact sheets on the GPU (sjpeg_hip_sheet_ragged_src, sjpeg_hip_encode_ragged_sheet_src, make_sheets, encode_sheets,
encode_yuv_sheets).  The contract is sjpeg_hip.h's: a sheet is `background` everywhere except in the rectangles of its
thumbnails, which hold exactly the pictures of the orient / yuv-resize entries, and its JPEG is what encode_ragged_full
makes of that sheet.  The model is tests/sheet_model.py, in Python integers; every comparison is byte equality.  All
sources are noise, the background has three different non-zero bytes so that a slipped fill phase shows, and every made
buffer lies inside a larger tensor of sentinels that must survive."""
import os

import numpy as np
import pytest
import torch

import sheet_model as sm
import sjpeg_amd as sj
from test_reduce import F16, XFORM3, _on_device, _quant, _rgb_planes, _seen, _streams
from test_yuv_resize import _device_planes, _source

pytestmark = pytest.mark.gpu

BG = (0x11, 0x7E, 0xEF)
SENTINEL, GUARD = 0xA5, 64
YUV = {"nv12": sj.SRC_NV12, "nv21": sj.SRC_NV21, "yuv420": sj.SRC_YUV420, "yuv444": sj.SRC_YUV444}


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.fixture(scope="module")
def risk_table():
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        tab = f.read()
    sj.set_riskiness_table(tab)
    return tab


def _noise(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _grid(sheet):
    return sheet.cols, sheet.rows, sheet.cell, sheet.gutter, sheet.margin, sheet.background


def _orients(n, orientations):
    return [1] * n if orientations is None else list(orientations)


def _make(engine, fmt, planes, dims, sheet, sizes, orientations):
    """Engine.sheet_ragged into the middle of a tensor of sentinels, which survive; (out_fmt, sheets)"""
    frames, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
    st = sheet._struct()
    arr = None if sizes is None else np.ascontiguousarray(np.asarray(sizes, np.int32))
    oarr = None if orientations is None else np.ascontiguousarray(np.asarray(orientations, np.uint8))
    need = sj.lib().sjpeg_hip_sheet_ragged_bytes(fmt, len(dims), frames, sj.C.addressof(st), None if arr is None else arr.ctypes.data,
                                                 None if oarr is None else oarr.ctypes.data)
    assert need > 0 and need % 16 == 0, sj.last_error()
    whole = torch.full((need + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (whole.data_ptr() + GUARD) % 16 == 0
    rfmt, sheets, _ = engine.sheet_ragged(fmt, planes, dims, sheet, sizes, orientations, out=whole[GUARD:GUARD + need])
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + need:] == SENTINEL).all()
    return rfmt, sheets


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, want.shape, np.argwhere(got != want)[:6])


def _check_rgb(sheets, wants):
    assert len(sheets) == len(wants)
    for s, (got, want) in enumerate(zip(sheets, wants)):
        assert got.data_ptr() % 16 == 0 and got.stride(0) == (want.shape[1] * want.shape[2] + 3) // 4 * 4
        _same(got, want if got.dim() == 3 else want[..., 0], ("sheet", s))


def _check_yuv(sheets, wants):
    assert len(sheets) == len(wants)
    for s, (got, want) in enumerate(zip(sheets, wants)):
        assert len(got) == 3
        for c in range(3):
            assert got[c].data_ptr() % 16 == 0 and got[c].stride(0) == (want[c].shape[1] + 3) // 4 * 4
            _same(got[c], want[c], ("sheet", s, "plane", c))


def _rgb_case(engine, ims, sheet, sizes, orientations):
    """uint8 [H, W, 3] pictures through Engine.sheet_ragged against the model; (device sheets of the model, places)"""
    devs = [torch.from_numpy(im).cuda() for im in ims]
    planes, dims = _rgb_planes(devs)
    rfmt, sheets = _make(engine, sj.SRC_RGB, planes, dims, sheet, sizes, orientations)
    os_ = _orients(len(ims), orientations)
    given = sizes if sizes is not None else sm.fitted_sizes(dims, sheet.cell, os_)
    wants, where = sm.rgb_sheets(ims, *_grid(sheet), given, os_)
    assert rfmt == sj.SRC_RGB
    _check_rgb(sheets, wants)
    assert sj.sheet_places(sheet, dims, sj.SRC_RGB, sizes, orientations) == where
    return devs, wants, where


# ---- 1. RGB, unturned: every phase of the exact-span store and of the fill

@pytest.mark.parametrize("margin", [0, 1, 2, 3])
def test_rgb_unturned_every_phase(engine, margin):
    """Thumbnails 5 and 6 samples wide in cells 6 wide with gutter 1: over the four margins the span's first byte,
    3 * x0 (+ 12 for the second tile), takes every residue mod 4, and head and tail every value 0..3.  640 x 6 -> 5 x 3
    has tw = 4: two tiles across, whose seam and both neighbours' bytes lie in the 3 x 1 sheet."""
    sheet = sj.Sheet(3, 1, (6, 4), gutter=1, margin=margin, background=BG)
    ims = [_noise(640, 6, 11), _noise(37, 23, 12), _noise(20, 12, 13)]
    sizes = [(5, 3), (6, 4), (5, 3)]
    _, _, where = _rgb_case(engine, ims, sheet, sizes, None)
    starts = set((3 * x0) % 4 for _, x0, _, _, _ in where)
    assert len(starts) == 3 and where[0][1] == margin            # (three cells a margin; the four margins cover the rest)


def test_the_margins_cover_every_residue():
    seen = set()
    for margin in range(4):
        for i in range(3):
            seen.add((3 * (margin + 7 * i)) % 4)
            seen.add((3 * (margin + 7 * i) + 12) % 4)
    assert seen == {0, 1, 2, 3}


# ---- 2. all eight orientations in one sheet

def test_all_eight_orientations_in_one_sheet(engine):
    sheet = sj.Sheet(4, 2, (14, 14), gutter=1, margin=1, background=BG)
    ims = [_noise(37, 23, 20 + k) for k in range(8)]
    _rgb_case(engine, ims, sheet, [(13, 9)] * 8, list(range(1, 9)))
    # ... and fitted: 14 x 9 stored for 1..4, 14 x 9 stored in the turned box for 5..8
    _rgb_case(engine, ims, sheet, None, list(range(1, 9)))


# ---- 3. gray and float formats, a negative row stride

@pytest.mark.parametrize("name", ["GRAY", "GRAY_F16", "RGB_PLANAR_F16"])
def test_gray_and_float16_channel_first(engine, name):
    fmt, layout, dtype = {"GRAY": (sj.SRC_GRAY, "gray", None), "GRAY_F16": (sj.SRC_GRAY_F16, "gray", F16),
                          "RGB_PLANAR_F16": (sj.SRC_RGB_PLANAR_F16, "planar", F16)}[name]
    if dtype is not None:
        engine.set_pixel_transform(*XFORM3[dtype])
    sheet = sj.Sheet(3, 2, (14, 10), gutter=1, margin=2, background=BG)
    dims = [(37, 23), (23, 37), (16, 16), (5, 3), (640, 6)]
    orientations = [1, 6, 3, 1, 8]
    planes, keep, seen = [], [], []
    for k, (w, h) in enumerate(dims):
        p, dev, host = _on_device(_noise(w, h, 30 + k), layout, dtype, seed=k, off=k % 3, pad=k % 2)
        planes.append(p); keep.append(dev)
        s = _seen(host, layout, dtype)
        seen.append(s[..., None] if layout == "gray" else s)
    rfmt, sheets = _make(engine, fmt, planes, dims, sheet, None, orientations)
    engine.set_pixel_transform(255.0, 0.0)
    wants, _ = sm.rgb_sheets(seen, *_grid(sheet), sm.fitted_sizes(dims, sheet.cell, orientations), orientations)
    assert rfmt == (sj.SRC_GRAY if layout == "gray" else sj.SRC_RGB)
    _check_rgb(sheets, wants)


def test_bgra_with_a_negative_row_stride(engine):
    sheet = sj.Sheet(2, 2, (9, 7), gutter=3, margin=1, background=BG)
    dims, orientations = [(37, 23), (20, 12), (9, 7)], [1, 5, 2]
    ims = [_noise(w, h, 40 + k) for k, (w, h) in enumerate(dims)]
    devs, planes = [], []
    for im in ims:
        bgra = np.full(im.shape[:2] + (4,), 77, np.uint8)
        bgra[..., :3] = im[..., ::-1]
        d = torch.from_numpy(np.ascontiguousarray(bgra[::-1])).cuda()                    # stored bottom-up
        devs.append(d)
        planes.append([(d.data_ptr() + (d.shape[0] - 1) * d.stride(0), -d.stride(0))])
    rfmt, sheets = _make(engine, sj.SRC_BGRA, planes, dims, sheet, None, orientations)
    wants, _ = sm.rgb_sheets(ims, *_grid(sheet), sm.fitted_sizes(dims, sheet.cell, orientations), orientations)
    assert rfmt == sj.SRC_RGB
    _check_rgb(sheets, wants)


# ---- 4. the YUV-plane formats: all three sheet planes

# odd thumbnails (13 x 9, 1 x 1) in even cells; a turned frame; the chunked 20001 x 3 -> 4 x 2; a frame at cell size; a
# seventh frame, which opens a second sheet
YUV_DIMS = [(37, 23), (1, 1), (37, 23), (20001, 3), (20, 12), (14, 14), (37, 23)]
YUV_SIZES = [(13, 9), (1, 1), (13, 9), (4, 2), (10, 6), (14, 14), (9, 13)]
YUV_ORIENTS = [1, 1, 6, 1, 3, 1, 8]


@pytest.fixture(scope="module")
def yuv_batches():
    """per format: the frames' (y, u, v) arrays.  Computed once, never written to."""
    return {name: [_source(fmt, w, h, 5000 + 10 * k) for k, (w, h) in enumerate(YUV_DIMS)] for name, fmt in YUV.items()}


@pytest.mark.parametrize("name", list(YUV))
def test_yuv_formats_all_three_planes(engine, yuv_batches, name):
    fmt = YUV[name]
    sheet = sj.Sheet(3, 2, (14, 14), gutter=2, margin=2, background=BG)
    srcs = yuv_batches[name]
    planes = [_device_planes(fmt, s) for s in srcs]
    rfmt, sheets = _make(engine, fmt, planes, YUV_DIMS, sheet, YUV_SIZES, YUV_ORIENTS)
    wants, where = sm.yuv_sheets(name, srcs, *_grid(sheet), YUV_SIZES, YUV_ORIENTS)
    assert rfmt == (sj.SRC_YUV444 if name == "yuv444" else sj.SRC_YUV420) and len(sheets) == 2
    _check_yuv(sheets, wants)
    assert sj.sheet_places(sheet, YUV_DIMS, fmt, YUV_SIZES, YUV_ORIENTS) == where
    if name == "yuv444":                                     # no evenness rule: odd cells, gutter and margin
        odd = sj.Sheet(4, 2, (15, 13), gutter=1, margin=3, background=BG)
        rfmt, sheets = _make(engine, fmt, planes, YUV_DIMS, odd, YUV_SIZES[:5] + [(14, 13), (9, 13)], YUV_ORIENTS)
        wants, _ = sm.yuv_sheets(name, srcs, *_grid(odd), YUV_SIZES[:5] + [(14, 13), (9, 13)], YUV_ORIENTS)
        _check_yuv(sheets, wants)


# ---- 5. two sheets; frames already at cell size

def test_two_sheets_the_second_holds_one_thumbnail(engine):
    sheet = sj.Sheet(2, 2, (9, 7), gutter=1, margin=2, background=BG)
    ims = [_noise(37, 23, 60 + k) for k in range(5)]
    _, wants, where = _rgb_case(engine, ims, sheet, None, [1, 2, 1, 4, 1])
    assert len(wants) == 2 and [p[0] for p in where] == [0, 0, 0, 0, 1]
    rest = wants[1].copy()
    s, x0, y0, uw, uh = where[4]
    rest[y0:y0 + uh, x0:x0 + uw] = BG
    assert (rest == np.asarray(BG, np.uint8)).all()          # the unused cells of the last sheet are background


def test_frames_already_at_cell_size_are_copied(engine):
    """the kernel runs as an identity copy; with no gutter and no margin the sheet is the pictures side by side"""
    sheet = sj.Sheet(2, 2, (14, 14), gutter=0, margin=0, background=BG)
    ims = [_noise(14, 14, 70 + k) for k in range(4)]
    _, wants, _ = _rgb_case(engine, ims, sheet, None, None)
    assert np.array_equal(wants[0], np.vstack([np.hstack(ims[:2]), np.hstack(ims[2:])]))
    _rgb_case(engine, [_noise(5, 3, 75), _noise(6, 4, 76)], sj.Sheet(2, 1, (6, 4), gutter=1, margin=1, background=BG), None, None)


# ---- 6. the encodes: each against encode_ragged_full of the model's sheets, uploaded

@pytest.fixture(scope="module")
def rgb_batch():
    """five 37 x 23 noise pictures in 2 x 2 sheets of 16 x 12 cells: two sheets; the model's sheets on the device"""
    sheet = sj.Sheet(2, 2, (16, 12), gutter=2, margin=3, background=BG)
    ims = [_noise(37 + k, 23 + k, 80 + k) for k in range(5)]
    orientations = [1, 6, 3, 8, 2]
    dims = [(im.shape[1], im.shape[0]) for im in ims]
    wants, where = sm.rgb_sheets(ims, *_grid(sheet), sm.fitted_sizes(dims, sheet.cell, orientations), orientations)
    return sheet, [torch.from_numpy(im).cuda() for im in ims], orientations, [torch.from_numpy(np.ascontiguousarray(w)).cuda() for w in wants], where


def _both_entries(engine, fmt, planes, dims, sheet, sizes, orientations, mode, method, want, **kw):
    """encode_ragged_sheet and _packed give `want` = (streams, modes, q, value)"""
    out, szs, offs, modes, q, v = engine.encode_ragged_sheet(fmt, planes, dims, sheet, sizes, orientations, mode, _quant(), method, **kw)
    assert (_streams(out, szs, offs), modes, q, v) == want
    out, szs, offs, modes, q, v = engine.encode_ragged_sheet_packed(fmt, planes, dims, sheet, sizes, orientations, mode, _quant(), method, **kw)
    torch.cuda.synchronize()
    offs = offs.cpu().numpy()
    assert not int(offs[-1]) >> 63
    assert (_streams(out, szs, offs), modes, q, v) == want


def test_encode_rgb_auto_method_4(engine, risk_table, rgb_batch):
    sheet, devs, orientations, want_dev, _ = rgb_batch
    planes, dims = _rgb_planes(devs)
    uplanes, udims = _rgb_planes(want_dev)
    out, szs, offs, modes, q, v = engine.encode_ragged_full(sj.SRC_RGB, uplanes, udims, sj.YUV_AUTO, _quant(), 4)
    want = (_streams(out, szs, offs), modes, q, v)
    assert len(want[0]) == 2 and all(s[:2] == b"\xff\xd8" and s[-2:] == b"\xff\xd9" for s in want[0])
    _both_entries(engine, sj.SRC_RGB, planes, dims, sheet, None, orientations, sj.YUV_AUTO, 4, want)


def test_encode_with_a_target_size_per_sheet(engine, rgb_batch):
    sheet, devs, orientations, want_dev, _ = rgb_batch
    planes, dims = _rgb_planes(devs)
    uplanes, udims = _rgb_planes(want_dev)
    search = [dict(target_mode=sj.TARGET_SIZE, target_value=t) for t in (2600, 1800)]
    out, szs, offs, modes, q, v = engine.encode_ragged_full(sj.SRC_RGB, uplanes, udims, sj.YUV_420, _quant(), 4, search=search)
    want = (_streams(out, szs, offs), modes, q, v)
    _both_entries(engine, sj.SRC_RGB, planes, dims, sheet, None, orientations, sj.YUV_420, 4, want, search=search)


def test_encode_with_metadata_per_sheet(engine, rgb_batch):
    sheet, devs, orientations, want_dev, _ = rgb_batch
    planes, dims = _rgb_planes(devs)
    uplanes, udims = _rgb_planes(want_dev)
    metas = [sj.PictureMetadata(xmp=b"<x:xmpmeta>sheet %d</x:xmpmeta>" % s) for s in range(2)]
    out, szs, offs, modes, q, v = engine.encode_ragged_full(sj.SRC_RGB, uplanes, udims, sj.YUV_444, _quant(), 4, metadata=metas)
    want = (_streams(out, szs, offs), modes, q, v)
    assert b"sheet 0" in want[0][0] and b"sheet 1" in want[0][1]
    _both_entries(engine, sj.SRC_RGB, planes, dims, sheet, None, orientations, sj.YUV_444, 4, want, metadata=metas)


def test_encode_gray_400(engine):
    sheet = sj.Sheet(2, 1, (16, 12), gutter=1, margin=1, background=BG)
    grays = [np.ascontiguousarray(_noise(37, 23, 90 + k)[..., 1]) for k in range(3)]
    orientations = [1, 6, 4]
    devs = [torch.from_numpy(g).cuda() for g in grays]
    planes, dims = [[d] for d in devs], [(37, 23)] * 3
    wants, _ = sm.rgb_sheets([g[..., None] for g in grays], *_grid(sheet), sm.fitted_sizes(dims, sheet.cell, orientations), orientations)
    want_dev = [torch.from_numpy(np.ascontiguousarray(w[..., 0])).cuda() for w in wants]
    out, szs, offs, modes, q, v = engine.encode_ragged_full(sj.SRC_GRAY, [[w] for w in want_dev], [(w.shape[1], w.shape[0]) for w in want_dev],
                                                            sj.YUV_400, _quant(), 4)
    want = (_streams(out, szs, offs), modes, q, v)
    _both_entries(engine, sj.SRC_GRAY, planes, dims, sheet, None, orientations, sj.YUV_400, 4, want)
    with pytest.raises(sj.SjpegError, match="4:0:0 only"):
        engine.encode_ragged_sheet(sj.SRC_GRAY, planes, dims, sheet, None, orientations, sj.YUV_420, _quant(), 4)


def _yuv_want(engine, name, srcs, sheet, sizes, orientations, **kw):
    wants, where = sm.yuv_sheets(name, srcs, *_grid(sheet), sizes, orientations)
    dev = [[torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in w] for w in wants]
    out_fmt, mode = (sj.SRC_YUV444, sj.YUV_444) if name == "yuv444" else (sj.SRC_YUV420, sj.YUV_420)
    out, szs, offs, modes, q, v = engine.encode_ragged_full(out_fmt, dev, [(w[0].shape[1], w[0].shape[0]) for w in wants], mode, _quant(), 4, **kw)
    return (_streams(out, szs, offs), modes, q, v), where, mode


def test_encode_nv12_420(engine, yuv_batches):
    sheet = sj.Sheet(3, 2, (14, 14), gutter=2, margin=2, background=BG)
    srcs = yuv_batches["nv12"]
    planes = [_device_planes(sj.SRC_NV12, s) for s in srcs]
    want, _, mode = _yuv_want(engine, "nv12", srcs, sheet, YUV_SIZES, YUV_ORIENTS)
    _both_entries(engine, sj.SRC_NV12, planes, YUV_DIMS, sheet, YUV_SIZES, YUV_ORIENTS, mode, 4, want)


# ---- 7. the top-level calls, end to end

def test_encode_sheets_end_to_end(engine, risk_table, rgb_batch):
    sheet, devs, orientations, want_dev, where = rgb_batch
    want = sj.encode_images_full(want_dev, 75.0, sj.YUV_AUTO, 4, engine=engine)
    for packed in (False, True):
        got, places = sj.encode_sheets(devs, sheet, orientations=orientations, engine=engine, packed=packed)
        assert got == want and places == where
    made = sj.make_sheets(devs, sheet, orientations=orientations, engine=engine)
    torch.cuda.synchronize()
    for m, w in zip(made, want_dev):
        assert torch.equal(m, w)
    # a network's float output: [N, 3, H, W] float16 in 0..1
    batch = (torch.from_numpy(np.stack([_noise(20, 12, 95 + k) for k in range(3)])).cuda().permute(0, 3, 1, 2).to(torch.float16) / 255.0)
    seen = [np.rint(np.clip(b.permute(1, 2, 0).cpu().to(torch.float32).numpy().astype(np.float64) * 255.0, 0, 255)).astype(np.uint8) for b in batch]
    grid = sj.Sheet(3, 1, (10, 6), gutter=1, margin=1, background=BG)
    wants, _ = sm.rgb_sheets(seen, *_grid(grid), [(10, 6)] * 3, [1] * 3)
    made = sj.make_sheets(sj.FloatPixels(list(batch)), grid, engine=engine, layout="chw")
    engine.set_pixel_transform(255.0, 0.0)
    _check_rgb(made, wants)


def test_encode_yuv_sheets_end_to_end(engine, yuv_batches):
    sheet = sj.Sheet(3, 2, (14, 14), gutter=2, margin=2, background=BG)
    for name in ("nv12", "yuv444"):
        fmt, srcs = YUV[name], yuv_batches[name]
        frames = [tuple(_device_planes(fmt, s)) for s in srcs]
        want, where, _ = _yuv_want(engine, name, srcs, sheet, YUV_SIZES, YUV_ORIENTS)
        for packed in (False, True):
            got, places = sj.encode_yuv_sheets(frames, fmt, sheet, sizes=YUV_SIZES, orientations=YUV_ORIENTS, engine=engine, packed=packed)
            assert got == want[0] and places == where
    # sizes None: every frame fitted into its cell
    keep = [k for k in range(len(YUV_DIMS)) if YUV_DIMS[k][0] < 1000]
    srcs = [yuv_batches["nv12"][k] for k in keep]
    dims, orientations = [YUV_DIMS[k] for k in keep], [YUV_ORIENTS[k] for k in keep]
    frames = [tuple(_device_planes(sj.SRC_NV12, s)) for s in srcs]
    want, where, _ = _yuv_want(engine, "nv12", srcs, sheet, sm.fitted_sizes(dims, sheet.cell, orientations), orientations)
    got, places = sj.encode_yuv_sheets(frames, sj.SRC_NV12, sheet, orientations=orientations, engine=engine)
    assert got == want[0] and places == where


def test_scratch_bytes_and_trim(rgb_batch):
    """the sheets of the encode entries live in the engine memory of the reduced and resized pictures"""
    sheet, devs, orientations, want_dev, _ = rgb_batch
    eng = sj.Engine(0)
    planes, dims = _rgb_planes(devs)
    uplanes, udims = _rgb_planes(want_dev)
    eng.encode_ragged_full(sj.SRC_RGB, uplanes, udims, sj.YUV_420, _quant(), 4)       # (what the inner call takes is there already)
    torch.cuda.synchronize()
    before = eng.scratch_bytes()
    st = sheet._struct()
    frames, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
    oarr = np.ascontiguousarray(np.asarray(orientations, np.uint8))
    need = sj.lib().sjpeg_hip_sheet_ragged_bytes(sj.SRC_RGB, len(dims), frames, sj.C.addressof(st), None, oarr.ctypes.data)
    assert need > 0
    out, szs, offs, _, _, _ = eng.encode_ragged_sheet(sj.SRC_RGB, planes, dims, sheet, None, orientations, sj.YUV_420, _quant(), 4)
    _streams(out, szs, offs)
    after = eng.scratch_bytes()
    assert after >= before + need
    eng.trim()
    assert eng.scratch_bytes() <= after - need
    eng.close()
