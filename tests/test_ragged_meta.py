"""Per-picture metadata in ragged batches (sjpeg_hip_encode_ragged_full_meta_src and its packed twin): the splice identity
against the call without metadata, the reference's answers of tests/golden/ragged_meta.json (size searches that count the
metadata among them), the 16-byte header copy at every destination alignment and around its 2048-byte threshold against
the parent's path (sjpeg_hip_encode_ragged_src with ready headers), capacity, invalid metadata, and the Python entries.

The golden cases run in one mixed batch per method AND sampling (a call has one yuv_mode): every batch holds frames
that are not searched, frames searched for a PSNR and frames searched for a size."""
import ctypes as C
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
Q = 75.0
OVERFLOW = 1 << 63
SIZES = [(1, 1), (17, 13), (64, 64), (250, 130), (97, 61)]
NOTE = b'xmpNote:HasExtendedXMP="' + b"0" * 32 + b'"'


def _rand(n, seed):
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8).tobytes()


# every frame different metadata; frame 1 none; frame 3 extended XMP (main packet + extension chunks)
METAS = [sj.PictureMetadata(exif=_rand(700, 1), iccp=_rand(3000, 2)),
         None,
         sj.PictureMetadata(app_markers=b"\xff\xe3\x00\x0a" + _rand(8, 3), xmp=b"<x:xmpmeta>" + b"b" * 900),
         sj.PictureMetadata(xmp=b"<x:xmpmeta " + NOTE + b">" + b"c" * 70000),
         sj.PictureMetadata(iccp=_rand(70000, 4), exif=_rand(64, 5))]


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.fixture(scope="module")
def risk_table():
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        sj.set_riskiness_table(f.read())


def _imgs(sizes=SIZES):
    return [(synth.g_struct if k % 2 == 0 else synth.g_noise)(w, h, 5000 + k) for k, (w, h) in enumerate(sizes)]


def _dev(imgs, pad=16):
    out = []
    for im in imgs:
        h, w, _ = im.shape
        buf = np.zeros((h, 3 * w + pad), np.uint8)
        buf[:, :3 * w] = im.reshape(h, 3 * w)
        out.append([torch.from_numpy(buf).cuda()[:, :3 * w]])
    return out


def _dims(imgs):
    return [(im.shape[1], im.shape[0]) for im in imgs]


def _quant(q=Q):
    m = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(float(q), m.ctypes.data)
    return m


def _block(meta):
    """The metadata block: what make_header_meta puts behind byte 20."""
    if meta is None:
        return b""
    q = _quant()
    with_meta = sj.make_header_meta(8, 8, sj.YUV_420, q, None, meta.app_markers, meta.exif, meta.iccp, meta.xmp, meta.xmp_split_point)
    return with_meta[20:20 + len(with_meta) - len(sj.make_header_ex(8, 8, sj.YUV_420, q, None))]


def _frames(out, sizes, offsets):
    torch.cuda.synchronize()
    sz = [int(s) for s in sizes.cpu().numpy()]
    host = out.cpu().numpy()
    return [host[int(o):int(o) + s].tobytes() for o, s in zip(list(offsets), sz)]


def _packed_frames(out, sizes, offsets):
    torch.cuda.synchronize()
    sz, off = sizes.cpu().numpy(), offsets.cpu().numpy()
    host = out.cpu().numpy()
    n = len(sz)
    for k in range(n):
        assert int(off[k]) % 16 == 0
        end = int(off[k]) + int(sz[k])
        assert not host[end:(end + 15) & ~15].any(), "the padding behind a frame is zero"
    return [host[int(off[k]):int(off[k]) + int(sz[k])].tobytes() for k in range(n)], int(off[n])


# ---- 1. the splice identity
@pytest.mark.parametrize("method", [0, 4, 7])
@pytest.mark.parametrize("yuv_mode", [sj.YUV_AUTO, sj.YUV_420])
def test_splice_identity(engine, risk_table, method, yuv_mode):
    imgs = _imgs()
    planes, dims = _dev(imgs), _dims(imgs)
    out, sizes, offs, modes, _, _ = engine.encode_ragged_full(sj.SRC_RGB, planes, dims, yuv_mode, _quant(), method)
    bare = _frames(out, sizes, offs)
    want = [b[:20] + _block(m) + b[20:] for b, m in zip(bare, METAS)]
    out, sizes, offs, modes_m, _, _ = engine.encode_ragged_full(sj.SRC_RGB, planes, dims, yuv_mode, _quant(), method, metadata=METAS)
    assert _frames(out, sizes, offs) == want and modes_m == modes
    out, sizes, offs, modes_p, _, _ = engine.encode_ragged_full_packed(sj.SRC_RGB, planes, dims, yuv_mode, _quant(), method,
                                                                       metadata=METAS)
    got, used = _packed_frames(out, sizes, offs)
    assert sorted(got) == sorted(want) and got == want and used < OVERFLOW
    # meta_per_frame = 0: every frame carries the one entry
    one = METAS[0]
    out, sizes, offs, _, _, _ = engine.encode_ragged_full(sj.SRC_RGB, planes, dims, yuv_mode, _quant(), method, metadata=one)
    assert _frames(out, sizes, offs) == [b[:20] + _block(one) + b[20:] for b in bare]


def test_null_metadata_is_the_call_without(engine):
    imgs = _imgs()
    planes, dims = _dev(imgs), _dims(imgs)
    q = _quant()
    caps = [sj.frame_bound(w, h, sj.YUV_420, 2048) for (w, h) in dims]
    frames, out, sizes, offs = sj._ragged_frames(planes, dims, caps, None, None, None)
    params = sj.RaggedParams(sj.YUV_420, 4, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    st = sj.Engine._stream()
    out.fill_(0xA5)
    assert sj.lib().sjpeg_hip_encode_ragged_full_src(engine._h, sj.SRC_RGB, len(dims), frames, C.byref(params), out.data_ptr(),
                                                     sizes.data_ptr(), None, None, None, st) == 0
    torch.cuda.synchronize()
    want, want_sizes = out.cpu().numpy().copy(), sizes.cpu().numpy().copy()
    out.fill_(0xA5)
    sizes.zero_()
    assert sj.lib().sjpeg_hip_encode_ragged_full_meta_src(engine._h, sj.SRC_RGB, len(dims), frames, C.byref(params), None, 1,
                                                          out.data_ptr(), sizes.data_ptr(), None, None, None, st) == 0
    torch.cuda.synchronize()
    assert (sizes.cpu().numpy() == want_sizes).all() and (out.cpu().numpy() == want).all()


# ---- 2. the reference's answers
def _golden():
    spec = importlib.util.spec_from_file_location("make_ragged_meta", os.path.join(HERE, "golden", "make_ragged_meta.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(HERE, "golden", "ragged_meta.json")) as f:
        return mod, json.load(f)["cases"]


@pytest.mark.parametrize("method", [0, 4, 8])
@pytest.mark.parametrize("yuv_mode", [sj.YUV_AUTO, sj.YUV_420, sj.YUV_400])
def test_golden_answers(engine, risk_table, method, yuv_mode):
    mod, cases = _golden()
    cases = [c for c in cases if c["method"] == method and c["yuv_mode"] == yuv_mode]
    assert {c["target_mode"] for c in cases} >= {0, 1, 2}
    imgs = [np.ascontiguousarray(getattr(synth, c["gen"])(c["w"], c["h"], c["seed"])) for c in cases]
    metas = [sj.PictureMetadata(**mod.metadata_of(c["meta"])) for c in cases]
    search = [sj.SearchParams(c["target_mode"] or 1, c["target_value"], c["passes"], c["tolerance"], c["qmin"], c["qmax"])
              for c in cases]
    for packed in (False, True):
        fn = engine.encode_ragged_full_packed if packed else engine.encode_ragged_full
        res = fn(sj.SRC_RGB, _dev(imgs), _dims(imgs), yuv_mode, _quant(cases[0]["quality"]), method, search=search, metadata=metas)
        got = _packed_frames(res[0], res[1], res[2])[0] if packed else _frames(res[0], res[1], res[2])
        for k, c in enumerate(cases):
            assert (len(got[k]), hashlib.md5(got[k]).hexdigest()) == (c["size"], c["md5"]), (packed, k, c)


# ---- 3. the wide copy
HEADER_SIZES = [2047, 2048, 2049, 2050, 2063, 2064, 2065, 70000]


def _meta_for_header(total, bare):
    """EXIF (and an ICC profile where one APP1 is too short) that makes the header `total` bytes long."""
    need = total - bare
    if need <= 60000:
        return sj.PictureMetadata(exif=_rand(need - 10, need))
    return sj.PictureMetadata(exif=_rand(1000, 7), iccp=_rand(need - 1010 - 2 * 18, 8))


@pytest.mark.parametrize("shift", [0, 5])
def test_wide_header_copy_at_every_alignment(engine, shift):
    n = 16
    imgs = [synth.g_noise(8, 8, 6000 + k) for k in range(n)]
    planes, dims = _dev(imgs), _dims(imgs)
    q = _quant()
    bare = len(sj.make_header_ex(8, 8, sj.YUV_420, q, None))
    metas = [_meta_for_header(HEADER_SIZES[(k + shift) % len(HEADER_SIZES)], bare) for k in range(n)]
    headers = [sj.make_header_meta(8, 8, sj.YUV_420, q, None, m.app_markers, m.exif, m.iccp, m.xmp) for m in metas]
    assert [len(h) for h in headers] == [HEADER_SIZES[(k + shift) % len(HEADER_SIZES)] for k in range(n)]
    caps = [sj.frame_bound(8, 8, sj.YUV_420, len(h)) for h in headers]
    gap = 64
    offsets, at = [], gap
    for k in range(n):                                   # frame k starts at k modulo 16
        at = ((at + 15) & ~15) + k
        offsets.append(at)
        at += caps[k] + gap
    total = at + gap
    tables, _ = sj.make_tables(quality=Q)
    ref_out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    _, ref_sizes, _ = engine.encode_ragged(sj.SRC_RGB, planes, dims, sj.YUV_420, tables, headers, capacities=caps, out=ref_out,
                                           offsets=offsets)
    want = _frames(ref_out, ref_sizes, offsets)
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    _, sizes, _, _, _, _ = engine.encode_ragged_full(sj.SRC_RGB, planes, dims, sj.YUV_420, q, 0, capacities=caps, out=out,
                                                     offsets=offsets, metadata=metas)
    got = _frames(out, sizes, offsets)
    assert got == want
    assert all(g[:len(h)] == h for g, h in zip(got, headers))
    # nothing but the frames was written: the sentinel stands in front of, between and behind them
    host = out.cpu().numpy()
    mask = np.ones(total, bool)
    for o, g in zip(offsets, got):
        mask[o:o + len(g)] = False
    assert (host[mask] == 0xA5).all()
    # packed: every frame at a multiple of 16
    res = engine.encode_ragged_full_packed(sj.SRC_RGB, planes, dims, sj.YUV_420, q, 0, capacities=caps, metadata=metas)
    assert _packed_frames(res[0], res[1], res[2])[0] == want


def test_one_mebibyte_profile(engine):
    img = synth.g_struct(8, 8, 6100)
    meta = sj.PictureMetadata(iccp=_rand(1 << 20, 9))
    q = _quant()
    out, sizes, offs, _, _, _ = engine.encode_ragged_full(sj.SRC_RGB, _dev([img]), [(8, 8)], sj.YUV_420, q, 0, metadata=[meta])
    got = _frames(out, sizes, offs)[0]
    out, sizes, offs, _, _, _ = engine.encode_ragged_full(sj.SRC_RGB, _dev([img]), [(8, 8)], sj.YUV_420, q, 0)
    bare = _frames(out, sizes, offs)[0]
    assert got == bare[:20] + _block(meta) + bare[20:] and len(got) > (1 << 20)


# ---- 4. capacity
def test_a_frame_one_byte_short_reports_zero(engine):
    imgs = _imgs()
    planes, dims = _dev(imgs), _dims(imgs)
    q = _quant()
    out, sizes, offs, _, _, _ = engine.encode_ragged_full(sj.SRC_RGB, planes, dims, sj.YUV_420, q, 4, metadata=METAS)
    want = _frames(out, sizes, offs)
    caps = [sj.frame_bound(w, h, sj.YUV_420, 2048 + (m.size() if m else 0)) for (w, h), m in zip(dims, METAS)]
    caps[4] = len(want[4]) - 1
    out, sizes, offs, _, _, _ = engine.encode_ragged_full(sj.SRC_RGB, planes, dims, sj.YUV_420, q, 4, capacities=caps, metadata=METAS)
    torch.cuda.synchronize()
    assert int(sizes[4]) == 0
    got = _frames(out, sizes, offs)
    assert [g for k, g in enumerate(got) if k != 4] == [w for k, w in enumerate(want) if k != 4]
    # packed: a pool that ends inside the last frame sets bit 63 and names the bytes a second try needs
    need = sum((len(w) + 15) & ~15 for w in want)
    res = engine.encode_ragged_full_packed(sj.SRC_RGB, planes, dims, sj.YUV_420, q, 4, metadata=METAS, packed_capacity=need - 16,
                                           out=torch.zeros(need, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    end = int(res[2][len(dims)]) & 0xFFFFFFFFFFFFFFFF
    assert end & OVERFLOW and (end & ~OVERFLOW) == need
    assert int(res[1][4]) == 0 and [int(s) for s in res[1][:4]] == [len(w) for w in want[:4]]


# ---- 5. invalid metadata
def test_invalid_metadata_names_the_frame_before_any_device_work(engine):
    imgs = _imgs(SIZES[:4])
    planes, dims = _dev(imgs), _dims(imgs)
    metas = [sj.PictureMetadata(exif=b"ok"), None, sj.PictureMetadata(exif=b"\0" * 65530), None]
    arr = (sj.Metadata * 4)(*[(m or sj.PictureMetadata())._struct() for m in metas])
    q = _quant()
    caps = [sj.frame_bound(w, h, sj.YUV_420, 2048 + 70000) for (w, h) in dims]
    frames, out, sizes, offs = sj._ragged_frames(planes, dims, caps, None, None, None)
    out.fill_(0xA5)
    params = sj.RaggedParams(sj.YUV_420, 4, q.ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    rc = sj.lib().sjpeg_hip_encode_ragged_full_meta_src(engine._h, sj.SRC_RGB, 4, frames, C.byref(params), C.cast(arr, C.c_void_p), 1,
                                                        out.data_ptr(), sizes.data_ptr(), None, None, None, sj.Engine._stream())
    assert rc == -1
    msg = sj.lib().sjpeg_hip_last_error().decode()
    assert "meta[2] (frame 2): exif" in msg and msg.startswith("sjpeg_hip_encode_ragged_full_meta_src: "), msg
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all() and not sizes.cpu().numpy().any()


# ---- 6. Python
def test_python_entry_points_give_the_engine_calls_bytes(engine, risk_table):
    imgs = _imgs()
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    planes, dims = _dev(imgs), _dims(imgs)
    for yuv_mode, method, kw in ((sj.YUV_420, 0, {}), (sj.YUV_420, 4, {}), (sj.YUV_AUTO, 4, {}), (sj.YUV_420, 4, dict(target_size=9000))):
        search = None
        if kw:
            search = [sj.SearchParams(sj.TARGET_SIZE, 9000.0, 10, 1.0, 0.0, 100.0)] * len(imgs)
        out, sizes, offs, _, _, _ = engine.encode_ragged_full(sj.SRC_RGB, planes, dims, yuv_mode, _quant(), method, search=search,
                                                              metadata=METAS)
        want = _frames(out, sizes, offs)
        assert sj.encode_images(dev, Q, yuv_mode, engine=engine, method=method, metadata=METAS, **kw) == want
        assert sj.encode_images(dev, Q, yuv_mode, engine=engine, method=method, metadata=METAS, packed=True, **kw) == want
        assert sj.encode_images_full_meta(dev, METAS, quality=Q, yuv_mode=yuv_mode, method=method, engine=engine, **kw) == want
        chw = [d.permute(2, 0, 1).contiguous() for d in dev]
        assert sj.encode_images_full_meta(chw, METAS, layout="chw", quality=Q, yuv_mode=yuv_mode, method=method, engine=engine,
                                          packed=True, **kw) == want
        assert sj.encode_images(chw, Q, yuv_mode, engine=engine, method=method, metadata=METAS, layout="chw", **kw) == want
    out, sizes, offs, _, _, _ = engine.encode_ragged_full(sj.SRC_RGB, planes, dims, sj.YUV_AUTO, _quant(), 4, metadata=METAS[0])
    assert sj.compress_images(dev, Q, engine=engine, metadata=METAS[0]) == _frames(out, sizes, offs)


# ---- 7. several launches: the staged headers
def test_staged_headers_over_several_launches(monkeypatch):
    """A limit of one byte makes every frame a launch of its own, so every launch stages its headers afresh in the engine's
    buffer and finds them by its own offsets; a limit between one and two of the large headers cuts the launches by the
    header bytes alone.  The bytes are those of the one-launch call; the staging buffer shows in scratch_bytes and goes
    with trim."""
    imgs = _imgs()
    planes, dims = _dev(imgs), _dims(imgs)
    eng = sj.Engine(0)
    out, sizes, offs, _, _, _ = eng.encode_ragged_full(sj.SRC_RGB, planes, dims, sj.YUV_420, _quant(), 4, metadata=METAS)
    want = _frames(out, sizes, offs)
    eng.close()
    monkeypatch.setenv("SJPEG_HIP_SCRATCH_LIMIT_BYTES", "1")
    eng = sj.Engine(0)                                        # (made after the limit is set)
    for packed in (False, True):
        fn = eng.encode_ragged_full_packed if packed else eng.encode_ragged_full
        res = fn(sj.SRC_RGB, planes, dims, sj.YUV_420, _quant(), 4, metadata=METAS)
        got = _packed_frames(res[0], res[1], res[2])[0] if packed else _frames(res[0], res[1], res[2])
        assert got == want, packed
    # the largest header of the call (frame 3 or 4: about 70 KB) is staged: the buffer is counted, and trim frees it
    held = eng.scratch_bytes()
    assert held >= max(m.size() for m in METAS if m)
    eng.trim()
    assert eng.scratch_bytes() < max(m.size() for m in METAS if m)
    eng.close()
    # sixteen 8 x 8 frames with 70 000-byte headers: a launch a frame, launches of a few frames (the header bytes count
    # against the limit), one launch (the headers travel with the call's one upload) -- the same bytes
    n = 16
    small = [synth.g_noise(8, 8, 6200 + k) for k in range(n)]
    metas = [sj.PictureMetadata(iccp=_rand(69000 + k, 20 + k)) for k in range(n)]
    eng = sj.Engine(0)                                        # (still the limit of one byte: one launch a frame)
    out, sizes, offs, _, _, _ = eng.encode_ragged_full(sj.SRC_RGB, _dev(small), _dims(small), sj.YUV_420, _quant(), 0, metadata=metas)
    each = _frames(out, sizes, offs)
    eng.close()
    monkeypatch.setenv("SJPEG_HIP_SCRATCH_LIMIT_BYTES", "200000")
    eng = sj.Engine(0)
    out, sizes, offs, _, _, _ = eng.encode_ragged_full(sj.SRC_RGB, _dev(small), _dims(small), sj.YUV_420, _quant(), 0, metadata=metas)
    assert _frames(out, sizes, offs) == each
    eng.close()
    monkeypatch.delenv("SJPEG_HIP_SCRATCH_LIMIT_BYTES")
    eng = sj.Engine(0)
    out, sizes, offs, _, _, _ = eng.encode_ragged_full(sj.SRC_RGB, _dev(small), _dims(small), sj.YUV_420, _quant(), 0, metadata=metas)
    got = _frames(out, sizes, offs)
    eng.close()
    assert got == each
    for g, m in zip(got, metas):
        assert g[20:20 + m.size()] == _block(m)


def test_one_entry_for_all_frames_packed(engine):
    imgs = _imgs()
    planes, dims = _dev(imgs), _dims(imgs)
    one = METAS[4]
    out, sizes, offs, _, _, _ = engine.encode_ragged_full(sj.SRC_RGB, planes, dims, sj.YUV_420, _quant(), 4)
    want = [b[:20] + _block(one) + b[20:] for b in _frames(out, sizes, offs)]
    res = engine.encode_ragged_full_packed(sj.SRC_RGB, planes, dims, sj.YUV_420, _quant(), 4, metadata=one)
    assert _packed_frames(res[0], res[1], res[2])[0] == want
