"""Ragged batches with trellis quantization (sjpeg_hip_encode_ragged_trellis_src, methods 7 and 8): every frame of every
batch against the oracle or the host API of the same build, byte for byte -- small pictures, wide kept blocks, large
frames, parameters, layouts, AUTO / SHARP, capacity, parts, concurrency, bad arguments and the Python keyword."""
import os
import threading

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(1, 1), (7, 13), (17, 13), (64, 64), (250, 130), (1, 300), (300, 1), (97, 61), (33, 200)]
MODES = [sj.YUV_420, sj.YUV_444, sj.YUV_400]
MIXED = [(128, 128), (1, 1), (7, 13), (300, 1), (17, 130), (250, 130), (97, 61), (640, 480), (64, 64), (33, 200),
         (211, 97), (80, 64), (70, 50), (60, 90), (1920, 1080), (5, 300)]


def _content(k, w, h):
    if k % 3 == 0:
        return synth.g_struct(w, h, 1000 + k)
    if k % 3 == 1:
        return synth.g_noise(w, h, 2000 + k)
    return np.full((h, w, 3), (37 * k) % 256, np.uint8)


def _gradient(w, h):
    x = np.arange(w)[None, :] * 200 // w
    y = np.arange(h)[:, None] * 200 // h
    return np.stack([np.broadcast_to(x + 20, (h, w)), np.broadcast_to(y + 30, (h, w)), np.full((h, w), 90)],
                    2).astype(np.uint8)


def _auto_content(k, w, h):
    """The pictures of test_ragged_auto.py: their verdicts cover 4:2:0, sharp, 4:4:4 and 4:0:0."""
    rng = np.random.RandomState(500 + k)
    kind = k % 5
    if kind == 4:
        return _gradient(w, h)
    if kind == 0:
        return synth.g_struct(w, h, 1000 + k)
    if kind == 1:
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == 2:
        return np.repeat(rng.randint(0, 256, (h, w, 1)), 3, 2).astype(np.uint8)
    return (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def _mixed():
    imgs = [_auto_content(k, w, h) for k, (w, h) in enumerate(MIXED)]
    imgs[0] = np.fromfile(os.path.join(ROOT, "tests", "golden", "test128.rgb"), np.uint8).reshape(128, 128, 3)
    return imgs


def _dev(imgs, pad=16):
    """One device allocation per picture, rows padded by `pad` bytes: [rows, 3 w] views."""
    out = []
    for im in imgs:
        h, w, _ = im.shape
        buf = np.zeros((h, 3 * w + pad), np.uint8)
        buf[:, :3 * w] = im.reshape(h, 3 * w)
        out.append([torch.from_numpy(buf).cuda()[:, :3 * w]])
    return out


def _dims(imgs):
    return [(im.shape[1], im.shape[0]) for im in imgs]


def _quant(q):
    m = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(float(q), m.ctypes.data)
    return m


def _frames(out, sizes, offs):
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    sz = sizes.cpu().numpy()
    return [host[o:o + int(s)].tobytes() if s > 0 else b"" for o, s in zip(offs, sz)]


def _trellis(eng, imgs, q, mode, method=7, **kw):
    quant = [_quant(qq) for qq in q] if isinstance(q, list) else _quant(q)
    out, sizes, offs, modes = eng.encode_ragged_trellis(sj.SRC_RGB, _dev(imgs), _dims(imgs), mode, quant, method, **kw)
    return _frames(out, sizes, offs), modes


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.fixture(scope="module")
def risk_table():
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        tab = f.read()
    assert len(tab) == 117649
    sj.set_riskiness_table(tab)
    return tab


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("method", [7, 8])
def test_every_frame_equals_the_oracle(engine, oracle, mode, method):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(SMALL)]
    for q in (5.0, 50.0, 75.0, 95.0):
        got, modes = _trellis(engine, imgs, q, mode, method)
        assert modes == [mode] * len(imgs)
        for k, im in enumerate(imgs):
            assert got[k] == oracle.encode_method(im, q, mode, method), (mode, method, q, k, im.shape)


def test_the_trellis_really_ran(engine, oracle):
    im = synth.g_struct(250, 130, 1004)
    got7, _ = _trellis(engine, [im], 75.0, sj.YUV_420, 7)
    got4 = _frames(*engine.encode_ragged_batch(sj.SRC_RGB, _dev([im]), _dims([im]), sj.YUV_420, _quant(75.0), 4))
    assert got7[0] == oracle.encode_method(im, 75.0, sj.YUV_420, 7)
    assert got4[0] == oracle.encode_method(im, 75.0, sj.YUV_420, 4)
    assert got7[0] != got4[0]


def test_wide_kept_blocks_and_the_checked_walk(engine, oracle):
    """Noise at q 97 and 100: levels above 127 (the two-plane kept block) and blocks past the lean walk's bound, which
    comes from the codes of the pass that CODES a replayed block (the cases of
    test_gpu_parity.py::test_replayed_blocks_are_classified_by_the_coding_tables, as frames among thumbnails)."""
    rng = np.random.RandomState(77)
    for (w, h, q, method, mode) in ((215, 279, 100.0, 7, 1), (331, 257, 97.0, 8, 1), (260, 190, 100.0, 8, 3),
                                   (300, 200, 100.0, 7, 1), (180, 260, 97.0, 7, 3), (200, 150, 100.0, 7, 4)):
        imgs = [synth.g_struct(33, 17, 1), rng.randint(0, 256, (h, w, 3)).astype(np.uint8), synth.g_noise(1, 1, 2),
                synth.g_struct(w, h, 5 + w), synth.g_noise(40, 40, 3), synth.g_noise(w, h, 9)]
        got, _ = _trellis(engine, imgs, q, mode, method)
        for k, im in enumerate(imgs):
            assert got[k] == oracle.encode_method(im, q, mode, method), (w, h, q, method, mode, k)


@pytest.mark.parametrize("method", [7, 8])
def test_large_frames_equal_the_host_api(engine, method):
    imgs = [synth.g_struct(31, 17, 1), synth.g_struct(1920, 1080, 5), synth.g_noise(3840, 2160, 6), synth.g_noise(7, 7, 2),
            synth.g_struct(3840, 2160, 7), synth.g_noise(1920, 1080, 8), synth.g_struct(64, 64, 3)]
    got, _ = _trellis(engine, imgs, 75.0, sj.YUV_420, method)
    for k, im in enumerate(imgs):
        assert got[k] == sj.SjpegEncode(im, 75.0, method, sj.YUV_420), (method, k)
    if method == 7:
        for mode in (sj.YUV_444, sj.YUV_400):
            got, _ = _trellis(engine, imgs[:3], 75.0, mode, method)
            for k, im in enumerate(imgs[:3]):
                assert got[k] == sj.SjpegEncode(im, 75.0, method, mode), (mode, k)


def test_per_frame_quality_min_quant_q_bias_and_qdelta(engine, oracle):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate([(33, 21), (640, 480), (16, 16), (250, 130), (97, 61)])]
    quals = [5.0, 50.0, 75.0, 90.0, 100.0]
    for mode in (sj.YUV_420, sj.YUV_400):
        got, _ = _trellis(engine, imgs, quals, mode, 7)
        for k, im in enumerate(imgs):
            assert got[k] == oracle.encode_full(im, _quant(quals[k]), yuv_mode=mode, method=7), (mode, k)
    mq = np.full((2, 64), 6, np.uint8)
    got, _ = _trellis(engine, imgs, quals, sj.YUV_420, 7, min_quant=mq, q_bias=0x60, dmax_luma=4, dmax_chroma=-2)
    for k, im in enumerate(imgs):
        want = oracle.encode_full(im, _quant(quals[k]), mq, 0x60, 4, -2, yuv_mode=sj.YUV_420, method=7)
        assert got[k] == want, k
    got, _ = _trellis(engine, imgs, 60.0, sj.YUV_444, 7, min_quant=mq, q_bias=0x40, dmax_luma=0, dmax_chroma=12)
    for k, im in enumerate(imgs):
        want = oracle.encode_full(im, _quant(60.0), mq, 0x40, 0, 12, yuv_mode=sj.YUV_444, method=7)
        assert got[k] == want, k


def _layout_planes(rng, fmt, w, h):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    shapes = {1: [(h, 4 * w)], 2: [(h, 4 * w)], 3: [(h, w)], 4: [(h, w)] * 3,
              5: [(h, w), (ch, cw), (ch, cw)], 6: [(h, w), (ch, 2 * cw)], 7: [(h, w), (ch, 2 * cw)]}[fmt]
    return [(rng.randint(0, 64, s) + np.arange(s[1])[None, :] // 3).astype(np.uint8) for s in shapes]


@pytest.mark.parametrize("fmt", [1, 2, 3, 4, 5, 6, 7])
def test_source_layouts(engine, oracle, fmt):
    rng = np.random.RandomState(500 + fmt)
    mode = {3: sj.YUV_400, 4: sj.YUV_444}.get(fmt, sj.YUV_420)
    dims = [(1, 1), (17, 13), (250, 130), (40, 9), (97, 61)]
    host = [_layout_planes(rng, fmt, w, h) for (w, h) in dims]
    dev, keep = [], []
    for k, planes in enumerate(host):
        fr = []
        for p in planes:
            padded = np.zeros((p.shape[0], p.shape[1] + 24), np.uint8)
            padded[:, :p.shape[1]] = p
            if k == 2:
                # bottom-up: row 0 is the allocation's last row, the stride is negative
                t = torch.from_numpy(np.ascontiguousarray(padded[::-1])).cuda()
                keep.append(t)
                fr.append((t.data_ptr() + (p.shape[0] - 1) * padded.shape[1], -padded.shape[1]))
            else:
                fr.append(torch.from_numpy(padded).cuda()[:, :p.shape[1]])
        dev.append(fr)
    out, sizes, offs, _ = engine.encode_ragged_trellis(fmt, dev, dims, mode, _quant(70.0), 7)
    got = _frames(out, sizes, offs)
    for k, (w, h) in enumerate(dims):
        want = oracle.encode_src(fmt, host[k], w, h, _quant(70.0), yuv_mode=mode, method=7)
        assert got[k] == want, (fmt, k, w, h)


@pytest.mark.parametrize("yuv_mode", [sj.YUV_AUTO, sj.YUV_SHARP])
def test_auto_and_sharp_equal_the_host_api(engine, oracle, risk_table, yuv_mode):
    imgs = _mixed()
    verdicts = [oracle.riskiness(im, risk_table)[0] for im in imgs]
    assert {sj.YUV_420, sj.YUV_SHARP, sj.YUV_444, sj.YUV_400} <= set(verdicts), verdicts
    got, modes = _trellis(engine, imgs, 75.0, yuv_mode, 7)
    assert modes == (verdicts if yuv_mode == sj.YUV_AUTO else [sj.YUV_SHARP] * len(imgs))
    for k, im in enumerate(imgs):
        assert got[k] == sj.SjpegEncode(im, 75.0, 7, yuv_mode), (yuv_mode, k, im.shape, modes[k])


def test_capacity_and_canary(engine):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate([(64, 64), (250, 130), (97, 61), (640, 480)])]
    mode = sj.YUV_420
    caps = [sj.frame_bound(w, h, mode, 2048) for (w, h) in _dims(imgs)]
    caps[1] = 700                                          # far too small for frame 1
    offs, at = [], 64
    for c in caps:
        offs.append(at)
        at += c + 48                                       # gaps between the ranges
    out = torch.full((at + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out, sizes, _, _ = engine.encode_ragged_trellis(sj.SRC_RGB, _dev(imgs), _dims(imgs), mode, _quant(90.0), 7,
                                                    capacities=caps, out=out, offsets=offs)
    torch.cuda.synchronize()
    sz = sizes.cpu().numpy()
    host = out.cpu().numpy()
    assert sz[1] == 0
    for k in (0, 2, 3):
        assert host[offs[k]:offs[k] + sz[k]].tobytes() == sj.SjpegEncode(imgs[k], 90.0, 7, mode), k
    inside = np.zeros(host.size, bool)
    for o, c in zip(offs, caps):
        inside[o:o + c] = True
    assert (host[~inside] == 0xA5).all()


def _thumbs(n, seed):
    rng = np.random.RandomState(seed)
    imgs = []
    for k in range(n):
        w, h = int(rng.randint(1, 97)), int(rng.randint(1, 97))
        imgs.append(synth.g_noise(w, h, k) if k % 2 else synth.g_struct(w, h, k))
    return imgs


def test_every_frame_its_own_part(monkeypatch, risk_table):
    imgs = _thumbs(60, 31)
    imgs.insert(20, synth.g_struct(1920, 1080, 3))
    imgs.append(synth.g_noise(640, 480, 4))
    eng = sj.Engine(0)
    want, _ = _trellis(eng, imgs, 75.0, sj.YUV_420, 7)
    whole = eng.scratch_bytes()
    mixed = _mixed()
    want_auto, modes_auto = _trellis(eng, mixed, 75.0, sj.YUV_AUTO, 7)
    eng.close()
    monkeypatch.setenv("SJPEG_HIP_SCRATCH_LIMIT_BYTES", "1")
    small = sj.Engine(0)                                   # (made after the limit is set: every frame its own part)
    got, _ = _trellis(small, imgs, 75.0, sj.YUV_420, 7)
    assert got == want
    assert small.scratch_bytes() < whole                   # (a part's scratch is one frame's)
    for k in list(range(0, len(imgs), 7)) + [20, len(imgs) - 1]:
        assert want[k] == sj.SjpegEncode(imgs[k], 75.0, 7, sj.YUV_420), k
    got_auto, modes = _trellis(small, mixed, 75.0, sj.YUV_AUTO, 7)
    assert got_auto == want_auto and modes == modes_auto
    small.close()


def test_pipelined_engine():
    eng = sj.Engine(0)
    eng.set_pipelined(True)
    a = synth.g_struct(640, 360, 1)
    frames = torch.from_numpy(a).cuda().unsqueeze(0)
    want = sj.encode_device(frames, 75.0, sj.YUV_420)
    t, quant = sj.make_tables(quality=75.0)
    header = sj.make_header(a.shape[1], a.shape[0], sj.YUV_420, quant)
    outs = [eng.encode_frames(frames, t, header, sj.YUV_420) for _ in range(2)]
    imgs = [synth.g_noise(w, h, 5) for (w, h) in ((33, 17), (640, 480), (1, 1))]
    got = sj.encode_images([torch.from_numpy(im).cuda() for im in imgs], 75.0, engine=eng, method=4, use_trellis=True)
    for k, im in enumerate(imgs):
        assert got[k] == sj.SjpegEncode(im, 75.0, 7, sj.YUV_420), k
    eng.wait()
    torch.cuda.synchronize()
    for out, sizes in outs:
        assert out[0, :int(sizes[0])].cpu().numpy().tobytes() == want[0]
    assert sj.encode_device(frames, 75.0, sj.YUV_420, engine=eng) == want
    eng.close()


def test_two_threads():
    imgs = [_thumbs(40, 41), _thumbs(40, 42)]
    wants = [[sj.SjpegEncode(im, 70.0, 7, sj.YUV_420) for im in b] for b in imgs]
    errors = []

    def work(i):
        try:
            eng = sj.Engine(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(3):
                    if _trellis(eng, imgs[i], 70.0, sj.YUV_420, 7)[0] != wants[i]:
                        errors.append(i)
            eng.close()
        except Exception as ex:                            # (reported below)
            errors.append(repr(ex))

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_back_to_back_without_a_host_wait_and_trim(engine):
    a, b = _thumbs(40, 51), _thumbs(40, 52)
    a.append(synth.g_struct(640, 480, 9))
    da, db = _dev(a), _dev(b)
    ra = engine.encode_ragged_trellis(sj.SRC_RGB, da, _dims(a), sj.YUV_420, _quant(80.0), 7)
    rb = engine.encode_ragged_batch(sj.SRC_RGB, db, _dims(b), sj.YUV_444, _quant(40.0), 2)
    rc = engine.encode_ragged_trellis(sj.SRC_RGB, db, _dims(b), sj.YUV_444, _quant(40.0), 8)
    got_a, got_b, got_c = _frames(*ra[:3]), _frames(*rb), _frames(*rc[:3])
    for k in range(len(a)):
        assert got_a[k] == sj.SjpegEncode(a[k], 80.0, 7, sj.YUV_420), k
    for k in range(len(b)):
        assert got_b[k] == sj.SjpegEncode(b[k], 40.0, 2, sj.YUV_444), k
        assert got_c[k] == sj.SjpegEncode(b[k], 40.0, 8, sj.YUV_444), k
    before = engine.scratch_bytes()
    kept = sum(sj.lib().sjpeg_hip_segment_count(w, h, sj.YUV_420) for (w, h) in _dims(a)) * 36864
    assert before >= kept                                  # (the kept blocks are engine scratch ...)
    engine.trim()
    assert engine.scratch_bytes() <= before - kept         # (... and trim gives them back)
    assert _frames(*engine.encode_ragged_trellis(sj.SRC_RGB, da, _dims(a), sj.YUV_420, _quant(80.0), 7)[:3]) == got_a


def test_argument_errors(engine):
    buf = torch.zeros((64, 3 * 64), dtype=torch.uint8, device="cuda")
    out = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(4, dtype=torch.int64, device="cuda")
    q = np.ascontiguousarray(_quant(75.0).reshape(1, 2, 64))

    def fr(w=16, h=16, stride=3 * 64, plane=True, off=0, cap=60000):
        f = sj.RaggedFrame()
        f.plane[0] = buf.data_ptr() if plane else None
        f.row_stride[0] = stride
        f.width, f.height, f.out_offset, f.out_capacity = w, h, off, cap
        return f

    def call(frames, method=7, quant=q, dl=12, dc=1, fmt=sj.SRC_RGB, mode=sj.YUV_420, nframes=None):
        arr = (sj.RaggedFrame * max(len(frames), 1))(*frames)
        n = len(frames) if nframes is None else nframes
        return sj.lib().sjpeg_hip_encode_ragged_trellis_src(engine._h, fmt, mode, n, arr,
                                                            quant.ctypes.data if quant is not None else None, 0, None,
                                                            0x78, method, dl, dc, out.data_ptr(), sizes.data_ptr(), None,
                                                            None)

    def err(rc, *words):
        assert rc != 0
        msg = sj.lib().sjpeg_hip_last_error().decode().lower()
        for w in words:
            assert w in msg, (w, msg)

    for method in (4, 6, 9, -1, 0):
        err(call([fr()], method=method), "methods 7 and 8")
        err(call([fr()], method=method, mode=sj.YUV_AUTO), "methods 7 and 8")
    err(call([fr()], quant=None), "quant")
    err(call([fr()], dl=13), "qdelta")
    err(call([fr()], dc=-13), "qdelta")
    err(call([fr()], nframes=0), "nframes")
    err(call([fr()], mode=5), "yuv_mode")
    for mode in (sj.YUV_420, sj.YUV_AUTO, sj.YUV_SHARP):
        err(call([fr(), fr(plane=False)], mode=mode), "frame 1", "null plane")
        err(call([fr(w=0)], mode=mode), "frame 0", "dimensions")
        err(call([fr(), fr(), fr(w=65536)], mode=mode), "frame 2", "dimensions")
        err(call([fr(stride=10)], mode=mode), "frame 0", "row_stride")
        err(call([fr(), fr(off=(1 << 64) - 100, cap=1000)], mode=mode), "frame 1", "overflows")
    err(call([fr()], fmt=sj.SRC_GRAY, mode=sj.YUV_420), "yuv_mode")
    err(call([fr()], fmt=sj.SRC_GRAY, mode=sj.YUV_AUTO), "rgb")
    err(call([fr()], fmt=sj.SRC_YUV420, mode=sj.YUV_SHARP), "rgb")
    assert call([fr()]) == 0                               # (the good call, after all of them)
    torch.cuda.synchronize()
    assert int(sizes[0]) > 0


def test_encode_images_and_compress_images(engine, risk_table):
    imgs = [synth.g_struct(w, h, 8) for (w, h) in ((640, 480), (31, 17), (1, 1), (250, 130))] + _mixed()[:6]
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    assert sj.encode_images(dev, engine=engine, method=4, use_trellis=True) == \
        [sj.SjpegEncode(im, 75.0, 7, sj.YUV_420) for im in imgs]
    quals = [10.0, 95.0, 50.0, 75.0, 20.0, 90.0, 60.0, 35.0, 80.0, 99.0]
    assert sj.encode_images(dev, quals, sj.YUV_444, engine=engine, method=6, use_trellis=True) == \
        [sj.SjpegEncode(im, q, 8, sj.YUV_444) for im, q in zip(imgs, quals)]
    assert sj.compress_images(dev, engine=engine, use_trellis=True) == \
        [sj.SjpegEncode(im, 75.0, 7, sj.YUV_AUTO) for im in imgs]
    # the reference ignores use_trellis with the other methods (src/api.cc:155-157)
    assert sj.encode_images(dev, engine=engine, method=1, use_trellis=True) == \
        [sj.SjpegEncode(im, 75.0, 1, sj.YUV_420) for im in imgs]
    assert sj.encode_images(dev, engine=engine, method=1, use_trellis=True) == sj.encode_images(dev, engine=engine, method=1)
    # without the keyword nothing changes
    assert sj.compress_images(dev, engine=engine) == [sj.SjpegCompress(im, 75.0) for im in imgs]
    with pytest.raises(sj.SjpegError, match="host API"):
        sj.encode_images(dev, engine=engine, method=7)
