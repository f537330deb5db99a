"""Ragged batches with the reference's per-picture analysis (sjpeg_hip_encode_ragged_batch_src, methods 0..6): the two
ragged analysis passes against the uniform ones picture by picture, every frame against the oracle or the uniform batch
path, layouts, capacity, split launches, concurrency and bad arguments."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import synth

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 13), (16, 16), (17, 13), (64, 64), (3840, 2160), (250, 130), (1, 4000), (4000, 1), (1920, 1080)]
SMALL = [(1, 1), (7, 13), (17, 13), (64, 64), (250, 130), (1, 300), (300, 1), (97, 61), (33, 200)]
MODES = [sj.YUV_420, sj.YUV_444, sj.YUV_400]


def _content(k, w, h):
    if k % 3 == 0:
        return synth.g_struct(w, h, 1000 + k)
    if k % 3 == 1:
        return synth.g_noise(w, h, 2000 + k)
    return np.full((h, w, 3), (37 * k) % 256, np.uint8)


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


def _batch(eng, imgs, q, mode, method, **kw):
    quant = [_quant(qq) for qq in q] if isinstance(q, list) else _quant(q)
    return _frames(*eng.encode_ragged_batch(sj.SRC_RGB, _dev(imgs), _dims(imgs), mode, quant, method, **kw))


def _one_source(d):
    """The uniform source of one picture (a [rows, 3 w] view) as a batch of one."""
    src, _ = sj.make_source(sj.SRC_RGB, [d.unsqueeze(0)])
    return src


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.mark.parametrize("mode", MODES)
def test_analysis_passes_equal_the_uniform_ones(engine, mode):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(SIZES)]
    dev = _dev(imgs)
    hist = engine.scan_histogram_ragged(sj.SRC_RGB, dev, _dims(imgs), mode).cpu().numpy()
    tables = [sj.make_tables(quality=q)[0] for q in (30.0, 75.0, 95.0, 50.0, 10.0, 90.0, 75.0, 60.0, 80.0, 20.0)]
    freq = engine.scan_symbol_stats_ragged(sj.SRC_RGB, dev, _dims(imgs), mode, tables).cpu().numpy()
    freq1 = engine.scan_symbol_stats_ragged(sj.SRC_RGB, dev, _dims(imgs), mode, tables[1]).cpu().numpy()
    for k, im in enumerate(imgs):
        h, w, _ = im.shape
        src = _one_source(dev[k][0])
        want_h = engine.scan_histogram_source(src, 1, w, h, mode).cpu().numpy()[0]
        assert np.array_equal(hist[k], want_h), (mode, k, w, h)
        want_f = engine.scan_symbol_stats_source(src, 1, w, h, tables[k], mode).cpu().numpy()[0]
        assert np.array_equal(freq[k], want_f), (mode, k, w, h)
        want_f1 = engine.scan_symbol_stats_source(src, 1, w, h, tables[1], mode).cpu().numpy()[0]
        assert np.array_equal(freq1[k], want_f1), (mode, k, w, h)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("method", [1, 2, 3, 4, 6])
def test_every_frame_equals_the_oracle(engine, oracle, mode, method):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(SMALL)]
    for q in (5.0, 50.0, 75.0, 95.0):
        got = _batch(engine, imgs, q, mode, method)
        for k, im in enumerate(imgs):
            assert got[k] == oracle.encode_method(im, q, mode, method), (mode, method, q, k, im.shape)


@pytest.mark.parametrize("method", [4, 1, 3])
def test_large_frames_equal_the_uniform_batch_path(engine, method):
    imgs = [synth.g_struct(1920, 1080, 5), synth.g_noise(3840, 2160, 6), synth.g_struct(3840, 2160, 7),
            synth.g_noise(1920, 1080, 8)]
    got = _batch(engine, imgs, 75.0, sj.YUV_420, method)
    for k, im in enumerate(imgs):
        want = sj.encode_device_method(torch.from_numpy(im).cuda().unsqueeze(0), 75.0, sj.YUV_420, method, engine=engine)
        assert got[k] == want[0], (method, k)


def test_per_frame_quality(engine):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate([(33, 21), (640, 480), (16, 16), (250, 130), (97, 61)])]
    quals = [5.0, 50.0, 75.0, 90.0, 100.0]
    for mode in (sj.YUV_420, sj.YUV_400):
        got = _batch(engine, imgs, quals, mode, 4)
        for k, im in enumerate(imgs):
            want = sj.encode_device_method(torch.from_numpy(im).cuda().unsqueeze(0), quals[k], mode, 4, engine=engine)
            assert got[k] == want[0], (mode, k)


def test_min_quant_q_bias_and_qdelta(engine, oracle):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate([(64, 64), (250, 130), (97, 61)])]
    mq = np.full((2, 64), 6, np.uint8)
    got = _batch(engine, imgs, 60.0, sj.YUV_420, 4, min_quant=mq, q_bias=0x60, dmax_luma=4, dmax_chroma=-2)
    for k, im in enumerate(imgs):
        want = sj.encode_device_method(torch.from_numpy(im).cuda().unsqueeze(0), 60.0, sj.YUV_420, 4, engine=engine,
                                       min_quant=mq, q_bias=0x60, dmax_luma=4, dmax_chroma=-2)
        assert got[k] == want[0], k


def _layout_planes(rng, fmt, w, h):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    shapes = {1: [(h, 4 * w)], 2: [(h, 4 * w)], 3: [(h, w)], 4: [(h, w)] * 3,
              5: [(h, w), (ch, cw), (ch, cw)], 6: [(h, w), (ch, 2 * cw)], 7: [(h, w), (ch, 2 * cw)]}[fmt]
    return [(rng.randint(0, 64, s) + np.arange(s[1])[None, :] // 3).astype(np.uint8) for s in shapes]


@pytest.mark.parametrize("fmt", [1, 2, 3, 4, 5, 6, 7])
def test_source_layouts(engine, fmt):
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
    for method in (4, 1):
        out, sizes, offs = engine.encode_ragged_batch(fmt, dev, dims, mode, _quant(70.0), method)
        got = _frames(out, sizes, offs)
        for k, (w, h) in enumerate(dims):
            planes = [torch.from_numpy(p).cuda().unsqueeze(0) for p in host[k]]
            want = sj.encode_source_method(fmt, planes, w, h, 70.0, mode, method, engine=engine)
            assert got[k] == want, (fmt, method, k, w, h)


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
    out, sizes, _ = engine.encode_ragged_batch(sj.SRC_RGB, _dev(imgs), _dims(imgs), mode, _quant(90.0), 4,
                                               capacities=caps, out=out, offsets=offs)
    torch.cuda.synchronize()
    sz = sizes.cpu().numpy()
    host = out.cpu().numpy()
    assert sz[1] == 0
    for k in (0, 2, 3):
        want = sj.encode_device_method(torch.from_numpy(imgs[k]).cuda().unsqueeze(0), 90.0, mode, 4, engine=engine)
        assert host[offs[k]:offs[k] + sz[k]].tobytes() == want[0], k
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


def test_split_launches(monkeypatch):
    imgs = _thumbs(300, 31)
    imgs.insert(120, synth.g_struct(1920, 1080, 3))
    imgs.append(synth.g_noise(640, 480, 4))
    eng = sj.Engine(0)
    want = _batch(eng, imgs, 75.0, sj.YUV_420, 4)
    whole = eng.scratch_bytes()
    eng.close()
    monkeypatch.setenv("SJPEG_HIP_SCRATCH_LIMIT_BYTES", "1")
    small = sj.Engine(0)                                   # (made after the limit is set: every frame its own launch)
    assert _batch(small, imgs, 75.0, sj.YUV_420, 4) == want
    assert small.scratch_bytes() < whole                   # (a launch's scratch is one frame's)
    for k in list(range(0, len(imgs), 29)) + [120, len(imgs) - 1]:
        one = sj.encode_device_method(torch.from_numpy(imgs[k]).cuda().unsqueeze(0), 75.0, sj.YUV_420, 4, engine=small)
        assert want[k] == one[0], k
    small.close()


def test_pipelined_engine():
    eng = sj.Engine(0)
    eng.set_pipelined(True)
    a = synth.g_struct(640, 360, 1)
    frames = torch.from_numpy(a).cuda().unsqueeze(0)
    want = sj.encode_device(frames, 75.0, sj.YUV_420)
    outs = [eng.encode_frames(frames, *_tables_header(a, 75.0)) for _ in range(2)]
    imgs = [synth.g_noise(w, h, 5) for (w, h) in ((33, 17), (640, 480), (1, 1))]
    got = sj.encode_images([torch.from_numpy(im).cuda() for im in imgs], 75.0, engine=eng, method=4)
    for k, im in enumerate(imgs):
        assert got[k] == sj.encode_device_method(torch.from_numpy(im).cuda().unsqueeze(0), 75.0, sj.YUV_420, 4)[0]
    eng.wait()
    torch.cuda.synchronize()
    for out, sizes in outs:
        assert out[0, :int(sizes[0])].cpu().numpy().tobytes() == want[0]
    assert sj.encode_device(frames, 75.0, sj.YUV_420, engine=eng) == want
    eng.close()


def _tables_header(img, q):
    t, quant = sj.make_tables(quality=q)
    return t, sj.make_header(img.shape[1], img.shape[0], sj.YUV_420, quant), sj.YUV_420


def test_two_threads(engine):
    imgs = [_thumbs(60, 41), _thumbs(60, 42)]
    wants = [[sj.encode_device_method(torch.from_numpy(im).cuda().unsqueeze(0), 70.0, sj.YUV_420, 4, engine=engine)[0]
              for im in b] for b in imgs]
    errors = []

    def work(i):
        try:
            eng = sj.Engine(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(3):
                    if _batch(eng, imgs[i], 70.0, sj.YUV_420, 4) != wants[i]:
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


def test_back_to_back_without_a_host_wait(engine):
    a, b = _thumbs(40, 51), _thumbs(40, 52)
    da, db = _dev(a), _dev(b)
    ra = engine.encode_ragged_batch(sj.SRC_RGB, da, _dims(a), sj.YUV_420, _quant(80.0), 4)
    rb = engine.encode_ragged_batch(sj.SRC_RGB, db, _dims(b), sj.YUV_444, _quant(40.0), 2)
    got_a, got_b = _frames(*ra), _frames(*rb)
    for k in range(len(a)):
        one = torch.from_numpy(a[k]).cuda().unsqueeze(0)
        assert got_a[k] == sj.encode_device_method(one, 80.0, sj.YUV_420, 4, engine=engine)[0], k
        one = torch.from_numpy(b[k]).cuda().unsqueeze(0)
        assert got_b[k] == sj.encode_device_method(one, 40.0, sj.YUV_444, 2, engine=engine)[0], k


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

    def call(frames, method=4, quant=q, dl=12, dc=1, fmt=sj.SRC_RGB, mode=sj.YUV_420, nframes=None):
        arr = (sj.RaggedFrame * max(len(frames), 1))(*frames)
        n = len(frames) if nframes is None else nframes
        return sj.lib().sjpeg_hip_encode_ragged_batch_src(engine._h, fmt, mode, n, arr,
                                                          quant.ctypes.data if quant is not None else None, 0, None,
                                                          0x78, method, dl, dc, out.data_ptr(), sizes.data_ptr(), None)

    def err(rc, *words):
        assert rc != 0
        msg = sj.lib().sjpeg_hip_last_error().decode().lower()
        for w in words:
            assert w in msg, (w, msg)

    err(call([fr()], method=7), "methods 0..6")
    err(call([fr()], method=8), "methods 0..6")
    err(call([fr()], method=-1), "methods 0..6")
    err(call([fr()], quant=None), "quant")
    err(call([fr()], dl=13), "qdelta")
    err(call([fr()], dc=-13), "qdelta")
    err(call([fr()], nframes=0), "nframes")
    err(call([fr(), fr(plane=False)]), "frame 1", "null plane")
    err(call([fr(w=0)]), "frame 0", "dimensions")
    err(call([fr(), fr(), fr(w=65536)]), "frame 2", "dimensions")
    err(call([fr(stride=10)]), "frame 0", "row_stride")
    err(call([fr()], fmt=sj.SRC_GRAY, mode=sj.YUV_420), "yuv_mode")
    err(call([fr(), fr(off=(1 << 64) - 100, cap=1000)]), "frame 1", "overflows")
    hist = torch.zeros((2, 2, 64, 128), dtype=torch.int32, device="cuda")
    arr = (sj.RaggedFrame * 2)(fr(), fr(stride=10))
    err(sj.lib().sjpeg_hip_scan_histogram_ragged_src(engine._h, sj.SRC_RGB, sj.YUV_420, 2, arr, hist.data_ptr(), None),
        "frame 1", "row_stride")
    t = sj.make_tables(quality=75.0)[0]
    t.flags = sj.QUANT_TRELLIS
    arr = (sj.RaggedFrame * 1)(fr())
    err(sj.lib().sjpeg_hip_scan_symbol_stats_ragged_src(engine._h, sj.SRC_RGB, sj.YUV_420, 1, arr,
                                                        C.cast(C.pointer(t), C.c_void_p), 0, hist.data_ptr(), None),
        "tables[0]")


def test_encode_images(engine):
    imgs = [synth.g_struct(w, h, 8) for (w, h) in ((640, 480), (31, 17), (1, 1), (1920, 1080))]
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    want = [sj.encode_device_method(d.unsqueeze(0), 75.0, sj.YUV_420, 4, engine=engine)[0] for d in dev]
    assert sj.encode_images(dev, engine=engine, method=4) == want
    quals = [10.0, 95.0, 50.0, 75.0]
    want = [sj.encode_device_method(d.unsqueeze(0), q, sj.YUV_444, 6, engine=engine)[0] for d, q in zip(dev, quals)]
    assert sj.encode_images(dev, quals, sj.YUV_444, engine=engine, method=6) == want
    # without `method`: method 0, as before
    want = [sj.encode_device(d.unsqueeze(0), 75.0, sj.YUV_420, engine=engine)[0] for d in dev]
    assert sj.encode_images(dev, engine=engine) == want
    assert sj.encode_images(dev, engine=engine, method=0) == want
