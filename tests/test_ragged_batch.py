"""Ragged batches (sjpeg_hip_encode_ragged_src): pictures of different sizes in one call, every frame checked against
the oracle's single-picture encode (method 0)."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import synth

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 13), (16, 16), (17, 13), (64, 64), (3840, 2160), (250, 130), (1, 4000), (4000, 1), (1920, 1080)]


def _content(k, w, h):
    if k % 3 == 0:
        return synth.g_struct(w, h, 1000 + k)
    if k % 3 == 1:
        return synth.g_noise(w, h, 2000 + k)
    return np.full((h, w, 3), (37 * k) % 256, np.uint8)


def _rgb_planes(img, pad=16):
    """One device allocation per picture, rows padded by `pad` bytes."""
    h, w, _ = img.shape
    buf = np.zeros((h, 3 * w + pad), np.uint8)
    buf[:, :3 * w] = img.reshape(h, 3 * w)
    return [torch.from_numpy(buf).cuda()[:, :3 * w]]


def _ragged(eng, imgs, q, mode, per_frame_q=None, **kw):
    quals = per_frame_q or [q] * len(imgs)
    made = {qq: sj.make_tables(quality=qq) for qq in set(quals)}
    headers = [sj.make_header(im.shape[1], im.shape[0], mode, made[qq][1]) for im, qq in zip(imgs, quals)]
    tables = [made[qq][0] for qq in quals] if per_frame_q else made[q][0]
    planes = [_rgb_planes(im) for im in imgs]
    dims = [(im.shape[1], im.shape[0]) for im in imgs]
    out, sizes, offs = eng.encode_ragged(sj.SRC_RGB, planes, dims, mode, tables, headers, **kw)
    torch.cuda.synchronize()
    return out, sizes.cpu().numpy(), offs


def _frames(out, sizes, offs):
    host = out.cpu().numpy()
    return [host[o:o + int(s)].tobytes() for o, s in zip(offs, sizes)]


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.mark.parametrize("mode", [sj.YUV_420, sj.YUV_444, sj.YUV_400])
def test_mixed_geometries_vs_oracle(engine, oracle, mode):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(SIZES)]
    for q in (0.0, 20.0, 75.0, 95.0, 100.0):
        out, sizes, offs = _ragged(engine, imgs, q, mode)
        got = _frames(out, sizes, offs)
        for k, im in enumerate(imgs):
            assert got[k] == oracle.encode(im, q, mode), (mode, q, k, im.shape)


def test_per_frame_quality(engine, oracle):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate([(33, 21), (640, 480), (16, 16), (250, 130), (97, 61)])]
    quals = [5.0, 50.0, 75.0, 90.0, 100.0]
    out, sizes, offs = _ragged(engine, imgs, None, sj.YUV_420, per_frame_q=quals)
    for k, (im, g) in enumerate(zip(imgs, _frames(out, sizes, offs))):
        assert g == oracle.encode(im, quals[k], sj.YUV_420), k


def test_equivalences(engine):
    imgs = [synth.g_struct(250, 130, 50 + k) for k in range(5)]
    stacked = torch.from_numpy(np.stack(imgs)).cuda()
    want = sj.encode_device(stacked, 80.0, sj.YUV_420, engine=engine)
    out, sizes, offs = _ragged(engine, imgs, 80.0, sj.YUV_420)
    assert _frames(out, sizes, offs) == want
    one = sj.encode_device(stacked[2:3], 80.0, sj.YUV_420, engine=engine)
    out, sizes, offs = _ragged(engine, imgs[2:3], 80.0, sj.YUV_420)
    assert _frames(out, sizes, offs) == one
    mixed = [synth.g_noise(w, h, 9) for (w, h) in ((31, 17), (640, 480), (8, 8))]
    a = _frames(*_ragged(engine, mixed, 60.0, sj.YUV_444))
    b = _frames(*_ragged(engine, mixed, 60.0, sj.YUV_444))
    assert a == b


def _layout_planes(rng, fmt, w, h):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    shapes = {0: [(h, 3 * w)], 1: [(h, 4 * w)], 2: [(h, 4 * w)], 3: [(h, w)], 4: [(h, w)] * 3,
              5: [(h, w), (ch, cw), (ch, cw)], 6: [(h, w), (ch, 2 * cw)], 7: [(h, w), (ch, 2 * cw)]}[fmt]
    return [(rng.randint(0, 64, s) + np.arange(s[1])[None, :] // 3).astype(np.uint8) for s in shapes]


@pytest.mark.parametrize("fmt", [0, 1, 2, 3, 4, 5, 6, 7])
def test_source_layouts(engine, oracle, fmt):
    rng = np.random.RandomState(300 + fmt)
    mode = {3: sj.YUV_400, 4: sj.YUV_444, 5: sj.YUV_420, 6: sj.YUV_420, 7: sj.YUV_420}.get(fmt, sj.YUV_420)
    dims = [(1, 1), (17, 13), (250, 130), (40, 9), (97, 61)]
    host = [_layout_planes(rng, fmt, w, h) for (w, h) in dims]
    q = 75.0
    tables, quant = sj.make_tables(quality=q)
    headers = [sj.make_header(w, h, mode, quant) for (w, h) in dims]
    dev, keep = [], []
    for k, planes in enumerate(host):
        fr = []
        for p in planes:
            padded = np.zeros((p.shape[0], p.shape[1] + 24), np.uint8)   # (separate allocation, padded rows)
            padded[:, :p.shape[1]] = p
            if k == 2:
                # bottom-up: the rows lie last to first in memory, row 0 is the allocation's last row
                t = torch.from_numpy(np.ascontiguousarray(padded[::-1])).cuda()
                keep.append(t)
                fr.append((t.data_ptr() + (p.shape[0] - 1) * padded.shape[1], -padded.shape[1]))
            else:
                fr.append(torch.from_numpy(padded).cuda()[:, :p.shape[1]])
        dev.append(fr)
    out, sizes, offs = engine.encode_ragged(fmt, dev, dims, mode, tables, headers)
    got = _frames(out, sizes.cpu().numpy(), offs)
    for k, (w, h) in enumerate(dims):
        assert got[k] == oracle.encode_src(fmt, host[k], w, h, quant, yuv_mode=mode, method=0), (fmt, k, w, h)


def test_capacity_and_canary(engine, oracle):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate([(64, 64), (250, 130), (97, 61), (640, 480)])]
    q, mode = 90.0, sj.YUV_420
    tables, quant = sj.make_tables(quality=q)
    headers = [sj.make_header(im.shape[1], im.shape[0], mode, quant) for im in imgs]
    caps = [sj.frame_bound(im.shape[1], im.shape[0], mode, len(headers[k])) for k, im in enumerate(imgs)]
    caps[1] = 700                                          # far too small for frame 1
    offs, at = [], 64
    for c in caps:
        offs.append(at)
        at += c + 48                                       # gaps between the ranges
    out = torch.full((at + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    planes = [_rgb_planes(im) for im in imgs]
    dims = [(im.shape[1], im.shape[0]) for im in imgs]
    out, sizes, _ = engine.encode_ragged(sj.SRC_RGB, planes, dims, mode, tables, headers, capacities=caps,
                                         out=out, offsets=offs)
    torch.cuda.synchronize()
    sz = sizes.cpu().numpy()
    host = out.cpu().numpy()
    assert sz[1] == 0
    for k in (0, 2, 3):
        assert host[offs[k]:offs[k] + sz[k]].tobytes() == oracle.encode(imgs[k], q, mode), k
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


@pytest.mark.parametrize("limit", [None, "1", "300000000"])
def test_many_thumbnails_and_4k(oracle, monkeypatch, limit):
    if limit is not None:
        monkeypatch.setenv("SJPEG_HIP_SCRATCH_LIMIT_BYTES", limit)
    eng = sj.Engine(0)                                     # (made after the limit is set)
    imgs = _thumbs(2000, 11)
    imgs.insert(700, synth.g_struct(3840, 2160, 3))
    imgs.append(synth.g_noise(3840, 2160, 4))
    got = _frames(*_ragged(eng, imgs, 75.0, sj.YUV_420))
    for k in list(range(0, len(imgs), 7)) + [700, len(imgs) - 1]:
        assert got[k] == oracle.encode(imgs[k], 75.0, sj.YUV_420), k
    h = __import__("hashlib").md5(b"".join(got)).hexdigest()
    test_many_thumbnails_and_4k.digests = getattr(test_many_thumbnails_and_4k, "digests", set()) | {h}
    assert len(test_many_thumbnails_and_4k.digests) == 1
    eng.close()


def test_pipelined_engine(oracle):
    eng = sj.Engine(0)
    eng.set_pipelined(True)
    a = synth.g_struct(640, 360, 1)
    frames = torch.from_numpy(a).cuda().unsqueeze(0)
    want = oracle.encode(a, 75.0, sj.YUV_420)
    for _ in range(3):
        assert sj.encode_device(frames, 75.0, sj.YUV_420, engine=eng) == [want]
    outs = [eng.encode_frames(frames, *_tables_header(a, 75.0)) for _ in range(2)]
    imgs = [synth.g_noise(w, h, 5) for (w, h) in ((33, 17), (640, 480), (1, 1))]
    got = sj.encode_images([torch.from_numpy(im).cuda() for im in imgs], 75.0, engine=eng)
    for k, im in enumerate(imgs):
        assert got[k] == oracle.encode(im, 75.0, sj.YUV_420)
    eng.wait()
    torch.cuda.synchronize()
    for out, sizes in outs:
        assert out[0, :int(sizes[0])].cpu().numpy().tobytes() == want
    for _ in range(3):
        assert sj.encode_device(frames, 75.0, sj.YUV_420, engine=eng) == [want]
    eng.close()


def _tables_header(img, q):
    t, quant = sj.make_tables(quality=q)
    return t, sj.make_header(img.shape[1], img.shape[0], sj.YUV_420, quant), sj.YUV_420


def test_two_threads(oracle):
    imgs = [_thumbs(60, 21), _thumbs(60, 22)]
    wants = [[oracle.encode(im, 70.0, sj.YUV_420) for im in batch] for batch in imgs]
    errors = []

    def work(i):
        try:
            eng = sj.Engine(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(5):
                    got = _frames(*_ragged(eng, imgs[i], 70.0, sj.YUV_420))
                    if got != wants[i]:
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


def _call(eng, frames, nframes=None, fmt=sj.SRC_RGB, mode=sj.YUV_420, tables=None, headers=None, hoffs=None):
    L = sj.lib()
    t = tables if tables is not None else sj.make_tables(quality=75.0)[0]
    arr = (sj.RaggedFrame * max(len(frames), 1))(*frames)
    out = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(max(len(frames), 1), dtype=torch.int64, device="cuda")
    n = len(frames) if nframes is None else nframes
    return L.sjpeg_hip_encode_ragged_src(eng._h, fmt, mode, n, arr, C.cast(C.pointer(t), C.c_void_p), 0, headers,
                                         C.cast(hoffs, C.c_void_p) if hoffs is not None else None, 1,
                                         out.data_ptr(), sizes.data_ptr(), None)


def test_argument_errors(engine):
    buf = torch.zeros((64, 3 * 64), dtype=torch.uint8, device="cuda")

    def fr(w=16, h=16, stride=3 * 64, plane=True, off=0, cap=60000):
        f = sj.RaggedFrame()
        f.plane[0] = buf.data_ptr() if plane else None
        f.row_stride[0] = stride
        f.width, f.height, f.out_offset, f.out_capacity = w, h, off, cap
        return f

    def err(rc, *words):
        assert rc != 0
        msg = sj.lib().sjpeg_hip_last_error().decode().lower()
        for w in words:
            assert w in msg, (w, msg)

    err(_call(engine, [fr()], nframes=0), "nframes")
    err(_call(engine, [fr(), fr(plane=False)]), "frame 1", "null plane")
    err(_call(engine, [fr(w=0)]), "frame 0", "dimensions")
    err(_call(engine, [fr(), fr(), fr(w=65536)]), "frame 2", "dimensions")
    err(_call(engine, [fr(stride=10)]), "frame 0", "row_stride")
    err(_call(engine, [fr()], fmt=sj.SRC_GRAY, mode=sj.YUV_420), "yuv_mode")
    hoffs = (C.c_size_t * 3)(0, 10, 5)
    err(_call(engine, [fr(), fr()], headers=b"x" * 10, hoffs=hoffs), "header_offsets")
    for flag in (sj.QUANT_TRELLIS, sj.RESTART_MARKERS, sj.QUANT_KEEP, sj.QUANT_REPLAY):
        t = sj.make_tables(quality=75.0)[0]
        t.flags = flag
        err(_call(engine, [fr()], tables=t), "tables[0]")
    err(_call(engine, [fr(), fr(off=(1 << 64) - 100, cap=1000)]), "frame 1", "overflows")


def test_encode_images(engine):
    imgs = [synth.g_struct(w, h, 8) for (w, h) in ((640, 480), (31, 17), (1, 1), (1920, 1080))]
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    want = [sj.encode_device(d.unsqueeze(0), 75.0, sj.YUV_420, engine=engine)[0] for d in dev]
    assert sj.encode_images(dev, engine=engine) == want
    quals = [10.0, 95.0, 50.0, 75.0]
    want = [sj.encode_device(d.unsqueeze(0), q, sj.YUV_444, engine=engine)[0] for d, q in zip(dev, quals)]
    assert sj.encode_images(dev, quals, sj.YUV_444, engine=engine) == want
    # a strided row view (a crop of a larger picture)
    big = torch.from_numpy(synth.g_noise(300, 200, 2)).cuda()
    crop = big[10:110, 20:220]
    assert sj.encode_images([crop], engine=engine) == sj.encode_device(crop.contiguous().unsqueeze(0), engine=engine)
