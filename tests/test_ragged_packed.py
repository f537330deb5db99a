"""Ragged batches into one packed buffer (sjpeg_hip_encode_ragged_packed_src): every flow of the unpacked ragged entry
points with the frames back to back -- the bytes of the unpacked call, the layout sjpeg_hip_gather_streams takes, the
two refusals (a frame over its own capacity, a frame past the end of the pool), several launches and parts, the
pipelined engine, the exchange, and encode_images / compress_images with packed=True."""
import os
import threading

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import synth

pytestmark = pytest.mark.gpu

# 1 x 1, 1 x N, N x 1, sizes that clip MCUs, one 4K among thumbnails
SIZES = [(1, 1), (1, 37), (41, 1), (7, 13), (17, 13), (64, 64), (250, 130), (3840, 2160), (97, 61), (33, 21),
         (640, 480), (5, 300), (128, 128), (211, 97)]
Q = 75.0
OVERFLOW = 1 << 63

SIZE_SEARCH = dict(target_mode=sj.TARGET_SIZE, target_value=2500.0, passes=5)
PSNR_SEARCH = dict(target_mode=sj.TARGET_PSNR, target_value=36.0, passes=5)
# (name, yuv_mode, method, search); a search list is cut to the batch
FLOWS = [(f"m{m}-{mode}", mode, m, None) for m in (0, 4, 6) for mode in (sj.YUV_420, sj.YUV_444, sj.YUV_400)] + [
    ("auto-m4", sj.YUV_AUTO, 4, None), ("sharp-m4", sj.YUV_SHARP, 4, None),
    ("trellis7-auto", sj.YUV_AUTO, 7, None), ("trellis8-420", sj.YUV_420, 8, None),
    ("size-search", sj.YUV_420, 4, SIZE_SEARCH), ("psnr-search", sj.YUV_444, 1, PSNR_SEARCH),
    # some frames searched for a size, some for a PSNR, every third one not at all: the sub-calls reorder the frames
    ("mixed-search", sj.YUV_420, 4, "mixed"),
]
FLOW_IDS = [f[0] for f in FLOWS]


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


def _gradient(w, h):
    x = np.arange(w)[None, :] * 200 // w
    y = np.arange(h)[:, None] * 200 // h
    return np.stack([np.broadcast_to(x + 20, (h, w)), np.broadcast_to(y + 30, (h, w)), np.full((h, w), 90)],
                    2).astype(np.uint8)


def _content(k, w, h):
    """Content whose SJPEG_YUV_AUTO verdicts differ (structure, noise, gray noise, saturated noise, a gradient)."""
    rng = np.random.RandomState(700 + k)
    kind = k % 5
    if kind == 4:
        return _gradient(w, h)
    if kind == 0:
        return synth.g_struct(w, h, 3000 + k)
    if kind == 1:
        return synth.g_noise(w, h, 3000 + k)
    if kind == 2:
        return np.repeat(rng.randint(0, 256, (h, w, 1)), 3, 2).astype(np.uint8)
    return (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def _imgs(sizes=SIZES):
    return [_content(k, w, h) for k, (w, h) in enumerate(sizes)]


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


def _search_of(search, n):
    if search != "mixed":
        return search
    kinds = [SIZE_SEARCH, PSNR_SEARCH, dict(SIZE_SEARCH, passes=1)]
    return [kinds[k % 3] for k in range(n)]


def _unpacked(eng, imgs, mode, method, search, **kw):
    """The frames (bytes, b"" for size 0) and modes of the unpacked entry point the same arguments go to."""
    planes, dims = _dev(imgs), _dims(imgs)
    modes = None
    search = _search_of(search, len(imgs))
    if search is not None:
        out, sizes, offs, _, _ = eng.encode_ragged_search(sj.SRC_RGB, planes, dims, mode, _quant(), search, method, **kw)
    elif method >= 7:
        out, sizes, offs, modes = eng.encode_ragged_trellis(sj.SRC_RGB, planes, dims, mode, _quant(), method, **kw)
    elif mode in (sj.YUV_AUTO, sj.YUV_SHARP):
        out, sizes, offs, modes = eng.encode_ragged_auto(sj.SRC_RGB, planes, dims, mode, _quant(), method, **kw)
    else:
        out, sizes, offs = eng.encode_ragged_batch(sj.SRC_RGB, planes, dims, mode, _quant(), method, **kw)
    eng.wait()
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    return [host[o:o + int(s)].tobytes() if s > 0 else b"" for o, s in zip(offs, sz)], modes


class Packed:
    """One packed call into a buffer pre-filled with 0xA5, `slack` bytes longer than the capacity it is given."""

    def __init__(self, eng, imgs, mode, method, search, packed_capacity=None, capacities=None, slack=4096):
        planes, dims = _dev(imgs), _dims(imgs)
        n = len(imgs)
        if packed_capacity is None:
            bm = sj.YUV_444 if mode in (sj.YUV_AUTO, sj.YUV_SHARP) else mode
            packed_capacity = sum((sj.frame_bound(w, h, bm, 2048) + 15) & ~15 for (w, h) in dims)
        buf = torch.full((packed_capacity + slack,), 0xA5, dtype=torch.uint8, device="cuda")
        res = eng.encode_ragged_packed(sj.SRC_RGB, planes, dims, mode, _quant(), method,
                                       search=_search_of(search, n), capacities=capacities,
                                       packed_capacity=packed_capacity, out=buf)
        eng.wait()
        torch.cuda.synchronize()
        out, sizes, offsets, self.modes = res[:4]
        assert out.data_ptr() == buf.data_ptr() and sizes.numel() == n and offsets.numel() == n + 1
        self.n, self.capacity = n, packed_capacity
        self.host = out.cpu().numpy()
        self.sz = [int(x) for x in sizes.cpu().numpy()]
        off = [int(x) for x in offsets.cpu().numpy()]
        self.off, end = off[:n], off[n]
        self.overflow = end < 0                               # bit 63 of the int64
        self.end = end & (OVERFLOW - 1)
        self.frames = [self.host[o:o + s].tobytes() if s > 0 else b"" for o, s in zip(self.off, self.sz)]

    def check_layout(self):
        """Starts at multiples of 16, back to back in the order of the starts, zero padding, nothing behind the end."""
        kept = sorted((o, s) for o, s in zip(self.off, self.sz) if s > 0)
        at = 0
        for o, s in kept:
            assert o % 16 == 0 and o == at, (o, at)
            pad_end = (o + s + 15) & ~15
            assert (self.host[o + s:pad_end] == 0).all(), o
            at = pad_end
        if not self.overflow:
            assert at == self.end, (at, self.end)
        assert at <= self.capacity
        assert (self.host[at:] == 0xA5).all()
        assert (self.host[self.capacity:] == 0xA5).all()


@pytest.mark.parametrize("name,mode,method,search", FLOWS, ids=FLOW_IDS)
def test_bytes_and_layout_of_every_flow(engine, oracle, name, mode, method, search):
    imgs = _imgs()
    want, want_modes = _unpacked(engine, imgs, mode, method, search)
    assert all(len(w) > 0 for w in want)
    p = Packed(engine, imgs, mode, method, search)
    assert not p.overflow
    for k in range(len(imgs)):
        assert p.frames[k] == want[k], (name, k, imgs[k].shape)
    p.check_layout()
    if want_modes is not None:
        assert p.modes == want_modes
    else:
        assert p.modes == [mode] * len(imgs)
    one_group = mode != sj.YUV_AUTO and search != "mixed"
    if one_group:
        assert p.off == sorted(p.off), name                   # the caller's order
    if search is None and mode == sj.YUV_420 and method in (0, 4):
        for k, im in enumerate(imgs):                         # not only the library against itself
            assert p.frames[k] == oracle.encode_method(im, Q, mode, method), (name, k)


def test_auto_groups_by_mode(engine):
    imgs = _imgs()
    verdicts = [m for (m, _) in sj.riskiness_images([torch.from_numpy(im).cuda() for im in imgs], engine=engine)]
    assert len(set(verdicts)) >= 2, verdicts
    want, want_modes = _unpacked(engine, imgs, sj.YUV_AUTO, 4, None)
    p = Packed(engine, imgs, sj.YUV_AUTO, 4, None)
    assert p.modes == want_modes == verdicts
    assert p.frames == want
    p.check_layout()
    # grouped by mode in the order 4:2:0, 4:4:4, 4:0:0, sharp; the caller's order inside a group
    order = sorted(range(len(imgs)), key=lambda k: p.off[k])
    rank = {sj.YUV_420: 0, sj.YUV_444: 1, sj.YUV_400: 2, sj.YUV_SHARP: 3}
    assert order == sorted(range(len(imgs)), key=lambda k: (rank[verdicts[k]], k))


def test_mixed_search_codes_unsearched_frames_first(engine):
    imgs = _imgs()
    p = Packed(engine, imgs, sj.YUV_420, 4, "mixed")
    order = sorted(range(len(imgs)), key=lambda k: p.off[k])
    assert order == sorted(range(len(imgs)), key=lambda k: (0 if k % 3 == 2 else 1, k))
    p.check_layout()


@pytest.mark.parametrize("k", [0, 6, 9])
def test_pool_overflow_drops_the_frames_from_k_on(engine, k):
    imgs = _imgs()
    full = Packed(engine, imgs, sj.YUV_420, 4, None)
    assert not full.overflow and full.off == sorted(full.off)
    p = Packed(engine, imgs, sj.YUV_420, 4, None, packed_capacity=full.off[k])
    assert p.overflow
    assert p.end == full.end                                  # the capacity that would have been enough
    for f in range(len(imgs)):
        if f < k:
            assert p.frames[f] == full.frames[f] and p.off[f] == full.off[f], f
        else:
            assert p.sz[f] == 0, f
    p.check_layout()
    assert (p.host[full.off[k]:] == 0xA5).all()


def test_frame_over_its_own_capacity_takes_no_room(engine):
    imgs = _imgs([(64, 64), (250, 130), (97, 61), (640, 480)])
    caps = [sj.frame_bound(w, h, sj.YUV_420, 2048) for (w, h) in _dims(imgs)]
    want, _ = _unpacked(engine, imgs, sj.YUV_420, 4, None)
    caps[1] = 700                                             # far too small for frame 1
    p = Packed(engine, imgs, sj.YUV_420, 4, None, capacities=caps)
    assert not p.overflow
    assert p.sz[1] == 0
    for f in (0, 2, 3):
        assert p.frames[f] == want[f], f
    assert p.off[2] == (p.off[0] + p.sz[0] + 15) & ~15        # frame 2 lies right behind frame 0
    p.check_layout()


def _thumbs(n, seed):
    rng = np.random.RandomState(seed)
    return [_content(k, int(rng.randint(1, 97)), int(rng.randint(1, 97))) for k in range(n)]


@pytest.mark.parametrize("name,mode,method", [("m4-420", sj.YUV_420, 4), ("auto-m4", sj.YUV_AUTO, 4),
                                              ("trellis7-420", sj.YUV_420, 7)])
def test_several_launches_and_parts(monkeypatch, name, mode, method):
    imgs = _thumbs(300, 5)
    imgs.insert(120, synth.g_struct(3840, 2160, 3))
    runs = []
    for limit in (None, "1", "300000000"):
        if limit is not None:
            monkeypatch.setenv("SJPEG_HIP_SCRATCH_LIMIT_BYTES", limit)
        eng = sj.Engine(0)                                    # (made after the limit is set)
        p = Packed(eng, imgs, mode, method, None)
        assert not p.overflow
        p.check_layout()
        runs.append(p)
        if limit is None:
            want, _ = _unpacked(eng, imgs, mode, method, None)
            assert p.frames == want
        eng.close()
    for p in runs[1:]:
        assert p.frames == runs[0].frames and p.modes == runs[0].modes and p.end == runs[0].end
        if mode != sj.YUV_AUTO:                               # one group: the caller's order whatever the launches
            assert p.off == runs[0].off


def test_pipelined_engine(oracle):
    eng = sj.Engine(0)
    eng.set_pipelined(True)
    a = synth.g_struct(640, 360, 1)
    frames = torch.from_numpy(a).cuda().unsqueeze(0)
    for _ in range(2):                                        # (the stitch stream has work the packed call must follow)
        assert sj.encode_device(frames, Q, sj.YUV_420, engine=eng) == [oracle.encode(a, Q, sj.YUV_420)]
    imgs = _imgs()
    t, quant = sj.make_tables(quality=Q)
    pending = eng.encode_frames(frames, t, sj.make_header(640, 360, sj.YUV_420, quant), sj.YUV_420)
    p = Packed(eng, imgs, sj.YUV_420, 4, None)                # (waits: Engine.wait)
    for k, im in enumerate(imgs):
        assert p.frames[k] == oracle.encode_method(im, Q, sj.YUV_420, 4), k
    p.check_layout()
    assert pending[0][0, :int(pending[1][0])].cpu().numpy().tobytes() == oracle.encode(a, Q, sj.YUV_420)
    eng.close()


def _local_world(world, body):
    """body(rank, comm) on `world` threads, each with a stream of its own and a communicator of the local transport
    (the scaffold of tests/test_gpu_parity.py, restated)."""
    ident = os.urandom(128)
    results, errors = [None] * world, [None] * world

    def run(r):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                comm = sj.Comm(ident, r, world, local=True)
                try:
                    results[r] = body(r, comm)
                    torch.cuda.current_stream().synchronize()
                finally:
                    comm.close()
        except BaseException as e:          # noqa: BLE001 -- handed to the main thread
            errors[r] = e

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
        assert not t.is_alive(), "a rank of the local world hangs"
    return results, errors


def test_exchange_takes_the_packed_ragged_output(engine):
    world, root = 2, 0
    batches = [_imgs([(64, 64), (250, 130), (1, 1), (640, 480), (97, 61)]), _imgs([(33, 21), (1920, 1080), (17, 13)])]
    batches[1] = [np.ascontiguousarray(im[:, ::-1]) for im in batches[1]]       # (other pictures than rank 0's)
    want_frames = [_unpacked(engine, b, sj.YUV_420, 4, None)[0] for b in batches]
    want = b"".join(f + b"\0" * (-len(f) % 16) for b in want_frames for f in b)
    per_max = max(len(b) for b in batches)

    def body(rank, comm):
        imgs = batches[rank]
        n = len(imgs)
        eng = sj.Engine(0)
        out, sizes, offsets, _ = eng.encode_ragged_packed(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_420, _quant(), 4)
        offs = torch.zeros(per_max + 1, dtype=torch.int64, device="cuda")
        offs[:n + 1] = offsets
        rows_dev = torch.zeros((world + 1) * (per_max + 2), dtype=torch.int64, device="cuda")
        cap = len(want) + 64
        gathered = torch.full((cap,), 0xC3, dtype=torch.uint8, device="cuda") if rank == root else cap
        rows, ro = comm.gather_streams(root, out, offs, sizes, n, per_max, rows_dev, gathered)
        torch.cuda.current_stream().synchronize()
        assert int(ro[world]) == len(want)
        for r in range(world):
            assert [int(v) for v in rows[r][2:2 + len(batches[r])]] == [len(f) for f in want_frames[r]]
        res = gathered[:len(want)].cpu().numpy().tobytes() if rank == root else None
        eng.close()
        return res

    results, errors = _local_world(world, body)
    assert errors == [None] * world, errors
    assert results[root] == want


# (encode_images takes one kind of target: every flow but the mixed search)
@pytest.mark.parametrize("name,mode,method,search", FLOWS[:-1], ids=FLOW_IDS[:-1])
def test_encode_images_packed_equals_unpacked(engine, name, mode, method, search):
    imgs = _imgs([(64, 64), (250, 130), (1, 1), (640, 480), (97, 61), (1, 37), (1920, 1080)])
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    kw = dict(quality=Q, yuv_mode=mode, engine=engine)
    if method >= 7:
        kw.update(method=method, use_trellis=True)
    else:
        kw.update(method=method)
    if search is not None:
        key = "target_size" if search["target_mode"] == sj.TARGET_SIZE else "target_psnr"
        kw.update({key: search["target_value"], "passes": search["passes"]})
    want = sj.encode_images(dev, packed=False, **kw)
    assert sj.encode_images(dev, packed=True, **kw) == want


def test_compress_images_packed_equals_unpacked(engine):
    imgs = _imgs()
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    for trellis in (False, True):
        want = sj.compress_images(dev, Q, engine=engine, use_trellis=trellis)
        assert sj.compress_images(dev, Q, engine=engine, use_trellis=trellis, packed=True) == want


def test_full_first_pool_is_retried(engine, oracle):
    """Noise at quality 100, 4:4:4: the JPEGs are larger than the first pool (2048 + half a byte per sample a picture),
    so the first packed call drops pictures and the second one codes exactly those."""
    dims = [(256, 256), (300, 200), (64, 64), (256, 192)]
    imgs = [synth.g_noise(w, h, 90 + k) for k, (w, h) in enumerate(dims)]
    want = [oracle.encode_method(im, 100.0, sj.YUV_444, 0) for im in imgs]
    first_pool = sum((2048 + (3 * w * h) // 2 + 15) & ~15 for (w, h) in dims)
    assert first_pool > 65536                                 # (the call's floor does not hide it)
    assert sum((len(w) + 15) & ~15 for w in want) > first_pool
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    before = sj.packed_stats()
    got = sj.encode_images(dev, 100.0, sj.YUV_444, engine=engine, packed=True)
    after = sj.packed_stats()
    assert got == want
    assert after["calls"] == before["calls"] + 1 and after["retries"] == before["retries"] + 1
    # ... and a batch that fits does not retry
    small = [torch.from_numpy(synth.g_struct(64, 64, 1)).cuda()]
    assert sj.encode_images(small, 75.0, engine=engine, packed=True) == [oracle.encode(synth.g_struct(64, 64, 1), 75.0, sj.YUV_420)]
    assert sj.packed_stats()["retries"] == after["retries"]


def test_method_0_packed_ignores_what_the_unpacked_path_ignores(engine):
    """encode_images method 0 with a fixed sampling codes with the tables of the quality alone (make_tables): min_quant
    and q_bias do not reach it, packed or not."""
    imgs = _imgs([(64, 64), (250, 130), (97, 61)])
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    mq = np.full((2, 64), 9, np.uint8)
    for mode in (sj.YUV_420, sj.YUV_444):
        want = sj.encode_images(dev, 90.0, mode, engine=engine, method=0, min_quant=mq, q_bias=0x40)
        assert want == sj.encode_images(dev, 90.0, mode, engine=engine, method=0)
        assert sj.encode_images(dev, 90.0, mode, engine=engine, method=0, min_quant=mq, q_bias=0x40, packed=True) == want
    # ... and where the unpacked path hands them down (method 4), so does the packed one
    want = sj.encode_images(dev, 90.0, sj.YUV_420, engine=engine, method=4, min_quant=mq, q_bias=0x40)
    assert want != sj.encode_images(dev, 90.0, sj.YUV_420, engine=engine, method=4)
    assert sj.encode_images(dev, 90.0, sj.YUV_420, engine=engine, method=4, min_quant=mq, q_bias=0x40, packed=True) == want
