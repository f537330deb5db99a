"""Ragged batches searched to a target size or PSNR (sjpeg_hip_encode_ragged_search_src): the two new measurement passes
against the uniform pass and the oracle picture by picture, every searched frame against the oracle's encode_search,
the unsearched call against encode_ragged_batch, split launches, capacity, concurrency and encode_images."""
import os
import subprocess
import threading

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import orc, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [(1, 1), (7, 13), (17, 13), (1, 300), (300, 1), (250, 130), (640, 480), (1920, 1080), (3840, 2160)]
SMALL = [(1, 1), (7, 13), (17, 13), (1, 300), (300, 1), (250, 130), (97, 61)]
MODES = [sj.YUV_420, sj.YUV_444, sj.YUV_400]


def _content(k, w, h):
    if k % 3 == 0:
        return synth.g_struct(w, h, 1000 + k)
    if k % 3 == 1:
        return synth.g_noise(w, h, 2000 + k)
    return np.full((h, w, 3), (37 * k) % 256, np.uint8)


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


def _quant(q):
    m = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(float(q), m.ctypes.data)
    return m


def _frames(out, sizes, offs):
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    sz = sizes.cpu().numpy()
    return [host[o:o + int(s)].tobytes() if s > 0 else b"" for o, s in zip(offs, sz)]


def _rgb2d(im):
    return [im.reshape(im.shape[0], -1)]


def _search(mode, value, passes=10, tol=1.0, qmin=0.0, qmax=100.0):
    return sj.SearchParams(mode, float(value), passes, float(tol), float(qmin), float(qmax))


def _want(oracle, im, q, yuv, method, sp):
    h, w, _ = im.shape
    return oracle.encode_search(orc.SRC_RGB, _rgb2d(im), w, h, _quant(q), yuv_mode=yuv,
                                huffman=method not in (0, 3), adaptive=method >= 3, target_mode=sp.target_mode,
                                target_value=sp.target_value, passes=sp.passes, tolerance=sp.tolerance,
                                qmin=sp.qmin, qmax=sp.qmax)


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.mark.parametrize("mode", MODES)
def test_quant_error_ragged(engine, oracle, mode):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(SIZES)]
    dev = _dev(imgs)
    qs = [(8.0, 60.0, 97.0)[k % 3] for k in range(len(imgs))]
    made = [sj.make_tables(quality=q) for q in qs]
    per = engine.scan_quant_error_ragged(sj.SRC_RGB, dev, _dims(imgs), mode, [t for t, _ in made]).cpu().numpy()
    shared = engine.scan_quant_error_ragged(sj.SRC_RGB, dev, _dims(imgs), mode, made[1][0]).cpu().numpy()
    for k, im in enumerate(imgs):
        h, w, _ = im.shape
        one = dev[k][0].contiguous().unsqueeze(0)          # (alive while the uniform pass reads it)
        src, n = sj.make_source(sj.SRC_RGB, [one])
        assert int(per[k]) == int(engine.scan_quant_error_source(src, n, w, h, made[k][0], mode)[0].item()), (k, w, h)
        assert int(per[k]) == oracle.quant_error(orc.SRC_RGB, _rgb2d(im), w, h, made[k][1], yuv_mode=mode), (k, w, h)
        assert int(shared[k]) == oracle.quant_error(orc.SRC_RGB, _rgb2d(im), w, h, made[1][1], yuv_mode=mode), (k, w, h)
    # one picture alone in a ragged call is the same total as inside the batch
    alone = engine.scan_quant_error_ragged(sj.SRC_RGB, [dev[5]], [_dims(imgs)[5]], mode, made[5][0]).cpu().numpy()
    assert int(alone[0]) == int(per[5])


@pytest.mark.parametrize("mode", MODES)
def test_counted_bits_ragged(engine, oracle, mode):
    sizes = SIZES[:7] + [(640, 480), (320, 240)]
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(sizes)]
    imgs[-1] = synth.g_noise(320, 240, 77)                 # q 100 noise: past the first plan, counted again
    imgs[-2] = synth.g_noise(640, 480, 78)
    qs = [(8.0, 60.0, 97.0)[k % 3] for k in range(len(imgs) - 2)] + [100.0, 100.0]
    made = [sj.make_tables(quality=q) for q in qs]
    bits = engine.scan_counted_bits_ragged(sj.SRC_RGB, _dev(imgs), _dims(imgs), mode,
                                           [t for t, _ in made]).cpu().numpy()
    for k, im in enumerate(imgs):
        h, w, _ = im.shape
        assert int(bits[k]) == oracle.counted_bits(orc.SRC_RGB, _rgb2d(im), w, h, made[k][1], yuv_mode=mode), (k, w, h)


@pytest.mark.parametrize("method", range(7))
@pytest.mark.parametrize("target_mode", [1, 2])
def test_search_equals_the_oracle(engine, oracle, method, target_mode):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(SMALL + [(640, 480)])]
    q75 = [len(oracle.encode_method(im, 75.0, sj.YUV_420, method)) for im in imgs]
    if target_mode == 1:                                   # per picture, below and above its q75 size
        search = [_search(1, q75[k] * (0.6 if k % 2 else 1.4)) for k in range(len(imgs))]
    else:
        search = [_search(2, (32.0, 38.0, 44.0)[k % 3]) for k in range(len(imgs))]
    out, sizes, offs, q, value = engine.encode_ragged_search(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_420,
                                                             _quant(75.0), search, method)
    got = _frames(out, sizes, offs)
    for k, im in enumerate(imgs):
        assert got[k] == _want(oracle, im, 75.0, sj.YUV_420, method, search[k]), (method, target_mode, k)
        assert 0.0 <= q[k] <= 100.0 and value[k] > 0.0


@pytest.mark.parametrize("mode", MODES)
def test_search_conditions(engine, oracle, mode):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(SMALL + [(640, 480), (1920, 1080)])]
    n = len(imgs)
    search = [_search(1, 100000000.0),                      # unreachable: pins qmax
              _search(1, 10.0),                             # unreachable: pins qmin
              _search(1, 3000.0, qmin=40.0, qmax=60.0),     # a narrow range
              _search(2, 40.0, tol=0.1),
              _search(2, 35.0, tol=5.0),
              _search(1, 20000.0, passes=3),                # frames that stop at different passes
              _search(2, 45.0, passes=20),
              _search(1, 40000.0, passes=6, tol=0.1),
              _search(2, 38.0)]
    assert len(search) == n
    quant = [_quant(q) for q in (20.0, 50.0, 75.0, 90.0, 75.0, 60.0, 30.0, 75.0, 80.0)]
    for method in (4, 0):
        out, sizes, offs, q, value = engine.encode_ragged_search(sj.SRC_RGB, _dev(imgs), _dims(imgs), mode, quant,
                                                                 search, method)
        got = _frames(out, sizes, offs)
        for k, im in enumerate(imgs):
            h, w, _ = im.shape
            sp = search[k]
            want = oracle.encode_search(orc.SRC_RGB, _rgb2d(im), w, h, quant[k], yuv_mode=mode,
                                        huffman=method != 0, adaptive=method >= 3, target_mode=sp.target_mode,
                                        target_value=sp.target_value, passes=sp.passes, tolerance=sp.tolerance,
                                        qmin=sp.qmin, qmax=sp.qmax)
            assert got[k] == want, (mode, method, k)


def _layout_planes(rng, fmt, w, h):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    shapes = {2: [(h, 4 * w)], 3: [(h, w)], 5: [(h, w), (ch, cw), (ch, cw)], 6: [(h, w), (ch, 2 * cw)]}[fmt]
    return [(rng.randint(0, 64, s) + np.arange(s[1])[None, :] // 3).astype(np.uint8) for s in shapes]


@pytest.mark.parametrize("fmt", [orc.SRC_RGB, 2, 3, 5, 6])
def test_source_formats(engine, oracle, fmt):
    rng = np.random.RandomState(900 + fmt)
    mode = sj.YUV_400 if fmt == 3 else sj.YUV_420
    dims = [(1, 1), (17, 13), (250, 130), (97, 61)]
    if fmt == orc.SRC_RGB:
        host = [_rgb2d(_content(k, w, h)) for k, (w, h) in enumerate(dims)]
    else:
        host = [_layout_planes(rng, fmt, w, h) for (w, h) in dims]
    dev = [[torch.from_numpy(p).cuda() for p in planes] for planes in host]
    search = [_search(1, 1500.0), _search(2, 36.0), _search(1, 4000.0), _search(2, 42.0)]
    for method in (4, 3, 1):
        out, sizes, offs, _, _ = engine.encode_ragged_search(fmt, dev, dims, mode, _quant(70.0), search, method)
        got = _frames(out, sizes, offs)
        for k, (w, h) in enumerate(dims):
            sp = search[k]
            want = oracle.encode_search(fmt, host[k], w, h, _quant(70.0), yuv_mode=mode, huffman=method not in (0, 3),
                                        adaptive=method >= 3, target_mode=sp.target_mode, target_value=sp.target_value,
                                        passes=sp.passes, tolerance=sp.tolerance, qmin=sp.qmin, qmax=sp.qmax)
            assert got[k] == want, (fmt, method, k)


def test_unsearched_call_is_the_batch_call(engine):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(SMALL + [(640, 480)])]
    search = [_search(1, 5000.0, passes=p) for p in (1, 0, -3, 1, 1, 1, 1, 1)]
    for method in (0, 4, 6):
        want = _frames(*engine.encode_ragged_batch(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_420, _quant(75.0),
                                                   method))
        out, sizes, offs, q, value = engine.encode_ragged_search(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_420,
                                                                 _quant(75.0), search, method)
        assert _frames(out, sizes, offs) == want
        assert q == [-1.0] * len(imgs) and value == [-1.0] * len(imgs)


def test_mixed_searched_and_plain_frames(engine, oracle):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(SMALL)]
    search = [_search(2, 40.0, passes=(1 if k % 2 else 10)) for k in range(len(imgs))]
    plain = _frames(*engine.encode_ragged_batch(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_420, _quant(75.0), 4))
    out, sizes, offs, q, _ = engine.encode_ragged_search(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_420,
                                                         _quant(75.0), search, 4)
    got = _frames(out, sizes, offs)
    for k, im in enumerate(imgs):
        if k % 2:
            assert got[k] == plain[k] and q[k] == -1.0
        else:
            assert got[k] == _want(oracle, im, 75.0, sj.YUV_420, 4, search[k])


def test_split_launches(monkeypatch):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(SMALL + [(640, 480), (1920, 1080)])]
    search = [_search(1 + k % 2, (3000.0 if k % 2 == 0 else 38.0)) for k in range(len(imgs))]
    eng = sj.Engine(0)
    want = eng.encode_ragged_search(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_420, _quant(75.0), search, 4)
    want_bytes = _frames(*want[:3])
    eng.close()
    monkeypatch.setenv("SJPEG_HIP_SCRATCH_LIMIT_BYTES", "1")
    small = sj.Engine(0)
    got = small.encode_ragged_search(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_420, _quant(75.0), search, 4)
    assert _frames(*got[:3]) == want_bytes
    assert got[3:] == want[3:]
    small.close()


@pytest.mark.parametrize("method", [0, 3, 4])
def test_both_kinds_an_unsearched_frame_and_parts_in_one_call(monkeypatch, oracle, method):
    """Size and PSNR targets, a frame that is not searched and a part split in one call: every frame is the oracle's,
    the split call equals the unsplit one, and the packed twin codes the unsearched frame first.  (On the oracle, with
    these targets, frames 0 and 4 -- size -- and 1 and 5 -- PSNR -- still change between 3 and 4 passes, whatever the
    method: no search here stops at its first pass.)"""
    dims = [(1, 1), (17, 13), (48, 40), (136, 104), (250, 130), (136, 104)]
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(dims)]
    q75 = [len(oracle.encode_method(im, 75.0, sj.YUV_420, method)) for im in imgs]
    search = [_search(1, q75[k] * 0.5, passes=4) if k % 2 == 0 else _search(2, 38.0, passes=4) for k in range(len(imgs))]
    search[2].passes = 1
    want = [_want(oracle, im, 75.0, sj.YUV_420, method, search[k]) for k, im in enumerate(imgs)]
    args = (sj.SRC_RGB, _dev(imgs), dims, sj.YUV_420, _quant(75.0))
    eng = sj.Engine(0)
    whole = eng.encode_ragged_search(*args, search, method)
    whole_bytes = _frames(*whole[:3])
    out, sizes, offsets, _, pq, pvalue = eng.encode_ragged_packed(*args, method, search=search)
    off, sz, host = offsets.cpu().tolist(), sizes.cpu().tolist(), out.cpu().numpy()
    eng.close()
    monkeypatch.setenv("SJPEG_HIP_SCRATCH_LIMIT_BYTES", "1")      # (every searched frame a part of its own)
    small = sj.Engine(0)
    split = small.encode_ragged_search(*args, search, method)
    split_bytes = _frames(*split[:3])
    small.close()
    for k in range(len(imgs)):
        assert whole_bytes[k] == want[k], (method, k)
    assert split_bytes == whole_bytes and split[3:] == whole[3:]
    q, value = whole[3:]
    assert [k for k in range(len(imgs)) if q[k] == -1.0] == [2] and [k for k in range(len(imgs)) if value[k] == -1.0] == [2]
    assert off[2] == 0 and all(off[k] > 0 for k in range(len(imgs)) if k != 2)
    assert [host[off[k]:off[k] + sz[k]].tobytes() for k in range(len(imgs))] == want
    assert (pq, pvalue) == (q, value)


def test_capacity(engine, oracle):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate([(64, 64), (250, 130), (97, 61), (640, 480)])]
    search = _search(1, 6000.0)
    caps = [sj.frame_bound(w, h, sj.YUV_420, 2048) for (w, h) in _dims(imgs)]
    caps[1] = 100
    out, sizes, offs, _, _ = engine.encode_ragged_search(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_420, _quant(75.0),
                                                         search, 4, capacities=caps)
    got = _frames(out, sizes, offs)
    assert got[1] == b""
    for k in (0, 2, 3):
        assert got[k] == _want(oracle, imgs[k], 75.0, sj.YUV_420, 4, search)


def test_threads_and_back_to_back():
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(SMALL + [(640, 480)])]
    search = [_search(1 + k % 2, (2500.0 if k % 2 == 0 else 40.0)) for k in range(len(imgs))]
    ref = sj.Engine(0)
    want = _frames(*ref.encode_ragged_search(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_420, _quant(75.0), search,
                                             4)[:3])
    a = ref.encode_ragged_search(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_420, _quant(75.0), search, 4)
    b = ref.encode_ragged_search(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_420, _quant(75.0), search, 4)
    assert _frames(*a[:3]) == want and _frames(*b[:3]) == want
    results = [None, None]

    def run(i):
        eng = sj.Engine(0)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            r = eng.encode_ragged_search(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_420, _quant(75.0), search, 4)
            s.synchronize()
            results[i] = _frames(*r[:3])
        eng.close()

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert results == [want, want]
    ref.close()


def test_two_engines_two_streams_one_thread():
    """Two engines, each on its own stream, called back to back from one thread with no wait in between: neither
    call's queued work may share memory with the other's."""
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(SMALL + [(640, 480)])]
    other = [_content(k + 5, w, h) for k, (w, h) in enumerate(SMALL + [(320, 240)])]
    search = [_search(1 + k % 2, (2500.0 if k % 2 == 0 else 40.0), passes=(1 if k == 3 else 10))
              for k in range(len(imgs))]
    ref = sj.Engine(0)
    want_a = _frames(*ref.encode_ragged_search(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_420, _quant(75.0), search,
                                               4)[:3])
    want_b = _frames(*ref.encode_ragged_search(sj.SRC_RGB, _dev(other), _dims(other), sj.YUV_420, _quant(60.0), search,
                                               0)[:3])
    ref.close()
    ea, eb = sj.Engine(0), sj.Engine(0)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    da, db = _dev(imgs), _dev(other)
    torch.cuda.synchronize()
    for _ in range(3):
        with torch.cuda.stream(sa):
            ra = ea.encode_ragged_search(sj.SRC_RGB, da, _dims(imgs), sj.YUV_420, _quant(75.0), search, 4)
        with torch.cuda.stream(sb):
            rb = eb.encode_ragged_search(sj.SRC_RGB, db, _dims(other), sj.YUV_420, _quant(60.0), search, 0)
        torch.cuda.synchronize()
        assert _frames(*ra[:3]) == want_a
        assert _frames(*rb[:3]) == want_b
    ea.close()
    eb.close()


def test_q_and_value_equal_the_cxx_search_hook(tmp_path, engine):
    """q_out / value_out are the floats a SearchHook holds after sjpeg::Encode of the picture alone (best q and best
    result), and the bytes are that call's."""
    exe = str(tmp_path / "search_hook_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "search_hook_test.cc"), "-o", exe, "-L", sj.CSRC,
                           "-lsjpeg_amd", "-lpthread", "-Wl,-rpath," + sj.CSRC, "-Wl,-rpath-link,/opt/rocm/lib"])
    dims = [(17, 13), (250, 130), (97, 61), (640, 480), (300, 1)]
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(dims)]
    search = [_search(1, 3000.0), _search(2, 38.0, passes=6), _search(1, 1200.0, tol=0.1, qmin=20.0, qmax=90.0),
              _search(2, 44.0, tol=5.0), _search(1, 400.0)]
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    lines = []
    for method in (4, 1, 0):
        lines.clear()
        for k, im in enumerate(imgs):
            path = tmp_path / f"{k}.rgb"
            path.write_bytes(im.tobytes())
            sp = search[k]
            lines.append(f"{path} {dims[k][0]} {dims[k][1]} 75 {method} {sj.YUV_420} {sp.target_mode} "
                         f"{sp.target_value!r} {sp.passes} {sp.tolerance!r} {sp.qmin!r} {sp.qmax!r}")
        (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
        env = dict(os.environ)
        env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
        r = subprocess.run([exe, str(tmp_path / "cases.txt"), str(out_dir)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        hook = {}
        for row in r.stdout.split("\n"):
            if row.strip():
                i, q, v = row.split()
                hook[int(i)] = (float.fromhex(q), float.fromhex(v))
        out, sizes, offs, q, value = engine.encode_ragged_search(sj.SRC_RGB, _dev(imgs), dims, sj.YUV_420,
                                                                 _quant(75.0), search, method)
        got = _frames(out, sizes, offs)
        for k in range(len(imgs)):
            assert (q[k], value[k]) == hook[k], (method, k)
            assert got[k] == (out_dir / f"{k}.jpg").read_bytes(), (method, k)


def test_encode_images_targets(oracle):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate([(17, 13), (250, 130), (97, 61), (640, 480)])]
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    sizes = [800.0, 5000.0, 1500.0, 20000.0]
    got = sj.encode_images(dev, 75.0, method=4, target_size=sizes)
    for k, im in enumerate(imgs):
        assert got[k] == _want(oracle, im, 75.0, sj.YUV_420, 4, _search(1, sizes[k]))
    got = sj.encode_images(dev, 60.0, method=1, target_psnr=41.0, passes=6, tolerance=0.5, qmin=10.0, qmax=95.0)
    for k, im in enumerate(imgs):
        assert got[k] == _want(oracle, im, 60.0, sj.YUV_420, 1, _search(2, 41.0, 6, 0.5, 10.0, 95.0))
    assert sj.encode_images(dev, 75.0, method=4) == sj.encode_images(dev, 75.0, method=4, passes=3)
    with pytest.raises(sj.SjpegError, match="one target per image"):
        sj.encode_images(dev, 75.0, method=4, target_size=[1000.0])
    with pytest.raises(sj.SjpegError, match="not both"):
        sj.encode_images(dev, target_size=1000.0, target_psnr=40.0)
