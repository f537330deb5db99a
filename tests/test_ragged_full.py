"""The search with any sampling and with the trellis over a ragged batch (sjpeg_hip_encode_ragged_full_src and its packed
twin): every picture's bytes against the oracle's encode_search (and the reference build's, where there is one) for that
picture alone -- SJPEG_YUV_AUTO and SJPEG_YUV_SHARP with a size or PSNR target, methods 7 and 8 with both, frames that
leave the search at different passes (both endings of Encoder::LoopScan), mixed targets, parts, the older flows through
the new entry, the host waits, and encode_images_full."""
import os

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import orc, refso, synth

pytestmark = pytest.mark.gpu

Q = 75.0
# 1 x 1; 17 x 9; one segment in 4:2:0 and 4:4:4; 2 / 3 / 1 segments; 4 / 7 / 3 segments (41 / 82 / 246 MCUs a segment)
SIZES = [(1, 1), (17, 9), (48, 40), (136, 104), (250, 130)]
# the same sizes with the contents turned round, so that every mode group holds frames of one and of several segments
SIZES10 = SIZES + [(250, 130), (136, 104), (48, 40), (17, 9), (136, 104)]


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


def _imgs(sizes, shift=0):
    return [_content(k + shift, w, h) for k, (w, h) in enumerate(sizes)]


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


def _sp(mode, value, passes=6, tol=1.0, qmin=0.0, qmax=100.0):
    return sj.SearchParams(mode, float(value), passes, float(tol), float(qmin), float(qmax))


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


_cache = {}


def _source(oracle, im, verdict):
    """(format, planes, yuv_mode) the oracle codes a picture of that verdict from: the sharp frames as planar 4:2:0."""
    if verdict == sj.YUV_SHARP:
        return orc.SRC_YUV420, list(oracle.sharp_yuv(im)), sj.YUV_420
    return orc.SRC_RGB, [im.reshape(im.shape[0], -1)], verdict


def _plain(oracle, im, verdict, method):
    key = ("plain", im.tobytes(), im.shape, verdict, method)
    if key not in _cache:
        fmt, planes, mode = _source(oracle, im, verdict)
        _cache[key] = oracle.encode_src(fmt, planes, im.shape[1], im.shape[0], _quant(), yuv_mode=mode, method=method)
    return _cache[key]


def _want(oracle, im, verdict, yuv_mode, method, sp):
    """What the reference's sjpeg::Encode() makes of the picture alone: the oracle's, checked against the reference
    build's own where that exists (it takes SJPEG_YUV_AUTO / SHARP itself)."""
    if sp is None or sp.passes <= 1:
        return _plain(oracle, im, verdict, method)
    key = ("search", im.tobytes(), im.shape, verdict, method, sp.target_mode, sp.target_value, sp.passes, sp.tolerance)
    if key not in _cache:
        fmt, planes, mode = _source(oracle, im, verdict)
        kw = dict(huffman=method not in (0, 3), adaptive=method >= 3, target_mode=sp.target_mode,
                  target_value=sp.target_value, passes=sp.passes, tolerance=sp.tolerance, qmin=sp.qmin, qmax=sp.qmax,
                  trellis=method >= 7)
        _cache[key] = oracle.encode_search(fmt, planes, im.shape[1], im.shape[0], _quant(), yuv_mode=mode, **kw)
        if refso.available():
            assert _cache[key] == refso.ref().encode_search(im, Q, yuv_mode, **kw), ("oracle != reference", im.shape)
    return _cache[key]


def _verdicts(oracle, imgs, yuv_mode, table):
    if yuv_mode == sj.YUV_AUTO:
        return [oracle.riskiness(im, table)[0] for im in imgs]
    return [yuv_mode] * len(imgs)


def _size_targets(oracle, imgs, verdicts, method, passes=6, frac=0.6):
    return [_sp(sj.TARGET_SIZE, int(frac * len(_plain(oracle, im, v, method))), passes) for im, v in zip(imgs, verdicts)]


def _full(eng, imgs, yuv_mode, method, search):
    out, sizes, offs, modes, q, v = eng.encode_ragged_full(sj.SRC_RGB, _dev(imgs), _dims(imgs), yuv_mode, _quant(), method,
                                                           search=search)
    eng.wait()
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    return [host[o:o + int(s)].tobytes() if s > 0 else b"" for o, s in zip(offs, sz)], modes, q, v, eng.search_stats()


def _full_packed(eng, imgs, yuv_mode, method, search):
    out, sizes, offsets, modes, q, v = eng.encode_ragged_full_packed(sj.SRC_RGB, _dev(imgs), _dims(imgs), yuv_mode, _quant(),
                                                                     method, search=search)
    eng.wait()
    torch.cuda.synchronize()
    host, sz, off = out.cpu().numpy(), sizes.cpu().numpy(), offsets.cpu().numpy()
    return [host[int(o):int(o) + int(s)].tobytes() if s > 0 else b"" for o, s in zip(off[:-1], sz)], sz, off, modes


def _check(oracle, got, imgs, verdicts, yuv_mode, method, search, what):
    for k, im in enumerate(imgs):
        assert got[k] == _want(oracle, im, verdicts[k], yuv_mode, method, search[k]), (what, k, im.shape, verdicts[k])


# ---- case 1 (and 7, 11): SJPEG_YUV_AUTO with a size target, method 4

def _case1(oracle, table):
    imgs = _imgs(SIZES10)
    verdicts = _verdicts(oracle, imgs, sj.YUV_AUTO, table)
    return imgs, verdicts, _size_targets(oracle, imgs, verdicts, 4)


def test_auto_with_a_size_target(engine, oracle, risk_table):
    imgs, verdicts, search = _case1(oracle, risk_table)
    assert len(set(verdicts)) >= 2, verdicts
    got, modes, q, v, stats = _full(engine, imgs, sj.YUV_AUTO, 4, search)
    print("case 1 verdicts", verdicts, "stats", stats)
    assert modes == verdicts
    _check(oracle, got, imgs, verdicts, sj.YUV_AUTO, 4, search, "auto-size")
    assert all(x >= 0 for x in q) and all(x > 0 for x in v)
    assert stats[0] >= 2 and stats[4] == len(imgs) and stats[3] == 0 and stats[5] == 0


# ---- case 2: SJPEG_YUV_SHARP with a PSNR target, method 6

def test_sharp_with_a_psnr_target(engine, oracle, risk_table):
    imgs = _imgs(SIZES)
    search = [_sp(sj.TARGET_PSNR, 38.0)] * len(imgs)
    got, modes, _, _, stats = _full(engine, imgs, sj.YUV_SHARP, 6, search)
    print("case 2 stats", stats)
    assert modes == [sj.YUV_SHARP] * len(imgs)
    _check(oracle, got, imgs, modes, sj.YUV_SHARP, 6, search, "sharp-psnr")


# ---- case 3 (and 7): method 7, 4:2:0, a size target, the frames leave the search at different passes

def _case3(oracle):
    imgs = _imgs(SIZES + [(136, 104)])
    verdicts = [sj.YUV_420] * len(imgs)
    search = _size_targets(oracle, imgs, verdicts, 7)
    search[2] = _sp(sj.TARGET_SIZE, search[2].target_value, passes=2)
    search[3] = _sp(sj.TARGET_SIZE, search[3].target_value, passes=6, tol=50.0)
    return imgs, verdicts, search


def test_trellis_size_search_takes_both_endings(engine, oracle):
    imgs, verdicts, search = _case3(oracle)
    got, modes, _, _, stats = _full(engine, imgs, sj.YUV_420, 7, search)
    print("case 3 stats", stats)
    assert modes == verdicts
    _check(oracle, got, imgs, verdicts, sj.YUV_420, 7, search, "trellis-size")
    # both endings of Encoder::LoopScan (src/dichotomy.cc:178-201): frames whose last pass was their best replay its
    # blocks; the others are quantized once more
    assert stats[3] > 0 and stats[4] > 0 and stats[3] + stats[4] == len(imgs)
    assert stats[5] >= stats[0] + 1


# ---- case 4 (and 10): method 8, SJPEG_YUV_AUTO, a size target: groups x trellis

def _case4(oracle, table):
    imgs = _imgs(SIZES + [(136, 104)], shift=1)
    verdicts = _verdicts(oracle, imgs, sj.YUV_AUTO, table)
    return imgs, verdicts, _size_targets(oracle, imgs, verdicts, 8, passes=5)


def test_trellis_auto_size_search_and_its_waits(engine, oracle, risk_table):
    imgs, verdicts, search = _case4(oracle, risk_table)
    assert len(set(verdicts)) >= 2, verdicts
    got, modes, _, _, stats = _full(engine, imgs, sj.YUV_AUTO, 8, search)
    print("case 4 verdicts", verdicts, "stats", stats)
    assert modes == verdicts
    _check(oracle, got, imgs, verdicts, sj.YUV_AUTO, 8, search, "trellis-auto-size")
    # the riskiness wait, two waits per pass, the final statistics wait, one spare for a recount -- whatever the groups
    P = stats[0]
    assert 2 <= P <= 5
    assert stats[2] <= 1 + 2 * P + 1 + 1
    # the same batch restricted to its 4:2:0 frames: the same bound per pass
    sub = [k for k, v in enumerate(verdicts) if v == sj.YUV_420]
    if sub:
        got1, modes1, _, _, stats1 = _full(engine, [imgs[k] for k in sub], sj.YUV_AUTO, 8, [search[k] for k in sub])
        print("case 10 one group stats", stats1)
        assert got1 == [got[k] for k in sub]
        assert stats1[2] <= 1 + 2 * stats1[0] + 1 + 1
        # (the waits of the whole batch are those of its longest search, not a sum over its groups)
        assert stats[2] - 2 * P <= stats1[2] - 2 * stats1[0] + 1


# ---- case 5: method 7, 4:4:4, a PSNR target

def test_trellis_444_with_a_psnr_target(engine, oracle):
    imgs = _imgs(SIZES)
    search = [_sp(sj.TARGET_PSNR, 38.0, passes=5)] * len(imgs)
    got, modes, _, _, stats = _full(engine, imgs, sj.YUV_444, 7, search)
    print("case 5 stats", stats)
    _check(oracle, got, imgs, [sj.YUV_444] * len(imgs), sj.YUV_444, 7, search, "trellis-444-psnr")
    assert stats[3] == 0 and stats[4] == len(imgs)          # (a PSNR search always ends with one trellis quantization)


# ---- case 6: some frames not searched, size and PSNR targets in one call

@pytest.mark.parametrize("method", [4, 7])
def test_mixed_targets_and_unsearched_frames(engine, oracle, risk_table, method):
    imgs = _imgs(SIZES10)
    verdicts = _verdicts(oracle, imgs, sj.YUV_AUTO, risk_table)
    size = _size_targets(oracle, imgs, verdicts, method, passes=4)
    search = [size[k] if k % 3 == 0 else _sp(sj.TARGET_PSNR, 36.0, passes=4) if k % 3 == 1 else
              _sp(sj.TARGET_SIZE, 100.0, passes=1) for k in range(len(imgs))]
    got, modes, q, v, stats = _full(engine, imgs, sj.YUV_AUTO, method, search)
    print("case 6 method", method, "stats", stats)
    assert modes == verdicts
    _check(oracle, got, imgs, verdicts, sj.YUV_AUTO, method, search, "mixed")
    for k in range(len(imgs)):
        assert (q[k] == -1.0 and v[k] == -1.0) if k % 3 == 2 else (q[k] >= 0.0 and v[k] > 0.0), k


# ---- case 7: the packed twin of cases 1 and 3

@pytest.mark.parametrize("case", [1, 3])
def test_the_packed_twin(engine, oracle, risk_table, case):
    if case == 1:
        imgs, verdicts, search = _case1(oracle, risk_table)
        yuv_mode, method = sj.YUV_AUTO, 4
    else:
        imgs, verdicts, search = _case3(oracle)
        yuv_mode, method = sj.YUV_420, 7
    want, modes, _, _, _ = _full(engine, imgs, yuv_mode, method, search)
    got, sz, off, pmodes = _full_packed(engine, imgs, yuv_mode, method, search)
    assert got == want and pmodes == modes and all(len(b) > 0 for b in got)
    assert (off % 16 == 0).all()
    assert int(off[-1]) == int(((sz + 15) & ~15).sum())
    # back to back: the frames' padded ranges tile [0, offsets[n])
    order = np.argsort(off[:-1])
    at = 0
    for k in order:
        assert int(off[k]) == at, k
        at += (int(sz[k]) + 15) & ~15


# ---- case 8: a scratch limit that cuts the call into parts

def test_parts_give_the_same_bytes(monkeypatch, oracle, risk_table):
    imgs, verdicts, search = _case4(oracle, risk_table)
    eng = sj.Engine(0)
    want, modes, _, _, whole = _full(eng, imgs, sj.YUV_AUTO, 8, search)
    eng.close()
    monkeypatch.setenv("SJPEG_HIP_SCRATCH_LIMIT_BYTES", "1")
    small = sj.Engine(0)                                   # (made after the limit is set: every frame its own part)
    got, modes1, _, _, parts = _full(small, imgs, sj.YUV_AUTO, 8, search)
    print("case 8 stats", whole, parts)
    assert got == want and modes1 == modes
    assert parts[2] > whole[2]                             # (every part a complete search with its own waits)
    assert parts[3] == whole[3] and parts[4] == whole[4]
    small.close()


# ---- case 9: old ground through the new door

def test_old_ground_gives_the_old_bytes(engine, risk_table):
    imgs = _imgs(SIZES10)
    planes, dims = _dev(imgs), _dims(imgs)

    def frames(out, sizes, offs):
        engine.wait()
        torch.cuda.synchronize()
        host, sz = out.cpu().numpy(), sizes.cpu().numpy()
        return [host[o:o + int(s)].tobytes() for o, s in zip(offs, sz)]

    sp = [_sp(sj.TARGET_SIZE, 900.0, passes=4)] * len(imgs)
    out, sizes, offs, _, _ = engine.encode_ragged_search(sj.SRC_RGB, planes, dims, sj.YUV_420, _quant(), sp, 4)
    got, modes, q, _, stats = _full(engine, imgs, sj.YUV_420, 4, sp)
    assert got == frames(out, sizes, offs) and modes == [sj.YUV_420] * len(imgs) and all(x >= 0 for x in q)
    assert stats == [0] * 6
    out, sizes, offs, m7 = engine.encode_ragged_trellis(sj.SRC_RGB, planes, dims, sj.YUV_AUTO, _quant(), 7)
    got, modes, q, _, _ = _full(engine, imgs, sj.YUV_AUTO, 7, None)
    assert got == frames(out, sizes, offs) and modes == m7 and q == [-1.0] * len(imgs)
    out, sizes, offs, m4 = engine.encode_ragged_auto(sj.SRC_RGB, planes, dims, sj.YUV_AUTO, _quant(), 4)
    got, modes, _, _, _ = _full(engine, imgs, sj.YUV_AUTO, 4, None)
    assert got == frames(out, sizes, offs) and modes == m4


# ---- case 11: encode_images_full with the defaults

def test_encode_images_full(engine, oracle, risk_table):
    imgs, verdicts, search = _case1(oracle, risk_table)
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    targets = [sp.target_value for sp in search]
    want = [_want(oracle, im, v, sj.YUV_AUTO, 4, _sp(sj.TARGET_SIZE, t, passes=10)) for im, v, t in zip(imgs, verdicts, targets)]
    got = sj.encode_images_full(dev, target_size=targets, engine=engine)
    assert got == want
    before = sj.packed_stats()["calls"]
    assert sj.encode_images_full(dev, target_size=targets, engine=engine, packed=True) == got
    assert sj.packed_stats()["calls"] == before + 1
    # without a target: the batch SjpegCompress()
    assert sj.encode_images_full(dev, engine=engine) == sj.compress_images(dev, engine=engine)
