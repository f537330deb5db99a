"""Ragged batches with SJPEG_YUV_AUTO and the sharp conversion (sjpeg_hip_riskiness_ragged_src,
sjpeg_hip_sharp_yuv_ragged, sjpeg_hip_encode_ragged_auto_src): every frame against the per-picture device calls and the
oracle, BASELINE config #1 inside a batch, explicit SHARP, capacity, split launches, concurrency and bad arguments."""
import ctypes as C
import hashlib
import os
import threading

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def risk_table():
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        tab = f.read()
    assert len(tab) == 117649
    sj.set_riskiness_table(tab)
    return tab


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


def _content(k, w, h):
    """Content whose verdicts cover 4:2:0, sharp, 4:4:4 and 4:0:0."""
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


def _gradient(w, h):
    x = np.arange(w)[None, :] * 200 // w
    y = np.arange(h)[:, None] * 200 // h
    return np.stack([np.broadcast_to(x + 20, (h, w)), np.broadcast_to(y + 30, (h, w)), np.full((h, w), 90)],
                    2).astype(np.uint8)


def _test128():
    return np.fromfile(os.path.join(ROOT, "tests", "golden", "test128.rgb"), np.uint8).reshape(128, 128, 3)


def _dev(imgs, pad=16, fmt=sj.SRC_RGB, flip=False):
    """One device allocation per picture, rows padded by `pad` bytes: [rows, bpp w] views, or (address of row 0,
    negative stride) pairs with the rows stored bottom-up."""
    out = []
    bpp = 3 if fmt == sj.SRC_RGB else 4
    for im in imgs:
        h, w, _ = im.shape
        px = im
        if fmt == sj.SRC_BGRA:
            px = np.concatenate([im[:, :, 2:3], im[:, :, 1:2], im[:, :, 0:1], np.full((h, w, 1), 7, np.uint8)], 2)
        elif fmt == sj.SRC_RGBA:
            px = np.concatenate([im, np.full((h, w, 1), 9, np.uint8)], 2)
        buf = np.zeros((h, bpp * w + pad), np.uint8)
        buf[:, :bpp * w] = px.reshape(h, bpp * w)
        if flip:
            t = torch.from_numpy(buf[::-1].copy()).cuda()
            out.append([(t.data_ptr() + (h - 1) * t.stride(0), -t.stride(0))])
            _KEEP.append(t)
        else:
            out.append([torch.from_numpy(buf).cuda()[:, :bpp * w]])
    return out


_KEEP = []


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


def _uniform_sums(im, fmt=sj.SRC_RGB):
    """sjpeg_hip_riskiness_sums of one picture alone."""
    d = _dev([im], fmt=fmt)[0][0]
    src, _ = sj.make_source(fmt, [d.unsqueeze(0)])
    tab = torch.frombuffer(bytearray(open(os.path.join(sj.CSRC, "riskiness.bin"), "rb").read()), dtype=torch.uint8).cuda()
    sums = torch.zeros(3, dtype=torch.int64, device="cuda")
    # (a prototype of its own: the shared library object's argtypes stay as they are)
    proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
    fn = C.cast(sj.lib().sjpeg_hip_riskiness_sums, proto)
    assert fn(C.addressof(src), im.shape[1], im.shape[0], 1, tab.data_ptr(), sums.data_ptr(),
              torch.cuda.current_stream().cuda_stream) == 0
    return sums.cpu().numpy()


# ---- 1. ragged riskiness

def test_riskiness_ragged_equals_uniform_and_oracle(engine, oracle, risk_table):
    rng = np.random.RandomState(71)
    dims = [(1, 1), (1, 300), (300, 1), (2, 2), (7, 13), (33, 200), (1920, 1080)]
    dims += [(int(rng.randint(1, 320)), int(rng.randint(1, 240))) for _ in range(600)]
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(dims)]
    sums = engine.riskiness_ragged(sj.SRC_RGB, _dev(imgs), _dims(imgs)).cpu().numpy()
    for k in (0, 1, 2):
        assert (sums[k] == 0).all()
    seen = set()
    for k, im in enumerate(imgs):
        if k < 40 or k % 10 == 0:
            assert (sums[k] == _uniform_sums(im)).all(), (k, im.shape)
        got = sj.riskiness_verdict(sums[k], im.shape[1], im.shape[0])
        want = oracle.riskiness(im, risk_table)
        assert got == want, (k, im.shape, got, want)
        seen.add(got[0])
    assert len(seen) >= 3
    got = sj.riskiness_images([torch.from_numpy(im).cuda() for im in imgs[:60]])
    assert got == [oracle.riskiness(im, risk_table) for im in imgs[:60]]


def test_riskiness_follows_the_installed_table(engine, oracle, risk_table):
    # another table installed: riskiness_images, the ragged sums with no table given and the AUTO call all follow it,
    # as SjpegRiskiness does
    imgs = [_content(k, w, h) for k, (w, h) in enumerate([(97, 61), (300, 200), (64, 64), (128, 90), (33, 200)])]
    imgs[0] = _test128()
    other = bytes((b * 3 + 1) % 17 for b in risk_table)
    try:
        sj.set_riskiness_table(other)
        got = sj.riskiness_images([torch.from_numpy(im).cuda() for im in imgs])
        want = [sj.SjpegRiskiness(im) for im in imgs]
        assert got == want == [oracle.riskiness(im, other) for im in imgs]
        assert got != [oracle.riskiness(im, risk_table) for im in imgs]
        out, sizes, offs, modes = engine.encode_ragged_auto(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_AUTO,
                                                            _quant(75.0), 4)
        assert modes == [m for m, _ in want]
        assert _frames(out, sizes, offs) == [sj.SjpegEncode(im, 75.0, 4, sj.YUV_AUTO) for im in imgs]
    finally:
        sj.set_riskiness_table(risk_table)


@pytest.mark.parametrize("fmt,flip", [(sj.SRC_BGRA, False), (sj.SRC_RGBA, False), (sj.SRC_RGB, True),
                                      (sj.SRC_BGRA, True)])
def test_riskiness_ragged_layouts(engine, oracle, risk_table, fmt, flip):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate([(1, 5), (5, 1), (3, 3), (97, 61), (300, 200), (640, 480)])]
    sums = engine.riskiness_ragged(fmt, _dev(imgs, pad=20, fmt=fmt, flip=flip), _dims(imgs)).cpu().numpy()
    want = engine.riskiness_ragged(sj.SRC_RGB, _dev(imgs), _dims(imgs)).cpu().numpy()
    assert (sums == want).all()
    for k, im in enumerate(imgs):
        assert sj.riskiness_verdict(sums[k], im.shape[1], im.shape[0]) == oracle.riskiness(im, risk_table)


# ---- 2. ragged sharp planes

def _sharp_check(engine, imgs, oracle=None, fmt=sj.SRC_RGB, flip=False):
    planes = engine.sharp_yuv_ragged(fmt, _dev(imgs, fmt=fmt, flip=flip), _dims(imgs))
    torch.cuda.synchronize()
    for k, im in enumerate(imgs):
        h, w, _ = im.shape
        y, u, v = (p.cpu().numpy() for p in planes[k])
        uy, uu, uv = sj.sharp_yuv(sj.SRC_RGB, torch.from_numpy(np.ascontiguousarray(im.reshape(1, h, 3 * w))).cuda())
        assert (y == uy[0].cpu().numpy()).all() and (u == uu[0].cpu().numpy()).all() and (v == uv[0].cpu().numpy()).all(), (k, w, h)
        if oracle is not None:
            oy, ou, ov = oracle.sharp_yuv(im)
            assert (y == oy).all() and (u == ou).all() and (v == ov).all(), (k, w, h)


def test_sharp_ragged_planes(engine, oracle):
    dims = [(3, 9), (9, 3), (4, 4), (5, 5), (300, 1), (1, 300), (383, 2), (384 * 2, 17), (384 * 2 + 1, 9),
            (384 * 6 + 50, 6), (640, 480), (101, 67), (1920, 1080), (6, 1080)]
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(dims)]
    _sharp_check(engine, imgs, oracle)


def test_sharp_ragged_layouts(engine):
    imgs = [_content(k, w, h) for k, (w, h) in enumerate([(3, 9), (97, 61), (800, 33)])]
    _sharp_check(engine, imgs, fmt=sj.SRC_BGRA)
    _sharp_check(engine, imgs, fmt=sj.SRC_RGBA, flip=True)


def test_sharp_ragged_several_launches(engine):
    # 6 strips a frame, 24 workgroups: 120 frames hold more than one strips launch may (three quarters of the device)
    imgs = [_content(3 + 4 * k, 2304, 16) for k in range(120)] + [_content(1, 3, 9)]
    _sharp_check(engine, imgs)


_SEVERAL_LAUNCHES_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np, torch
import sjpeg_amd as sj
import test_ragged_auto as t
imgs = [t._content(3 + 4 * k, 2304, 16) for k in range(120)] + [t._content(1, 3, 9), t._content(0, 640, 480)]
t._sharp_check(sj.Engine(0), imgs)
print("child ok")
"""


def test_sharp_ragged_split_into_launches():
    # In a child process of its own (SJPEG_HIP_SHARP_DEBUG is read there): the library reports how many strips
    # launches the batch went in, and the planes still equal the uniform call's.
    import subprocess
    import sys
    env = dict(os.environ, SJPEG_HIP_SHARP_DEBUG="1")
    p = subprocess.run([sys.executable, "-c", _SEVERAL_LAUNCHES_CHILD, ROOT], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stderr[-2000:]
    lines = [ln for ln in p.stderr.splitlines() if ln.startswith("sharp ragged:")]
    assert len(lines) == 1, p.stderr[-2000:]
    launches = int(lines[0].split(" strips launches")[0].rsplit(" ", 1)[1])
    slots = int(lines[0].split("at most ")[1].split()[0])
    assert launches >= 2 and launches >= (121 * 24 + slots - 1) // slots, lines[0]


# ---- 3. the AUTO encode

MIXED = [(128, 128), (1, 1), (7, 13), (300, 1), (17, 130), (250, 130), (97, 61), (640, 480), (64, 64), (33, 200),
         (211, 97), (80, 64), (70, 50), (60, 90), (1920, 1080), (5, 300)]


def _mixed():
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(MIXED)]
    imgs[0] = _test128()
    return imgs


def test_auto_equals_host_api_per_picture(engine, oracle, risk_table):
    imgs = _mixed()
    verdicts = [oracle.riskiness(im, risk_table)[0] for im in imgs]
    assert {sj.YUV_420, sj.YUV_SHARP, sj.YUV_444, sj.YUV_400} <= set(verdicts), verdicts
    for m in range(7):
        out, sizes, offs, modes = engine.encode_ragged_auto(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_AUTO,
                                                            _quant(75.0), m)
        got = _frames(out, sizes, offs)
        assert modes == verdicts
        for k, im in enumerate(imgs):
            assert got[k] == sj.SjpegEncode(im, 75.0, m, sj.YUV_AUTO), (m, k, im.shape, modes[k])


@pytest.mark.parametrize("m", [0, 1, 3, 4, 6])
def test_auto_equals_oracle(engine, oracle, risk_table, m):
    imgs = _mixed()
    qs = [30.0, 75.0, 95.0, 50.0, 10.0, 90.0, 75.0, 60.0, 80.0, 20.0, 40.0, 70.0, 85.0, 55.0, 65.0, 45.0]
    verdicts = [oracle.riskiness(im, risk_table)[0] for im in imgs]
    mq = np.full((2, 64), 3, np.uint8)
    out, sizes, offs, modes = engine.encode_ragged_auto(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_AUTO,
                                                        [_quant(q) for q in qs], m, min_quant=mq, q_bias=0x60,
                                                        dmax_luma=8, dmax_chroma=3)
    got = _frames(out, sizes, offs)
    assert modes == verdicts
    for k, im in enumerate(imgs):
        want = oracle.encode_full(im, _quant(qs[k]), mq, 0x60, 8, 3, yuv_mode=verdicts[k], method=m)
        assert got[k] == want, (m, k, im.shape, verdicts[k])
    out, sizes, offs, _ = engine.encode_ragged_auto(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_AUTO, _quant(75.0), m)
    got = _frames(out, sizes, offs)
    for k, im in enumerate(imgs):
        assert got[k] == oracle.encode_method(im, 75.0, verdicts[k], m), (m, k)


def test_baseline_config1_inside_a_batch(risk_table):
    imgs = _mixed()
    got = sj.compress_images([torch.from_numpy(im).cuda() for im in imgs])
    assert len(got[0]) == 2571 and hashlib.md5(got[0]).hexdigest() == "acc8ce8111f5ff4b32b3faa15ad5d994"
    for k, im in enumerate(imgs):
        assert got[k] == sj.SjpegCompress(im, 75.0), k


def test_encode_images_auto_qualities(risk_table):
    imgs = _mixed()[:8]
    qs = [20.0, 90.0, 75.0, 50.0, 35.0, 80.0, 60.0, 95.0]
    got = sj.encode_images([torch.from_numpy(im).cuda() for im in imgs], qs, sj.YUV_AUTO, method=0)
    for k, im in enumerate(imgs):
        assert got[k] == sj.SjpegEncode(im, qs[k], 0, sj.YUV_AUTO), k


# ---- 5. explicit SHARP, and the fixed modes passed through

@pytest.mark.parametrize("m", [0, 4, 6])
def test_explicit_sharp(engine, risk_table, m):
    imgs = _mixed()
    out, sizes, offs, modes = engine.encode_ragged_auto(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_SHARP, _quant(70.0), m)
    got = _frames(out, sizes, offs)
    assert modes == [sj.YUV_SHARP] * len(imgs)
    for k, im in enumerate(imgs):
        assert got[k] == sj.SjpegEncode(im, 70.0, m, sj.YUV_SHARP), (m, k)


@pytest.mark.parametrize("mode", [sj.YUV_420, sj.YUV_444, sj.YUV_400])
def test_fixed_modes_equal_ragged_batch(engine, mode):
    imgs = _mixed()
    dims = _dims(imgs)
    caps = [sj.frame_bound(w, h, sj.YUV_444, 2048) for (w, h) in dims]
    out, sizes, offs, modes = engine.encode_ragged_auto(sj.SRC_RGB, _dev(imgs), dims, mode, _quant(75.0), 4,
                                                        capacities=caps)
    assert modes == [mode] * len(imgs)
    want = engine.encode_ragged_batch(sj.SRC_RGB, _dev(imgs), dims, mode, _quant(75.0), 4, capacities=caps)
    assert _frames(out, sizes, offs) == _frames(*want)


# ---- 6. capacity and canary

def test_capacity_and_canary(engine, risk_table):
    imgs = _mixed()
    dims = _dims(imgs)
    caps = [sj.frame_bound(w, h, sj.YUV_444, 2048) for (w, h) in dims]
    caps[0] = 600                                    # test128 is 2571 bytes: does not fit
    offs, at = [], 0
    for c in caps:
        offs.append(at + 16)
        at += 16 + ((c + 15) & ~15) + 16
    out = torch.full((at + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    out, sizes, offs, modes = engine.encode_ragged_auto(sj.SRC_RGB, _dev(imgs), dims, sj.YUV_AUTO, _quant(75.0), 4,
                                                        capacities=caps, out=out, offsets=offs)
    got = _frames(out, sizes, offs)
    sz = sizes.cpu().numpy()
    assert sz[0] == 0
    host = out.cpu().numpy()
    assert (host[offs[0]:offs[0] + caps[0]] == 0xA5).all()
    inside = np.zeros(len(host), bool)
    for k in range(len(imgs)):
        inside[offs[k]:offs[k] + caps[k]] = True
    assert (host[~inside] == 0xA5).all()
    for k in range(1, len(imgs)):
        assert got[k] == sj.SjpegEncode(imgs[k], 75.0, 4, sj.YUV_AUTO), k


# ---- 7. split launches

def test_split_launches(monkeypatch, risk_table):
    imgs = _mixed()
    whole = sj.Engine(0)
    want = _frames(*whole.encode_ragged_auto(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_AUTO, _quant(75.0), 4)[:3])
    monkeypatch.setenv("SJPEG_HIP_SCRATCH_LIMIT_BYTES", "1")
    split = sj.Engine(0)
    got = _frames(*split.encode_ragged_auto(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_AUTO, _quant(75.0), 4)[:3])
    assert got == want
    got = _frames(*split.encode_ragged_auto(sj.SRC_RGB, _dev(imgs), _dims(imgs), sj.YUV_SHARP, _quant(75.0), 1)[:3])
    assert got == [sj.SjpegEncode(im, 75.0, 1, sj.YUV_SHARP) for im in imgs]


# ---- 8. concurrency and errors

def test_two_engines_two_threads_and_back_to_back(risk_table):
    imgs = _mixed()
    want = [sj.SjpegEncode(im, 75.0, 4, sj.YUV_AUTO) for im in imgs]
    results, errors = {}, []

    def work(i):
        try:
            eng = sj.Engine(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                dev = _dev(imgs)
                runs = [eng.encode_ragged_auto(sj.SRC_RGB, dev, _dims(imgs), sj.YUV_AUTO, _quant(75.0), 4)[:3]
                        for _ in range(3)]
                s.synchronize()
                results[i] = [_frames(*r) for r in runs]
        except Exception as e:                       # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i in range(2):
        for r in results[i]:
            assert r == want


def test_bad_arguments(engine, risk_table):
    imgs = _mixed()[:3]
    dev, dims = _dev(imgs), _dims(imgs)

    def refused(match, **kw):
        args = dict(fmt=sj.SRC_RGB, planes_per_frame=dev, dims=dims, yuv_mode=sj.YUV_AUTO, quant=_quant(75.0), method=4)
        args.update(kw)
        with pytest.raises(sj.SjpegError, match=match):
            engine.encode_ragged_auto(**args)

    refused("yuv_mode outside 0..4", yuv_mode=5)
    refused("yuv_mode outside 0..4", yuv_mode=-1)
    refused("methods 0..6", method=7)
    refused("methods 0..6", method=8)
    refused("methods 0..6", method=8, yuv_mode=sj.YUV_SHARP)
    refused("qdelta_max", dmax_luma=13)
    gray = [[torch.zeros((im.shape[0], im.shape[1]), dtype=torch.uint8, device="cuda")] for im in imgs]
    refused("RGB, BGRA or RGBA", fmt=sj.SRC_GRAY, planes_per_frame=gray)
    refused("RGB, BGRA or RGBA", fmt=sj.SRC_GRAY, planes_per_frame=gray, yuv_mode=sj.YUV_SHARP)
    yuv = [[torch.zeros((h, w), dtype=torch.uint8, device="cuda")] * 3 for (w, h) in dims]
    refused("RGB, BGRA or RGBA", fmt=sj.SRC_YUV444, planes_per_frame=yuv)
    refused("frame 1: bad dimensions", dims=[dims[0], (0, 5), dims[2]])
    short = [dev[0], dev[1], [(dev[2][0].data_ptr(), 3 * dims[2][0] - 1)]]
    refused("frame 2: .row_stride", planes_per_frame=short)
    nullp = [dev[0], [(0, 3 * dims[1][0])], dev[2]]
    refused("frame 1: null plane", planes_per_frame=nullp)
    refused("yuv_mode does not match", fmt=sj.SRC_GRAY, planes_per_frame=gray, yuv_mode=sj.YUV_444)
    with pytest.raises(sj.SjpegError, match="RGB, BGRA or RGBA"):
        engine.riskiness_ragged(sj.SRC_GRAY, gray, dims)
    with pytest.raises(sj.SjpegError, match="sharp conversion takes RGB"):
        engine.sharp_yuv_ragged(sj.SRC_GRAY, gray, dims)
