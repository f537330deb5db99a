"""Planar RGB (SJPEG_HIP_SRC_RGB_PLANAR, channel-first pictures) through every entry point: uniform batches of
[N, 3, H, W] tensors in the three samplings, padded and bottom-up rows, ragged batches through encode_images /
compress_images with layout="chw" and encode_images_full_chw (methods, trellis, targets, packed, SJPEG_YUV_AUTO), the analysis
passes against the [H, W, 3] calls, and the refusals.  The expected bytes are the oracle's for the interleaved picture."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import orc, synth

pytestmark = pytest.mark.gpu

PLANAR = sj.SRC_RGB_PLANAR
RAGGED = [(1, 1), (17, 13), (64, 48), (215, 279), (700, 24)]


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


def _gradient(w, h):
    x = np.arange(w)[None, :] * 200 // w
    y = np.arange(h)[:, None] * 200 // h
    return np.stack([np.broadcast_to(x + 20, (h, w)), np.broadcast_to(y + 30, (h, w)), np.full((h, w), 90)],
                    2).astype(np.uint8)


def _content(k, w, h):
    """The five kinds of tests/test_ragged_auto.py::_content: structure, noise, gray noise, saturated noise, a gradient."""
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


@pytest.fixture(scope="module")
def ragged():
    """The five pictures of the ragged tests (host [H, W, 3]); never written to."""
    return [synth.g_struct(w, h, 4200 + k) if k % 2 == 0 else synth.g_noise(w, h, 4200 + k) for k, (w, h) in enumerate(RAGGED)]


def _chw(im, pad=0, fill=0):
    """A CUDA [3, H, W] tensor of a host [H, W, 3] picture; pad: its rows lie pad bytes apart more than W (a crop of a
    [3, H, W + pad] tensor whose other columns hold `fill`)."""
    h, w, _ = im.shape
    buf = np.full((3, h, w + pad), fill, np.uint8)
    buf[:, :, :w] = im.transpose(2, 0, 1)
    return torch.from_numpy(buf).cuda()[:, :, :w]


def _quant(q=75.0):
    m = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(float(q), m.ctypes.data)
    return m


def _streams(out, sizes):
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    return [host[k, :int(sz[k])].tobytes() for k in range(len(sz))]


def _planes(imgs, pad=0):
    """planes_per_frame of the Engine's ragged calls: the three [H, W] planes of each picture's [3, H, W] tensor."""
    out = []
    for im in imgs:
        t = _chw(im, pad)
        out.append([t[0], t[1], t[2]])
    return out


def _packed(imgs, pad=16):
    out = []
    for im in imgs:
        h, w, _ = im.shape
        buf = np.zeros((h, 3 * w + pad), np.uint8)
        buf[:, :3 * w] = im.reshape(h, 3 * w)
        out.append([torch.from_numpy(buf).cuda()[:, :3 * w]])
    return out


def _dims(imgs):
    return [(im.shape[1], im.shape[0]) for im in imgs]


# ---- uniform batches

@pytest.mark.parametrize("mode", [sj.YUV_420, sj.YUV_444, sj.YUV_400])
@pytest.mark.parametrize("w,h", [(64, 48), (17, 13), (1, 1), (700, 24), (330, 50)])
def test_uniform_batch(engine, oracle, w, h, mode):
    # 64x48: interior segments only; 17x13: clipped in x and y, G and B planes at odd addresses; 700x24: more than 42
    # MCUs wide (a segment wraps to the next MCU row); 330x50: several segments, clipped
    n = 3
    imgs = [synth.g_struct(w, h, 900 + k) if k != 1 else synth.g_noise(w, h, 900 + k) for k in range(n)]
    x = torch.from_numpy(np.ascontiguousarray(np.stack(imgs).transpose(0, 3, 1, 2))).cuda()       # [N, 3, H, W]
    src, nf = sj.make_source(PLANAR, (x[:, 0], x[:, 1], x[:, 2]))
    assert nf == n
    tables, qm = sj.make_tables(quality=75.0)
    out, sizes = engine.encode_source(src, n, w, h, tables, sj.make_header(w, h, mode, qm), mode)
    got = _streams(out, sizes)
    for k in range(n):
        assert got[k] == oracle.encode(imgs[k], 75.0, mode), (k, w, h, mode)


def test_uniform_batch_method_4(engine, oracle):
    w, h, n = 330, 50, 3
    imgs = [synth.g_struct(w, h, 950 + k) for k in range(n)]
    x = torch.from_numpy(np.ascontiguousarray(np.stack(imgs).transpose(0, 3, 1, 2))).cuda()
    src, _ = sj.make_source(PLANAR, (x[:, 0], x[:, 1], x[:, 2]))
    out, sizes = engine.encode_batch(src, n, w, h, sj.YUV_420, _quant(80.0), method=4)
    engine.wait()
    got = _streams(out, sizes)
    for k in range(n):
        assert got[k] == oracle.encode_method(imgs[k], 80.0, sj.YUV_420, 4), k


# ---- padding and strides

@pytest.mark.parametrize("mode", [sj.YUV_420, sj.YUV_444])
def test_padded_rows_and_garbage_in_the_padding(engine, oracle, mode):
    im = synth.g_struct(215, 99, 31)
    want = oracle.encode(im, 75.0, mode)
    a = sj.encode_images([_chw(im, 16, 0)], 75.0, mode, engine=engine, layout="chw")
    b = sj.encode_images([_chw(im, 16, 0xa5)], 75.0, mode, engine=engine, layout="chw")
    assert a[0] == want and b[0] == want
    # a crop of a larger tensor: rows and planes of the parent's pitch, the first pixel anywhere
    big = np.random.RandomState(5).randint(0, 256, (3, 120, 260)).astype(np.uint8)
    big[:, 7:7 + 99, 21:21 + 215] = im.transpose(2, 0, 1)
    crop = torch.from_numpy(big).cuda()[:, 7:7 + 99, 21:21 + 215]
    assert sj.encode_images([crop], 75.0, mode, engine=engine, layout="chw")[0] == want


@pytest.mark.parametrize("mode", [sj.YUV_420, sj.YUV_400])
def test_bottom_up_rows(engine, oracle, mode):
    imgs = [synth.g_struct(101, 67, 77), synth.g_noise(64, 48, 78)]
    keep, planes = [], []
    for im in imgs:
        h = im.shape[0]
        t = _chw(im[::-1], 16)                      # stored bottom-up
        keep.append(t)
        planes.append([(t[c].data_ptr() + (h - 1) * t.stride(1), -t.stride(1)) for c in range(3)])
    tables, qm = sj.make_tables(quality=75.0)
    headers = [sj.make_header(im.shape[1], im.shape[0], mode, qm) for im in imgs]
    out, sizes, offs = engine.encode_ragged(PLANAR, planes, _dims(imgs), mode, tables, headers)
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    for k, im in enumerate(imgs):
        assert host[offs[k]:offs[k] + int(sz[k])].tobytes() == oracle.encode(im, 75.0, mode), k


# ---- ragged batches through the torch-facing calls

@pytest.mark.parametrize("method", [0, 4, 6])
def test_ragged_methods(engine, oracle, ragged, method):
    dev = [_chw(im, 16 if k % 2 else 0) for k, im in enumerate(ragged)]
    for mode in (sj.YUV_420, sj.YUV_444, sj.YUV_400):
        got = sj.encode_images(dev, 75.0, mode, engine=engine, method=method, layout="chw")
        for k, im in enumerate(ragged):
            assert got[k] == oracle.encode_method(im, 75.0, mode, method), (mode, method, k, im.shape)


@pytest.mark.parametrize("method", [4, 6])
def test_ragged_trellis(engine, oracle, ragged, method):
    dev = [_chw(im) for im in ragged]
    got = sj.encode_images(dev, 75.0, sj.YUV_420, engine=engine, method=method, use_trellis=True, layout="chw")
    for k, im in enumerate(ragged):
        assert got[k] == oracle.encode_method(im, 75.0, sj.YUV_420, {4: 7, 6: 8}[method]), (method, k, im.shape)


def _rgb2d(im):
    return [im.reshape(im.shape[0], -1)]


def test_ragged_target_size_and_psnr(engine, oracle, ragged):
    dev = [_chw(im) for im in ragged]
    plain = [len(oracle.encode_method(im, 75.0, sj.YUV_420, 4)) for im in ragged]
    sizes = [max(int(0.7 * n), 200) for n in plain]
    got = sj.encode_images(dev, 75.0, sj.YUV_420, engine=engine, method=4, target_size=sizes, passes=5, layout="chw")
    for k, im in enumerate(ragged):
        want = oracle.encode_search(orc.SRC_RGB, _rgb2d(im), im.shape[1], im.shape[0], _quant(75.0), yuv_mode=sj.YUV_420,
                                    target_mode=1, target_value=float(sizes[k]), passes=5)
        assert got[k] == want, ("size", k, im.shape)
    got = sj.encode_images(dev, 75.0, sj.YUV_444, engine=engine, method=4, target_psnr=38.0, passes=4, layout="chw")
    for k, im in enumerate(ragged):
        want = oracle.encode_search(orc.SRC_RGB, _rgb2d(im), im.shape[1], im.shape[0], _quant(75.0), yuv_mode=sj.YUV_444,
                                    target_mode=2, target_value=38.0, passes=4)
        assert got[k] == want, ("psnr", k, im.shape)


def test_ragged_packed(engine, oracle, ragged):
    dev = [_chw(im, 16) for im in ragged]
    got = sj.encode_images(dev, [60.0, 75.0, 90.0, 75.0, 40.0], sj.YUV_420, engine=engine, packed=True, layout="chw")
    for k, (im, q) in enumerate(zip(ragged, [60.0, 75.0, 90.0, 75.0, 40.0])):
        assert got[k] == oracle.encode(im, q, sj.YUV_420), k
    got = sj.encode_images(dev, 75.0, sj.YUV_444, engine=engine, method=4, packed=True, layout="chw")
    for k, im in enumerate(ragged):
        assert got[k] == oracle.encode_method(im, 75.0, sj.YUV_444, 4), k


def _auto_want(oracle, im, verdict, method=4, sp=None):
    """What sjpeg::Encode() makes of the picture with SJPEG_YUV_AUTO: the oracle, the sharp frames as planar 4:2:0."""
    if verdict == sj.YUV_SHARP:
        fmt, planes, mode = orc.SRC_YUV420, list(oracle.sharp_yuv(im)), sj.YUV_420
    else:
        fmt, planes, mode = orc.SRC_RGB, _rgb2d(im), verdict
    if sp is None:
        return oracle.encode_src(fmt, planes, im.shape[1], im.shape[0], _quant(75.0), yuv_mode=mode, method=method)
    return oracle.encode_search(fmt, planes, im.shape[1], im.shape[0], _quant(75.0), yuv_mode=mode, target_mode=1,
                                target_value=float(sp), passes=4)


def test_compress_images_and_the_full_call(engine, oracle, risk_table):
    # (content of five kinds at the ragged sizes and two more, so that every verdict of SJPEG_YUV_AUTO occurs)
    dims = RAGGED + [(97, 61), (128, 90), (160, 120), (33, 200), (120, 80)]
    imgs = [_content(k, w, h) for k, (w, h) in enumerate(dims)]
    verdicts = [oracle.riskiness(im, risk_table)[0] for im in imgs]
    assert set(verdicts) == {sj.YUV_420, sj.YUV_SHARP, sj.YUV_444, sj.YUV_400}, verdicts
    dev = [_chw(im, 16 if k % 2 else 0) for k, im in enumerate(imgs)]
    assert [m for m, _ in sj.riskiness_images(dev, engine=engine, layout="chw")] == verdicts
    out, sizes, offs, modes = engine.encode_ragged_auto(PLANAR, _planes(imgs), _dims(imgs), sj.YUV_AUTO, _quant(75.0), 4)
    engine.wait()
    torch.cuda.synchronize()
    assert list(modes) == verdicts
    got = sj.compress_images(dev, 75.0, engine=engine, layout="chw")
    for k, im in enumerate(imgs):
        assert got[k] == _auto_want(oracle, im, verdicts[k]), ("compress", k, im.shape, verdicts[k])
    plain = [len(g) for g in got]
    targets = [max(int(0.7 * n), 200) for n in plain]
    got = sj.encode_images_full_chw(dev, 75.0, sj.YUV_AUTO, method=4, target_size=targets, passes=4, engine=engine)
    for k, im in enumerate(imgs):
        assert got[k] == _auto_want(oracle, im, verdicts[k], sp=targets[k]), ("full", k, im.shape, verdicts[k])


# ---- the analysis passes on the ragged set: the [H, W, 3] call's arrays, exactly

def test_analysis_passes_equal_the_interleaved_calls(engine, oracle, ragged, risk_table):
    dims, pl, hw = _dims(ragged), _planes(ragged, 16), _packed(ragged)
    tables, qm = sj.make_tables(quality=75.0)
    for mode in (sj.YUV_420, sj.YUV_444, sj.YUV_400):
        a = engine.scan_histogram_ragged(PLANAR, pl, dims, mode).cpu().numpy()
        b = engine.scan_histogram_ragged(sj.SRC_RGB, hw, dims, mode).cpu().numpy()
        assert (a == b).all(), ("histogram", mode)
        a = engine.scan_symbol_stats_ragged(PLANAR, pl, dims, mode, tables).cpu().numpy()
        b = engine.scan_symbol_stats_ragged(sj.SRC_RGB, hw, dims, mode, tables).cpu().numpy()
        assert (a == b).all(), ("symbol statistics", mode)
        a = engine.scan_quant_error_ragged(PLANAR, pl, dims, mode, tables).cpu().numpy()
        b = engine.scan_quant_error_ragged(sj.SRC_RGB, hw, dims, mode, tables).cpu().numpy()
        assert (a == b).all(), ("quantization error", mode)
        a = engine.scan_counted_bits_ragged(PLANAR, pl, dims, mode, tables).cpu().numpy()
        b = engine.scan_counted_bits_ragged(sj.SRC_RGB, hw, dims, mode, tables).cpu().numpy()
        assert (a == b).all(), ("counted bits", mode)
    hist = engine.scan_histogram_ragged(PLANAR, pl, dims, sj.YUV_420).cpu().numpy().astype(np.uint32)
    for k, im in enumerate(ragged):       # ... and the oracle's, where it has the pass
        assert (hist[k] == oracle.histogram(im, sj.YUV_420)).all(), k
    a = engine.riskiness_ragged(PLANAR, pl, dims).cpu().numpy()
    b = engine.riskiness_ragged(sj.SRC_RGB, hw, dims).cpu().numpy()
    assert (a == b).all()
    sa = engine.sharp_yuv_ragged(PLANAR, pl, dims)
    torch.cuda.synchronize()
    sa = [[p.cpu().numpy() for p in fr] for fr in sa]
    sb = engine.sharp_yuv_ragged(sj.SRC_RGB, hw, dims)
    torch.cuda.synchronize()
    for k, im in enumerate(ragged):
        want = oracle.sharp_yuv(im)
        for i in range(3):
            assert (sa[k][i] == sb[k][i].cpu().numpy()).all(), (k, i)
            assert (sa[k][i] == want[i]).all(), (k, i)


def test_uniform_riskiness_and_sharp(engine, oracle, risk_table):
    w, h, n = 97, 61, 2
    imgs = [_content(k, w, h) for k in (0, 3)]
    x = torch.from_numpy(np.ascontiguousarray(np.stack(imgs).transpose(0, 3, 1, 2))).cuda()
    src, _ = sj.make_source(PLANAR, (x[:, 0], x[:, 1], x[:, 2]))
    tab = torch.frombuffer(bytearray(risk_table), dtype=torch.uint8).cuda()
    sums = torch.zeros((n, 3), dtype=torch.int64, device="cuda")
    proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
    fn = C.cast(sj.lib().sjpeg_hip_riskiness_sums, proto)
    assert fn(C.addressof(src), w, h, n, tab.data_ptr(), sums.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    sums = sums.cpu().numpy()
    for k, im in enumerate(imgs):
        assert sj.riskiness_verdict(sums[k], w, h) == oracle.riskiness(im, risk_table), k
    cw, ch = (w + 1) // 2, (h + 1) // 2
    py = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    pu = torch.empty((n, ch, cw), dtype=torch.uint8, device="cuda")
    pv = torch.empty((n, ch, cw), dtype=torch.uint8, device="cuda")
    L = sj.lib()
    L.sjpeg_hip_sharp_workspace.restype = C.c_size_t
    L.sjpeg_hip_sharp_workspace.argtypes = [C.c_int, C.c_int, C.c_int]
    wsz = L.sjpeg_hip_sharp_workspace(w, h, n)
    work = torch.empty(max(wsz, 16), dtype=torch.uint8, device="cuda")
    proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                        C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p)
    fn = C.cast(L.sjpeg_hip_sharp_yuv, proto)
    assert fn(C.addressof(src), w, h, n, py.data_ptr(), pu.data_ptr(), pv.data_ptr(), h * w, ch * cw, work.data_ptr(),
              wsz, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for k, im in enumerate(imgs):
        oy, ou, ov = oracle.sharp_yuv(im)
        assert (py[k].cpu().numpy() == oy).all() and (pu[k].cpu().numpy() == ou).all() and (pv[k].cpu().numpy() == ov).all(), k


# ---- refusals

def _refused(fn, *words):
    with pytest.raises(sj.SjpegError) as e:
        fn()
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals(engine):
    w, h = 32, 16
    a = torch.zeros((2, 3, h, w + 8), dtype=torch.uint8, device="cuda")
    tables, qm = sj.make_tables(quality=75.0)
    hdr = sj.make_header(w, h, sj.YUV_420, qm)
    x = a[0, :, :, :w]
    good = [x[0], x[1], x[2]]
    # ragged: the frame and the stride are named
    other = torch.zeros((h, w + 24), dtype=torch.uint8, device="cuda")[:, :w]
    _refused(lambda: engine.encode_ragged(PLANAR, [good, [x[0], other, x[2]]], [(w, h)] * 2, sj.YUV_420, tables, [hdr] * 2),
             "frame 1", "row_stride[1]", "row_stride[0]")
    _refused(lambda: engine.encode_ragged(PLANAR, [good, [x[0], x[1], other]], [(w, h)] * 2, sj.YUV_420, tables, [hdr] * 2),
             "frame 1", "row_stride[2]")
    _refused(lambda: engine.encode_ragged(PLANAR, [good, [(x[0].data_ptr(), x.stride(1)), (0, x.stride(1)),
                                                          (x[2].data_ptr(), x.stride(1))]],
                                          [(w, h)] * 2, sj.YUV_420, tables, [hdr] * 2), "frame 1", "null plane")
    narrow = [(x[c].data_ptr(), w - 1) for c in range(3)]
    _refused(lambda: engine.encode_ragged(PLANAR, [narrow], [(w, h)], sj.YUV_420, tables, [hdr]), "frame 0", "row_stride")
    _refused(lambda: engine.riskiness_ragged(PLANAR, [good, [x[0], other, x[2]]], [(w, h)] * 2), "frame 1", "row_stride[1]")
    _refused(lambda: engine.sharp_yuv_ragged(PLANAR, [good, [x[0], other, x[2]]], [(w, h)] * 2), "frame 1", "row_stride[1]")
    # uniform: unequal row or frame strides
    src, _ = sj.make_source(PLANAR, (a[:, 0, :, :w], a[:, 1, :, :w], a[:, 2, :, :w]))
    src.frame_stride[2] = src.frame_stride[0] + 16
    _refused(lambda: engine.encode_source(src, 2, w, h, tables, hdr, sj.YUV_420), "frame_stride[2]")
    src, _ = sj.make_source(PLANAR, (a[:, 0, :, :w], a[:, 1, :, :w], a[:, 2, :, :w]))
    src.row_stride[1] = src.row_stride[0] + 1
    _refused(lambda: engine.encode_source(src, 2, w, h, tables, hdr, sj.YUV_420), "row_stride[1]")
    # the layout keyword
    hwc = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    _refused(lambda: sj.encode_images([x, hwc], layout="chw", engine=engine), "image 1", "[3, H, W]")
    _refused(lambda: sj.encode_images([x, a[0, :, :, ::2]], layout="chw", engine=engine), "image 1")
    _refused(lambda: sj.encode_images([x], layout="nchw", engine=engine), "nchw")
    _refused(lambda: sj.compress_images([x], layout="nchw", engine=engine), "nchw")
    _refused(lambda: sj.encode_images_full_chw([hwc], engine=engine), "image 0")
    _refused(lambda: sj.riskiness_images([hwc], layout="chw", engine=engine), "image 0")
