"""Pictures turned upright inside the ragged call on the GPU (sjpeg_hip_orient_ragged_src,
sjpeg_hip_encode_ragged_oriented_src, Oriented).  The contract is sjpeg_hip.h's: with R the resized picture of
sjpeg_hip_resize_ragged_src, the upright picture of orientation o is U(x, y) = R(sx, sy) by the table there, and the JPEG
is that of the uint8 picture U.  Every comparison is exact.  The expected pictures are _upright() below -- the table in
numpy -- of _area() of tests/test_resize.py; the expected JPEGs come from the existing entry points on those pictures."""
import os

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import synth
from test_reduce import FORMATS, XFORM3, _check_pictures, _on_device, _quant, _rgb_planes, _seen, _streams
from test_resize import _area

pytestmark = pytest.mark.gpu

# source -> size, the smallest that reach each hazard of the store: 1 x 1; rows that end in padding and widths that are
# no multiple of 4; ratio 1 with two 256 x 16 tiles across and two down, the upright picture 17 wide; 64 lanes a column
# and tiles 4 wide, three across meeting inside dwords, five rows of tiles; a support of 44; a row wider than one
# workgroup's span; and a segment staged in chunks.
SHAPES = [((1, 1), (1, 1)), ((3, 2), (3, 2)), ((2, 3), (1, 2)), ((5, 7), (5, 7)), ((7, 5), (3, 2)), ((257, 17), (257, 17)),
          ((576, 130), (9, 65)), ((300, 40), (7, 3)), ((1030, 9), (1029, 8)), ((6000, 2), (1, 1))]
ORIENTATIONS = list(range(1, 9))


def _upright(R, o):
    """sjpeg_hip.h's table on a picture [h, w] or [h, w, c], in numpy"""
    if o == 1:
        return R
    if o == 2:
        return R[:, ::-1]
    if o == 3:
        return R[::-1, ::-1]
    if o == 4:
        return R[::-1]
    if o == 5:
        return R.swapaxes(0, 1)
    if o == 6:
        return np.rot90(R, -1)
    if o == 7:
        return R[::-1, ::-1].swapaxes(0, 1)
    assert o == 8
    return np.rot90(R, 1)


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.fixture(scope="module")
def risk_table():
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        tab = f.read()
    sj.set_riskiness_table(tab)
    return tab


@pytest.fixture(scope="module")
def sources():
    """(u8 [H, W, 3], (w, h)): noise and all 255 for every shape.  Never written to."""
    out = []
    for k, ((w, h), size) in enumerate(SHAPES):
        out.append((synth.g_noise(w, h, 9700 + k), size))
        out.append((np.full((h, w, 3), 255, np.uint8), size))
    return out


def test_the_expectation_itself():
    """_upright() against the table, sample by sample, on a 3 x 2 picture whose samples are all different"""
    R = np.arange(6, dtype=np.uint8).reshape(2, 3)
    w, h = 3, 2
    table = {1: lambda x, y: (x, y), 2: lambda x, y: (w - 1 - x, y), 3: lambda x, y: (w - 1 - x, h - 1 - y),
             4: lambda x, y: (x, h - 1 - y), 5: lambda x, y: (y, x), 6: lambda x, y: (y, h - 1 - x),
             7: lambda x, y: (w - 1 - y, h - 1 - x), 8: lambda x, y: (w - 1 - y, x)}
    for o in ORIENTATIONS:
        U = _upright(R, o)
        assert U.shape == ((3, 2) if o >= 5 else (2, 3))
        for y in range(U.shape[0]):
            for x in range(U.shape[1]):
                sx, sy = table[o](x, y)
                assert U[y, x] == R[sy, sx], (o, x, y)


# ---- 1. the kernel alone: ONE ragged call per format over every shape, content and orientation

@pytest.mark.parametrize("name", list(FORMATS))
def test_orient_ragged_against_numpy(engine, sources, name):
    fmt, layout, dtype = FORMATS[name]
    if dtype is not None:
        engine.set_pixel_transform(*XFORM3[dtype])
    planes, keep, wants, dims, sizes, orients = [], [], [], [], [], []
    for k, (u8, size) in enumerate(sources):
        p, dev, host = _on_device(u8, layout, dtype, seed=k, off=k % 3, pad=(k // 3) % 2)
        seen = _seen(host, layout, dtype)
        assert np.array_equal(seen, u8[..., 1] if layout == "gray" else u8)
        keep.append(dev)
        R = _area(seen, *size)
        for o in ORIENTATIONS:                       # (the same source, eight frames)
            planes.append(p); dims.append((u8.shape[1], u8.shape[0])); sizes.append(size); orients.append(o)
            wants.append(_upright(R, o))
    rfmt, pics, buf = engine.orient_ragged(fmt, planes, dims, sizes, orients)
    assert rfmt == (sj.SRC_GRAY if layout == "gray" else sj.SRC_RGB)
    for p, size, o in zip(pics, sizes, orients):
        assert (p.shape[1], p.shape[0]) == sj.oriented_size(*size, o)
        assert p.data_ptr() % 16 == 0 and p.stride(0) == (p.shape[1] * (1 if layout == "gray" else 3) + 3) // 4 * 4
    _check_pictures(pics, wants)
    engine.set_pixel_transform(255.0, 0.0)


def test_negative_row_stride_and_own_sizes(engine):
    """stored bottom-up, sizes None: the pure turn of every picture at its own size"""
    dims = [(17, 9), (63, 65), (300, 40), (5, 7)]
    ims = [synth.g_noise(w, h, 9750 + k) for k, (w, h) in enumerate(dims)]
    devs = [torch.from_numpy(np.ascontiguousarray(im[::-1])).cuda() for im in ims]
    planes = [[(d.data_ptr() + (d.shape[0] - 1) * d.stride(0), -d.stride(0))] for d in devs]
    for orients in ([6, 8, 3, 5], [7, 2, 4, 6]):
        _, pics, _ = engine.orient_ragged(sj.SRC_RGB, planes, dims, None, orients)
        _check_pictures(pics, [_upright(im, o) for im, o in zip(ims, orients)])


# ---- 2. guards around the caller's buffer

@pytest.mark.parametrize("fmt,layout", [(sj.SRC_RGB, "rgb"), (sj.SRC_GRAY, "gray")])
def test_guard_bytes_around_the_oriented_buffer(engine, sources, fmt, layout):
    made, planes, dims, sizes, orients, wants = [], [], [], [], [], []
    for k, (u8, size) in enumerate(sources[::2]):
        m = _on_device(u8, layout, None)
        made.append(m)
        R = _area(_seen(m[2], layout, None), *size)
        for o in ORIENTATIONS:
            planes.append(m[0]); dims.append((u8.shape[1], u8.shape[0])); sizes.append(size); orients.append(o)
            wants.append(_upright(R, o))
    frames, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
    arr = np.ascontiguousarray(np.asarray(sizes, np.int32))
    oarr = np.ascontiguousarray(np.asarray(orients, np.uint8))
    need = sj.lib().sjpeg_hip_orient_ragged_bytes(fmt, len(dims), frames, arr.ctypes.data, oarr.ctypes.data)
    assert need > 0 and need % 16 == 0
    guard = 64
    whole = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    assert (whole.data_ptr() + guard) % 16 == 0
    _, pics, _ = engine.orient_ragged(fmt, planes, dims, sizes, orients, out=whole[guard:guard + need])
    _check_pictures(pics, wants)
    host = whole.cpu().numpy()
    assert (host[:guard] == 0xA5).all() and (host[guard + need:] == 0xA5).all()
    # one byte short is refused before anything runs
    with pytest.raises(sj.SjpegError, match="bytes"):
        engine.orient_ragged(fmt, planes, dims, sizes, orients, out=whole[guard:guard + need - 16][:need - 1])


# ---- 3. it commutes: resize then turn == turn (in numpy, on the source) then the EXISTING resize at the swapped size

@pytest.mark.parametrize("dim,size", [((63, 65), (5, 64)), ((130, 70), (129, 1))])
def test_turning_commutes_with_the_resize(engine, dim, size):
    src = synth.g_noise(dim[0], dim[1], 9800 + dim[0])
    dev = torch.from_numpy(src).cuda()
    got = sj.orient_images([dev] * 8, ORIENTATIONS, size, engine=engine)
    turned = [torch.from_numpy(np.ascontiguousarray(_upright(src, o))).cuda() for o in ORIENTATIONS]
    want = sj.resize_images(turned, [sj.oriented_size(*size, o) for o in ORIENTATIONS], engine=engine)
    _check_pictures(got, [w.cpu().numpy() for w in want])


# ---- 4. encodes: each against the existing entry on the upright uint8 pictures, uploaded

ENC_DIMS = [(17, 9), (31, 33), (63, 65), (130, 70), (8, 8), (40, 21), (33, 31), (64, 48)]
ENC_SIZES = [(16, 9), (10, 33), (5, 64), (40, 21), (8, 8), (40, 21), (32, 9), (17, 48)]


@pytest.fixture(scope="module")
def batch():
    """(device pictures [H, W, 3], sizes, orientations -- all eight --, the upright pictures on the device and the host)"""
    ims = [synth.g_struct(w, h, 9900 + k) if k % 2 else synth.g_noise(w, h, 9900 + k) for k, (w, h) in enumerate(ENC_DIMS)]
    orients = [6, 3, 8, 1, 5, 2, 7, 4]
    up = [np.ascontiguousarray(_upright(_area(im, *s), o)) for im, s, o in zip(ims, ENC_SIZES, orients)]
    return [torch.from_numpy(im).cuda() for im in ims], ENC_SIZES, orients, [torch.from_numpy(x).cuda() for x in up], up


@pytest.mark.parametrize("method", [0, 4])
@pytest.mark.parametrize("mode", [sj.YUV_420, sj.YUV_444])
def test_engine_entries_against_the_full_call(engine, batch, method, mode):
    devs, sizes, orients, up_dev, up = batch
    planes, dims = _rgb_planes(devs)
    uplanes, udims = _rgb_planes(up_dev)
    out, szs, offs, modes, q, v = engine.encode_ragged_oriented(sj.SRC_RGB, planes, dims, sizes, orients, mode, _quant(), method)
    out2, szs2, offs2, modes2, q2, v2 = engine.encode_ragged_full(sj.SRC_RGB, uplanes, udims, mode, _quant(), method)
    want = _streams(out2, szs2, offs2)
    assert _streams(out, szs, offs) == want
    assert modes == modes2 == [mode] * len(devs) and q == q2 and v == v2
    assert offs == offs2                             # (the default capacities are the bounds of the upright sizes)
    out, szs, offs, modes, q, v = engine.encode_ragged_oriented_packed(sj.SRC_RGB, planes, dims, sizes, orients, mode, _quant(), method)
    out2, szs2, offs2, modes2, q2, v2 = engine.encode_ragged_full_packed(sj.SRC_RGB, uplanes, udims, mode, _quant(), method)
    torch.cuda.synchronize()
    assert _streams(out, szs, offs.cpu().numpy()) == want == _streams(out2, szs2, offs2.cpu().numpy())
    assert offs.cpu().tolist() == offs2.cpu().tolist() and szs.cpu().tolist() == szs2.cpu().tolist()
    assert modes == modes2 and q == q2 and v == v2
    assert sj.encode_images(sj.Oriented(devs, orients, sizes), 75.0, mode, engine=engine, method=method) == want


def test_compress_images_decides_on_the_upright_picture(engine, risk_table, batch):
    devs, sizes, orients, up_dev, up = batch
    assert sj.compress_images(sj.Oriented(devs, orients, sizes), 75.0, engine=engine) == sj.compress_images(up_dev, 75.0, engine=engine)
    planes, dims = _rgb_planes(devs)
    uplanes, udims = _rgb_planes(up_dev)
    out, szs, offs, modes, _, _ = engine.encode_ragged_oriented(sj.SRC_RGB, planes, dims, sizes, orients, sj.YUV_AUTO, _quant(), 4)
    out2, szs2, offs2, modes2, _, _ = engine.encode_ragged_full(sj.SRC_RGB, uplanes, udims, sj.YUV_AUTO, _quant(), 4)
    assert modes == modes2 and _streams(out, szs, offs) == _streams(out2, szs2, offs2)


def test_metadata_from_the_exif_tag(engine, batch):
    """Oriented.from_metadata: the orientations come out of the pictures' EXIF, the JPEGs carry it reset"""
    devs, sizes, orients, up_dev, up = batch
    def exif(o):
        return b"Exif\0\0II*\0\x08\0\0\0\x01\0\x12\x01\x03\0\x01\0\0\0" + bytes([o, 0, 0, 0]) + b"\0\0\0\0"
    metas = [sj.PictureMetadata(exif=exif(o), xmp=b"<x:xmpmeta>%d</x:xmpmeta>" % k) for k, o in enumerate(orients)]
    metas[3] = None                                  # (orientation 1 in the batch)
    made, reset = sj.Oriented.from_metadata(devs, metas)
    assert made.orientations == orients
    made = sj.Oriented(devs, made.orientations, sizes)
    want = sj.encode_images_full_meta(up_dev, reset, yuv_mode=sj.YUV_420, engine=engine)
    got = sj.encode_images_full_meta(made, reset, yuv_mode=sj.YUV_420, engine=engine)
    assert got == want
    assert all(exif(1) in g for k, g in enumerate(got) if k != 3) and all(exif(6) not in g for g in got)
    planes, dims = _rgb_planes(devs)
    out, szs, offs, _, _, _ = engine.encode_ragged_oriented(sj.SRC_RGB, planes, dims, sizes, orients, sj.YUV_420, _quant(), 4, metadata=reset)
    assert _streams(out, szs, offs) == want
    out, szs, offs, _, _, _ = engine.encode_ragged_oriented_packed(sj.SRC_RGB, planes, dims, sizes, orients, sj.YUV_420, _quant(), 4,
                                                                   metadata=reset)
    assert _streams(out, szs, offs.cpu().numpy()) == want


def test_target_size_search(engine, batch):
    devs, sizes, orients, up_dev, up = batch
    targets = [max(400, x.size // 6) for x in up]
    planes, dims = _rgb_planes(devs)
    uplanes, udims = _rgb_planes(up_dev)
    search = [dict(target_mode=sj.TARGET_SIZE, target_value=t) for t in targets]
    out, szs, offs, _, q, v = engine.encode_ragged_oriented(sj.SRC_RGB, planes, dims, sizes, orients, sj.YUV_420, _quant(), 4, search=search)
    out2, szs2, offs2, _, q2, v2 = engine.encode_ragged_full(sj.SRC_RGB, uplanes, udims, sj.YUV_420, _quant(), 4, search=search)
    want = _streams(out2, szs2, offs2)
    assert _streams(out, szs, offs) == want and q == q2 and v == v2
    assert sj.encode_images(sj.Oriented(devs, orients, sizes), 75.0, sj.YUV_420, engine=engine, method=4, target_size=targets) == want


# ---- 5. orientations that change nothing

def test_all_ones_is_the_resized_call(engine, batch):
    devs, sizes, orients, up_dev, up = batch
    planes, dims = _rgb_planes(devs)
    out2, szs2, offs2, _, _, _ = engine.encode_ragged_resized(sj.SRC_RGB, planes, dims, sizes, sj.YUV_420, _quant(), 4)
    want = _streams(out2, szs2, offs2)
    for o in (None, [1] * len(devs)):
        out, szs, offs, _, _, _ = engine.encode_ragged_oriented(sj.SRC_RGB, planes, dims, sizes, o, sj.YUV_420, _quant(), 4)
        assert _streams(out, szs, offs) == want
    assert sj.encode_images(sj.Oriented(devs, 1, sizes), 75.0, sj.YUV_420, engine=engine, method=4) == want
    # the kernel's own o = 1 frames in a mixed launch are the resize's pictures
    _, pics, _ = engine.orient_ragged(sj.SRC_RGB, planes, dims, sizes, [1, 6] * (len(devs) // 2))
    _, plain, _ = engine.resize_ragged(sj.SRC_RGB, planes, dims, sizes)
    _check_pictures(pics[::2], [p.cpu().numpy() for p in plain[::2]])
    # an NV12 batch at its own sizes passes with all 1, and is refused by name with a 6
    rs = np.random.RandomState(9950)
    nv, nvdims = [], [(34, 18), (17, 9)]
    for (w, h) in nvdims:
        nv.append([torch.from_numpy(rs.randint(0, 256, (h, w)).astype(np.uint8)).cuda(),
                   torch.from_numpy(rs.randint(0, 256, ((h + 1) // 2, 2 * ((w + 1) // 2))).astype(np.uint8)).cuda()])
    out2, szs2, offs2, _, _, _ = engine.encode_ragged_full(sj.SRC_NV12, nv, nvdims, sj.YUV_420, _quant(), 4)
    for sz in (nvdims, None):
        out, szs, offs, _, _, _ = engine.encode_ragged_oriented(sj.SRC_NV12, nv, nvdims, sz, [1, 1], sj.YUV_420, _quant(), 4)
        assert _streams(out, szs, offs) == _streams(out2, szs2, offs2)
    with pytest.raises(sj.SjpegError, match="SJPEG_HIP_SRC_NV12"):
        engine.encode_ragged_oriented(sj.SRC_NV12, nv, nvdims, None, [1, 6], sj.YUV_420, _quant(), 4)


# ---- 6. the engine's memory

def test_scratch_bytes_and_trim(batch):
    devs, sizes, orients, up_dev, up = batch
    eng = sj.Engine(0)
    planes, dims = _rgb_planes(devs)
    uplanes, udims = _rgb_planes(up_dev)
    eng.encode_ragged_full(sj.SRC_RGB, uplanes, udims, sj.YUV_420, _quant(), 4)       # (what the inner call takes is there already)
    torch.cuda.synchronize()
    before = eng.scratch_bytes()
    frames, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
    arr = np.ascontiguousarray(np.asarray(sizes, np.int32))
    oarr = np.ascontiguousarray(np.asarray(orients, np.uint8))
    need = sj.lib().sjpeg_hip_orient_ragged_bytes(sj.SRC_RGB, len(dims), frames, arr.ctypes.data, oarr.ctypes.data)
    assert need > 0
    out, szs, offs, _, _, _ = eng.encode_ragged_oriented(sj.SRC_RGB, planes, dims, sizes, orients, sj.YUV_420, _quant(), 4)
    _streams(out, szs, offs)
    after = eng.scratch_bytes()
    assert after >= before + need
    eng.trim()
    assert eng.scratch_bytes() <= after - need
    eng.close()
