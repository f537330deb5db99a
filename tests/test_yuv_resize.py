"""Decoded video resized and turned inside the ragged call on the GPU (sjpeg_hip_resize_ragged_yuv_src,
sjpeg_hip_encode_ragged_yuv_resized_src, encode_yuv_frames).  The contract is sjpeg_hip.h's: every plane of an NV12,
NV21, YUV420 or YUV444 frame is resized as a gray picture of its own by the exact area average, turned as a picture of
its own by the EXIF table, and the JPEG is what encode_ragged_full makes of the three planes handed over as planar
4:2:0 (YUV444: 4:4:4).  The model is here: _area() with Python integers, _turn() with numpy flips and transposes.  No
tolerance anywhere: every comparison is byte equality."""
import numpy as np
import pytest
import torch

import sjpeg_amd as sj

pytestmark = pytest.mark.gpu

FORMATS = {"nv12": sj.SRC_NV12, "nv21": sj.SRC_NV21, "yuv420": sj.SRC_YUV420, "yuv444": sj.SRC_YUV444}
# (W x H -> w' x h'): odd everywhere at a ratio that is no integer; a chroma plane of one sample, twice; the identity on
# one axis; 64 lanes a column (chroma 320 x 3 -> 3 x 2); a whole ratio; a tile whose segment of a row is longer than the
# staging memory, for luma and for the two-byte pixels of a UV plane alike, so that both go in chunks
CASES = [((37, 23), (13, 9)), ((1, 1), (1, 1)), ((2, 1), (1, 1)), ((16, 16), (16, 7)), ((640, 6), (5, 3)), ((18, 18), (9, 9)),
         ((20001, 3), (4, 2))]
TURNED = [((37, 23), (13, 9)), ((20, 12), (10, 6))]
SENTINEL = 0x5A


# ---- the model

def _span(i, n, m):
    """the source samples that output sample i of m covers among n, with their weights: sjpeg_hip.h's formula"""
    out = []
    x = i * n // m
    while x < n and x * m < (i + 1) * n:
        w = min((x + 1) * m, (i + 1) * n) - max(x * m, i * n)
        if w > 0:
            out.append((x, w))
        x += 1
    assert sum(w for _, w in out) == n
    return out


def _area(plane, w2, h2):
    """the exact area average of a uint8 plane [H, W], in Python integers: round half up"""
    H, W = plane.shape
    rows = plane.tolist()
    xs, ys = [_span(i, W, w2) for i in range(w2)], [_span(j, H, h2) for j in range(h2)]
    hsum = [[sum(w * row[x] for x, w in xs[i]) for i in range(w2)] for row in rows]
    out = np.empty((h2, w2), np.uint8)
    for j in range(h2):
        for i in range(w2):
            S = sum(w * hsum[y][i] for y, w in ys[j])
            out[j, i] = (2 * S + W * H) // (2 * W * H)
    return out


def _turn(R, o):
    """sjpeg_hip.h's table on a plane [h, w]: U(x, y) = R(sx, sy)"""
    return {1: R, 2: R[:, ::-1], 3: R[::-1, ::-1], 4: R[::-1], 5: R.T, 6: R[::-1].T, 7: R[::-1, ::-1].T, 8: R[:, ::-1].T}[o]


def _chroma(fmt, w, h):
    return (w, h) if fmt == sj.SRC_YUV444 else ((w + 1) // 2, (h + 1) // 2)


def _model(planes, fmt, size, o=1):
    """the three made planes of a frame whose planes are (y, u, v) uint8 arrays"""
    cw, ch = _chroma(fmt, *size)
    made = [_area(planes[0], *size), _area(planes[1], cw, ch), _area(planes[2], cw, ch)]
    return [np.ascontiguousarray(_turn(p, o)) for p in made]


def test_the_model_itself():
    """a box average where the ratio is whole; the identity; the table, sample by sample"""
    rs = np.random.RandomState(1)
    p = rs.randint(0, 256, (18, 18)).astype(np.uint8)
    box = (p.astype(np.int64).reshape(9, 2, 9, 2).sum((1, 3)) * 2 + 4) // 8
    assert np.array_equal(_area(p, 9, 9), box.astype(np.uint8)) and np.array_equal(_area(p, 18, 18), p)
    assert _area(np.array([[1, 2]], np.uint8), 1, 1)[0, 0] == 2                 # 1.5 rounds up
    R = np.arange(6, dtype=np.uint8).reshape(2, 3)
    w, h = 3, 2
    table = {1: lambda x, y: (x, y), 2: lambda x, y: (w - 1 - x, y), 3: lambda x, y: (w - 1 - x, h - 1 - y),
             4: lambda x, y: (x, h - 1 - y), 5: lambda x, y: (y, x), 6: lambda x, y: (y, h - 1 - x),
             7: lambda x, y: (w - 1 - y, h - 1 - x), 8: lambda x, y: (w - 1 - y, x)}
    for o in range(1, 9):
        U = _turn(R, o)
        assert U.shape == ((3, 2) if o >= 5 else (2, 3))
        for y in range(U.shape[0]):
            for x in range(U.shape[1]):
                sx, sy = table[o](x, y)
                assert U[y, x] == R[sy, sx], (o, x, y)


# ---- the frames

def _source(fmt, w, h, seed):
    """(y, u, v) uint8 arrays of a w x h picture of the format's sampling: noise, so that no two samples need agree"""
    rs = np.random.RandomState(seed)
    cw, ch = _chroma(fmt, w, h)
    return [rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (ch, cw)).astype(np.uint8),
            rs.randint(0, 256, (ch, cw)).astype(np.uint8)]


def _device_planes(fmt, yuv):
    """the caller's planes of a frame: [y, uv] for the semi-planar formats (NV21: V first), else [y, u, v]"""
    y, u, v = yuv
    if fmt in (sj.SRC_NV12, sj.SRC_NV21):
        first, second = (u, v) if fmt == sj.SRC_NV12 else (v, u)
        uv = np.stack([first, second], axis=-1).reshape(u.shape[0], 2 * u.shape[1])
        return [torch.from_numpy(y).cuda(), torch.from_numpy(np.ascontiguousarray(uv)).cuda()]
    return [torch.from_numpy(p).cuda() for p in yuv]


def _bottom_up(t):
    """a plane stored bottom-up inside a larger tensor of sentinels: (address of row 0, negative stride), and the tensor"""
    rows, nb = t.shape
    big = torch.full((rows + 2, nb + 13), SENTINEL, dtype=torch.uint8, device="cuda")
    big[1:rows + 1, 5:5 + nb] = t.flip(0)
    return (big.data_ptr() + rows * big.stride(0) + 5, -big.stride(0)), big


def _padded(t):
    rows, nb = t.shape
    big = torch.full((rows + 2, nb + 29), SENTINEL, dtype=torch.uint8, device="cuda")
    big[1:rows + 1, 3:3 + nb] = t
    return big[1:rows + 1, 3:3 + nb], big


def _untouched(big, t, col, flipped):
    host = big.cpu().numpy().copy()
    rows, nb = t.shape
    inner = host[1:rows + 1, col:col + nb]
    assert np.array_equal(inner[::-1] if flipped else inner, t.cpu().numpy())
    host[1:rows + 1, col:col + nb] = SENTINEL
    assert (host == SENTINEL).all()


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.fixture(scope="module")
def batches():
    """per format: the sources of CASES, then the 37 x 23 case twice more (to be stored bottom-up and padded), and the
    model's planes of every frame.  Computed once, never written to."""
    out = {}
    for name, fmt in FORMATS.items():
        dims = [c[0] for c in CASES] + [CASES[0][0]] * 2
        sizes = [c[1] for c in CASES] + [CASES[0][1]] * 2
        srcs = [_source(fmt, w, h, 4100 + 10 * k) for k, (w, h) in enumerate(dims)]
        out[name] = (dims, sizes, srcs, [_model(s, fmt, size) for s, size in zip(srcs, sizes)])
    return out


def _check_planes(pics, wants):
    torch.cuda.synchronize()
    assert len(pics) == len(wants)
    for k, (pic, want) in enumerate(zip(pics, wants)):
        assert len(pic) == 3
        for c in range(3):
            got = pic[c].cpu().numpy()
            assert got.shape == want[c].shape, (k, c, got.shape, want[c].shape)
            assert np.array_equal(got, want[c]), (k, c, want[c].shape, np.argwhere(got != want[c])[:4])
            assert pic[c].data_ptr() % 16 == 0 and pic[c].stride(0) == (want[c].shape[1] + 3) // 4 * 4 and pic[c].stride(1) == 1


def _planes_of_batch(fmt, srcs):
    """the device planes of a batch; the last two frames bottom-up and padded, views into tensors of sentinels"""
    planes, keep = [], []
    for k, s in enumerate(srcs):
        dev = _device_planes(fmt, s)
        if k == len(srcs) - 2:
            made = [_bottom_up(t) for t in dev]
            keep.append(("up", dev, [m[1] for m in made]))
            planes.append([m[0] for m in made])
        elif k == len(srcs) - 1:
            made = [_padded(t) for t in dev]
            keep.append(("pad", dev, [m[1] for m in made]))
            planes.append([m[0] for m in made])
        else:
            keep.append(("plain", dev, None))
            planes.append(dev)
    return planes, keep


# ---- 1. the kernel alone: ONE ragged call per format over every case

@pytest.mark.parametrize("name", list(FORMATS))
def test_planes_against_the_model(engine, batches, name):
    fmt = FORMATS[name]
    dims, sizes, srcs, wants = batches[name]
    planes, keep = _planes_of_batch(fmt, srcs)
    frames, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
    arr = np.ascontiguousarray(np.asarray(sizes, np.int32))
    need = sj.lib().sjpeg_hip_resize_ragged_yuv_bytes(fmt, len(dims), frames, arr.ctypes.data, None)
    assert need > 0 and need % 16 == 0
    guard = 256
    whole = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    assert (whole.data_ptr() + guard) % 16 == 0
    out_fmt, pics, buf = engine.resize_ragged_yuv(fmt, planes, dims, sizes, out=whole[guard:guard + need])
    assert out_fmt == (sj.SRC_YUV444 if fmt == sj.SRC_YUV444 else sj.SRC_YUV420)
    _check_planes(pics, wants)
    host = whole.cpu().numpy()
    assert (host[:guard] == 0xA5).all() and (host[guard + need:] == 0xA5).all()
    # frame after frame Y, U, V
    at = whole.data_ptr() + guard
    for pic in pics:
        for p in pic:
            assert p.data_ptr() == at
            at += (p.stride(0) * p.shape[0] + 15) & ~15
    assert at == whole.data_ptr() + guard + need
    # the sources were read, not written, and nothing around them matters
    for kind, dev, bigs in keep:
        for t, big in zip(dev, bigs or []):
            _untouched(big, t, 5 if kind == "up" else 3, kind == "up")
    # one byte short is refused before anything runs
    with pytest.raises(sj.SjpegError, match="bytes"):
        engine.resize_ragged_yuv(fmt, planes, dims, sizes, out=whole[guard:guard + need - 16][:need - 1])
    # picture k + 1 does not depend on picture k being in the batch
    _, fewer, _ = engine.resize_ragged_yuv(fmt, planes[1:], dims[1:], sizes[1:])
    _check_planes(fewer, wants[1:])
    # the luma plane is what the shipped gray resize makes of it alone
    rfmt, gray, _ = engine.resize_ragged(sj.SRC_GRAY, [[p[0]] for p in planes], dims, sizes)
    torch.cuda.synchronize()
    assert rfmt == sj.SRC_GRAY
    for k, (g, pic) in enumerate(zip(gray, pics)):
        assert torch.equal(g, pic[0]), k


def test_nv12_nv21_and_yuv420_of_one_picture_agree(engine, batches):
    dims, sizes, srcs, wants = batches["yuv420"]
    orients = [1 + k % 8 for k in range(len(dims))]
    made = {}
    for name in ("nv12", "nv21", "yuv420"):
        planes = [_device_planes(FORMATS[name], s) for s in srcs]
        out_fmt, pics, _ = engine.resize_ragged_yuv(FORMATS[name], planes, dims, sizes, orients)
        torch.cuda.synchronize()
        assert out_fmt == sj.SRC_YUV420
        made[name] = [[p.cpu().numpy() for p in pic] for pic in pics]
    for k in range(len(dims)):
        for c in range(3):
            assert np.array_equal(made["nv12"][k][c], made["yuv420"][k][c]), (k, c)
            assert np.array_equal(made["nv21"][k][c], made["yuv420"][k][c]), (k, c)


# ---- 2. the eight orientations, mixed with 1 in one batch

@pytest.fixture(scope="module")
def turned():
    out = {}
    for name, fmt in FORMATS.items():
        dims, sizes, orients, srcs, wants = [], [], [], [], []
        for k, ((w, h), size) in enumerate(TURNED):
            s = _source(fmt, w, h, 4500 + k)
            for o in range(1, 9):
                for oo in (o, 1):                    # (every turned frame has an upright neighbour)
                    dims.append((w, h)); sizes.append(size); orients.append(oo); srcs.append(s)
                    wants.append(_model(s, fmt, size, oo))
        out[name] = (dims, sizes, orients, srcs, wants)
    return out


@pytest.mark.parametrize("name", list(FORMATS))
def test_orientations_against_the_turned_model(engine, turned, name):
    fmt = FORMATS[name]
    dims, sizes, orients, srcs, wants = turned[name]
    planes = [_device_planes(fmt, s) for s in srcs]
    out_fmt, pics, _ = engine.resize_ragged_yuv(fmt, planes, dims, sizes, orients)
    _check_planes(pics, wants)
    for pic, size, o in zip(pics, sizes, orients):
        uw, uh = sj.oriented_size(*size, o)
        assert (pic[0].shape[1], pic[0].shape[0]) == (uw, uh)
        for c in (1, 2):                             # (the turned chroma planes' size is the one the upright luma's implies)
            assert (pic[c].shape[1], pic[c].shape[0]) == sj.yuv_plane_size(out_fmt, uw, uh, c)
    # sizes None: the pure turn of every plane at its own size
    _, own, _ = engine.resize_ragged_yuv(fmt, planes[:4], dims[:4], None, [6, 1, 3, 8])
    _check_planes(own, [[np.ascontiguousarray(_turn(p, o)) for p in s] for s, o in zip(srcs[:4], [6, 1, 3, 8])])


# ---- 3. the contract: the JPEGs are encode_ragged_full's of the model planes

ENC = [((37, 23), (13, 9), 6), ((640, 6), (5, 3), 1), ((20, 12), (10, 6), 3)]


def _quant(q=75.0):
    m = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(float(q), m.ctypes.data)
    return m


def _streams(out, sizes, offs):
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    return [host[int(offs[k]):int(offs[k]) + int(sz[k])].tobytes() for k in range(len(sz))]


@pytest.fixture(scope="module")
def enc():
    """per format: (the caller's planes, dims, sizes, orientations, the model planes uploaded, their dims, out_fmt, mode)"""
    out = {}
    for name, fmt in FORMATS.items():
        srcs = [_source(fmt, w, h, 4700 + k) for k, ((w, h), _, _) in enumerate(ENC)]
        model = [_model(s, fmt, size, o) for s, (_, size, o) in zip(srcs, ENC)]
        out[name] = ([_device_planes(fmt, s) for s in srcs], [e[0] for e in ENC], [e[1] for e in ENC], [e[2] for e in ENC],
                     [[torch.from_numpy(p).cuda() for p in m] for m in model], [(m[0].shape[1], m[0].shape[0]) for m in model],
                     sj.SRC_YUV444 if fmt == sj.SRC_YUV444 else sj.SRC_YUV420, sj.YUV_444 if fmt == sj.SRC_YUV444 else sj.YUV_420)
    return out


VARIANTS = {
    "method 0": dict(method=0),
    "method 4": dict(method=4),
    "method 4 with the trellis": dict(method=7),
    "target size": dict(method=4, search=[dict(target_mode=sj.TARGET_SIZE, target_value=t) for t in (300, 260, 280)]),
    "metadata": dict(method=4, metadata=[sj.PictureMetadata(exif=b"Exif\0\0II*\0\x08\0\0\0\0\0\0\0\0\0", xmp=b"<x:xmpmeta>0</x:xmpmeta>"),
                                         None, sj.PictureMetadata(iccp=b"profile " * 9, app_markers=b"\xff\xe5\x00\x04ab")]),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(FORMATS))
def test_the_jpegs_are_those_of_the_model_planes(engine, enc, name, variant):
    planes, dims, sizes, orients, mplanes, mdims, out_fmt, mode = enc[name]
    kw = VARIANTS[variant]
    out, szs, offs, modes, q, v = engine.encode_ragged_yuv_resized(FORMATS[name], planes, dims, sizes, orients, mode, _quant(), **kw)
    out2, szs2, offs2, modes2, q2, v2 = engine.encode_ragged_full(out_fmt, mplanes, mdims, mode, _quant(), **kw)
    got, want = _streams(out, szs, offs), _streams(out2, szs2, offs2)
    assert all(len(w) > 0 for w in want) and got == want
    assert modes == modes2 == [mode] * len(dims) and q == q2 and v == v2
    assert offs == offs2                             # (the default capacities are the bounds of the upright sizes)
    assert engine.search_stats() is not None


@pytest.mark.parametrize("name", list(FORMATS))
def test_the_packed_entry(engine, enc, name):
    planes, dims, sizes, orients, mplanes, mdims, out_fmt, mode = enc[name]
    search = [dict(target_mode=sj.TARGET_SIZE, target_value=t) for t in (300, 260, 280)]
    for kw in (dict(method=4), dict(method=4, search=search)):
        out, szs, offs, modes, q, v = engine.encode_ragged_yuv_resized_packed(FORMATS[name], planes, dims, sizes, orients, mode, _quant(), **kw)
        out2, szs2, offs2, modes2, q2, v2 = engine.encode_ragged_full_packed(out_fmt, mplanes, mdims, mode, _quant(), **kw)
        torch.cuda.synchronize()
        assert offs.cpu().tolist() == offs2.cpu().tolist() and szs.cpu().tolist() == szs2.cpu().tolist()
        got = _streams(out, szs, offs.cpu().numpy())
        assert all(len(g) > 0 for g in got) and got == _streams(out2, szs2, offs2.cpu().numpy())
        assert modes == modes2 and q == q2 and v == v2
    # ... and the unpacked entry's streams
    out3, szs3, offs3, _, _, _ = engine.encode_ragged_yuv_resized(FORMATS[name], planes, dims, sizes, orients, mode, _quant(), method=4,
                                                                  search=search)
    assert got == _streams(out3, szs3, offs3)


# ---- 4. nothing to do: the _full_ call on the caller's frames, no kernel, no memory

def test_own_sizes_and_all_ones_pass_through(enc):
    planes, dims, sizes, orients, mplanes, mdims, out_fmt, mode = enc["nv12"]
    eng = sj.Engine(0)
    out2, szs2, offs2, _, _, _ = eng.encode_ragged_full(sj.SRC_NV12, planes, dims, sj.YUV_420, _quant(), 4)
    want = _streams(out2, szs2, offs2)
    out2, szs2, offs2, _, _, _ = eng.encode_ragged_full_packed(sj.SRC_NV12, planes, dims, sj.YUV_420, _quant(), 4)
    assert _streams(out2, szs2, offs2.cpu().numpy()) == want
    before = eng.scratch_bytes()                     # (what the two inner calls take is there already)
    for sz, o in ((None, None), (dims, None), (None, [1] * len(dims)), (dims, [1] * len(dims))):
        out, szs, offs, _, _, _ = eng.encode_ragged_yuv_resized(sj.SRC_NV12, planes, dims, sz, o, sj.YUV_420, _quant(), 4)
        assert _streams(out, szs, offs) == want
        out, szs, offs, _, _, _ = eng.encode_ragged_yuv_resized_packed(sj.SRC_NV12, planes, dims, sz, o, sj.YUV_420, _quant(), 4)
        assert _streams(out, szs, offs.cpu().numpy()) == want
    assert eng.scratch_bytes() == before
    # with a turn the kernel's memory is the engine's: counted, and released by trim
    frames, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
    arr = np.ascontiguousarray(np.asarray(sizes, np.int32))
    oarr = np.ascontiguousarray(np.asarray(orients, np.uint8))
    need = sj.lib().sjpeg_hip_resize_ragged_yuv_bytes(sj.SRC_NV12, len(dims), frames, arr.ctypes.data, oarr.ctypes.data)
    out, szs, offs, _, _, _ = eng.encode_ragged_yuv_resized(sj.SRC_NV12, planes, dims, sizes, orients, sj.YUV_420, _quant(), 4)
    _streams(out, szs, offs)
    after = eng.scratch_bytes()
    assert need > 0 and after >= before + need
    eng.trim()
    assert eng.scratch_bytes() <= after - need
    with pytest.raises(sj.SjpegError, match="yuv_mode does not match the source format"):
        eng.encode_ragged_yuv_resized(sj.SRC_NV12, planes, dims, sizes, orients, sj.YUV_444, _quant(), 4)
    with pytest.raises(sj.SjpegError, match="SJPEG_HIP_SRC_RGB is not a YUV-plane format"):
        eng.encode_ragged_yuv_resized(sj.SRC_RGB, [[p[0]] for p in planes], [(4, 4)] * 3, None, None, sj.YUV_420, _quant(), 4)
    eng.close()


# ---- 5. a frame that does not fit reports size 0; its neighbours are exact

@pytest.mark.parametrize("name", ["nv12", "yuv444"])
def test_a_capacity_too_small_is_size_0(engine, enc, name):
    planes, dims, sizes, orients, mplanes, mdims, out_fmt, mode = enc[name]
    out2, szs2, offs2, _, _, _ = engine.encode_ragged_full(out_fmt, mplanes, mdims, mode, _quant(), 4)
    want = _streams(out2, szs2, offs2)
    caps = [sj.frame_bound(w, h, mode, 2048) for (w, h) in mdims]
    caps[1] = len(want[1]) - 1
    out, szs, offs, _, _, _ = engine.encode_ragged_yuv_resized(FORMATS[name], planes, dims, sizes, orients, mode, _quant(), 4, capacities=caps)
    got = _streams(out, szs, offs)
    assert szs.cpu().tolist()[1] == 0 and got[0] == want[0] and got[2] == want[2]


# ---- 6. the thumbnail call

@pytest.mark.parametrize("name", list(FORMATS))
def test_encode_yuv_frames_fits_the_upright_box(engine, enc, name):
    planes, dims, _, orients, _, _, out_fmt, mode = enc[name]
    fmt = FORMATS[name]
    sizes = [sj.fit_size(w, h, (8, 8)) for (w, h) in dims]           # (a square box: the same stored and upright)
    out, szs, offs, _, _, _ = engine.encode_ragged_yuv_resized(fmt, planes, dims, sizes, orients, mode, _quant(80.0), 4)
    want = _streams(out, szs, offs)
    frames = [tuple(p) for p in planes]
    assert sj.encode_yuv_frames(frames, fmt, box=(8, 8), orientations=orients, quality=80.0, engine=engine) == want
    assert sj.encode_yuv_frames(frames, fmt, sizes=sizes, orientations=orients, quality=80.0, packed=True, engine=engine) == want
    # a box that is no square is the UPRIGHT picture's: the 37 x 23 frame, turned by 6, is fitted into 16 x 8 as stored
    one = sj.encode_yuv_frames(frames[:1], fmt, box=(8, 16), orientations=6, engine=engine)
    out, szs, offs, _, _, _ = engine.encode_ragged_yuv_resized(fmt, planes[:1], dims[:1], [sj.fit_size(37, 23, (16, 8))], [6], mode, _quant(), 4)
    assert one == _streams(out, szs, offs)
    with pytest.raises(sj.SjpegError, match="not both"):
        sj.encode_yuv_frames(frames, fmt, sizes=sizes, box=(8, 8), engine=engine)
    with pytest.raises(sj.SjpegError, match="planes"):
        sj.encode_yuv_frames([f[:1] for f in frames], fmt, engine=engine)
