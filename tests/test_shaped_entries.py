"""The shaped ragged entries of the C layer called directly through ctypes: for each of the seven families (reduced,
resized, oriented, flattened, YUV resized, sheets, flattened sheets) and each route of it, the fused encode entry must
make byte for byte what the two-step call makes -- the family's SHAPE entry into a caller's buffer, then
sjpeg_hip_encode_ragged_full_meta_src (packed: _full_meta_packed_src) on the frames it reports.  Compared: the streams,
sizes, offsets, modes, q_out and value_out, unpacked and packed.

The batch is three pictures of odd, unequal sizes (33 x 17, 16 x 16, 8 x 50: the smallest at which a wrong frame count,
base, stride or sink shows); the shapes factor 2, a fit into 20 x 11, orientation 6 and a 2 x 2 sheet of 16 x 16 cells
(three pictures leave a cell empty); RGBA for the flattened entries, NV12 for the YUV ones.  What is coded first (picture
0, or the one sheet) has a size search of four passes, so that q_out and value_out carry something; the metadata is
per frame.  A route that an encode entry passes through (factors NULL or all 1, sizes NULL or the frames' own) is stated
to the shape entry by its explicit equivalent where that entry refuses the NULL."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
from oracle import synth

pytestmark = pytest.mark.gpu

DIMS = ((33, 17), (16, 16), (8, 50))
CAP = 1 << 16                                    # a frame's (a sheet's) output range, unpacked
PACKED_CAP = 1 << 20
BOX = (20, 11)
CELL = 16
N = len(DIMS)


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


@pytest.fixture(scope="module")
def pictures():
    """format -> (device tensors kept alive, RaggedFrame[3] without output ranges)"""
    out = {}
    rgb = [synth.g_struct(w, h, 1000 + k) for k, (w, h) in enumerate(DIMS)]
    rgba = [np.concatenate([p, synth.g_noise(p.shape[1], p.shape[0], 77 + k)[..., :1]], axis=2) for k, p in enumerate(rgb)]
    for fmt, host in ((sj.SRC_RGB, rgb), (sj.SRC_RGBA, rgba)):
        dev = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in host]
        frames = (sj.RaggedFrame * N)()
        for k, (w, h) in enumerate(DIMS):
            frames[k].width, frames[k].height = w, h
            frames[k].plane[0], frames[k].row_stride[0] = dev[k].data_ptr(), dev[k].shape[1] * dev[k].shape[2]
        out[fmt] = (dev, frames)
    dev, frames = [], (sj.RaggedFrame * N)()
    for k, (w, h) in enumerate(DIMS):
        cw, ch = (w + 1) // 2, (h + 1) // 2
        y = torch.from_numpy(np.ascontiguousarray(synth.g_struct(w, h, 2000 + k)[..., 0])).cuda()
        uv = torch.from_numpy(np.ascontiguousarray(synth.g_noise(cw, ch, 3000 + k)[..., :2]).reshape(ch, 2 * cw)).cuda()
        dev += [y, uv]
        frames[k].width, frames[k].height = w, h
        frames[k].plane[0], frames[k].row_stride[0] = y.data_ptr(), w
        frames[k].plane[1], frames[k].row_stride[1] = uv.data_ptr(), 2 * cw
    out[sj.SRC_NV12] = (dev, frames)
    torch.cuda.synchronize()
    return out


def _fit(w, h):
    fw, fh = C.c_int(0), C.c_int(0)
    assert sj.lib().sjpeg_hip_fit_size(w, h, BOX[0], BOX[1], C.byref(fw), C.byref(fh)) == 0
    return fw.value, fh.value


def _u8(vals):
    return None if vals is None else np.asarray(vals, np.uint8)


def _i32(vals):
    return None if vals is None else np.ascontiguousarray(np.asarray(vals, np.int32).reshape(-1, 2))


def _ptr(arr):
    return None if arr is None else arr.ctypes.data


# ---- the families: what an entry takes between params (frames, for its shape entry) and the rest, and its routes
FACTORS = {"f-": None, "f1": [1, 1, 1], "f2": [2, 1, 1]}
SIZES = {"s-": None, "s=": [list(d) for d in DIMS], "s<": [[20, 10]] + [list(d) for d in DIMS[1:]]}      # (33 x 17 fitted into BOX)
SHEET_SIZES = {"s-": None, "s<": [[16, 8], [16, 16], [2, 16]]}      # (explicit sizes inside the 16 x 16 cell)
ORIENTS = {"o-": None, "o1": [1, 1, 1], "o6": [6, 1, 1]}
FLATTEN = {"a-": False, "a+": True}
FAMILIES = {
    # name: (shape entry, format, what the entries take between params / frames and the rest, the axes of its routes)
    "reduced": ("sjpeg_hip_reduce_ragged_src", sj.SRC_RGB, ("factors",), {"factors": FACTORS}),
    "resized": ("sjpeg_hip_resize_ragged_src", sj.SRC_RGB, ("sizes",), {"sizes": SIZES}),
    "oriented": ("sjpeg_hip_orient_ragged_src", sj.SRC_RGB, ("sizes", "orientations"), {"sizes": SIZES, "orientations": ORIENTS}),
    "flattened": ("sjpeg_hip_flatten_ragged_src", sj.SRC_RGBA, ("flatten", "sizes", "orientations"),
                  {"flatten": FLATTEN, "sizes": SIZES, "orientations": ORIENTS}),
    "yuv_resized": ("sjpeg_hip_resize_ragged_yuv_src", sj.SRC_NV12, ("sizes", "orientations"), {"sizes": SIZES, "orientations": ORIENTS}),
    "sheet": ("sjpeg_hip_sheet_ragged_src", sj.SRC_RGB, ("sheet", "sizes", "orientations"), {"sizes": SHEET_SIZES, "orientations": ORIENTS}),
    "sheet_flat": ("sjpeg_hip_sheet_ragged_flat_src", sj.SRC_RGBA, ("sheet", "flatten", "sizes", "orientations"),
                   {"flatten": FLATTEN, "sizes": SHEET_SIZES, "orientations": ORIENTS}),
}
# (no flatten: the route of the entry without one, so the two-step call starts with that entry's shape entry)
UNFLATTENED = {"flattened": "sjpeg_hip_orient_ragged_src", "sheet_flat": "sjpeg_hip_sheet_ragged_src"}


def test_the_fitted_size_is_the_one_the_routes_use():
    assert _fit(*DIMS[0]) == (20, 10)


class _Params:
    """sjpeg_hip_ragged_params for `n` coded pictures, the first with a size search of four passes; per-frame metadata"""

    def __init__(self, n):
        L = sj.lib()
        self.quant = np.zeros((1, 2, 64), np.uint8)
        L.sjpeg_hip_quality_matrices(75.0, self.quant.ctypes.data)
        self.search = (sj.SearchParams * n)()
        for k in range(n):
            s = self.search[k]
            s.target_mode, s.target_value, s.passes, s.tolerance, s.qmin, s.qmax = 1, 700.0, (4 if k == 0 else 1), 1.0, 0.0, 100.0
        self.params = sj.RaggedParams(sj.YUV_420, 4, self.quant.ctypes.data, 0, None, 0x78, 12, 1, self.search, 1)
        self.blobs = [b"Exif\0\0" + bytes(range(40)) * (k + 1) for k in range(n)]
        self.meta = (sj.Metadata * n)()
        self.meta_sizes = []
        for k in range(n):
            self.meta[k].exif, self.meta[k].exif_size = self.blobs[k], len(self.blobs[k])
            size = C.c_size_t(0)
            assert L.sjpeg_hip_metadata_size(C.byref(self.meta[k]), C.byref(size)) == 0
            self.meta_sizes.append(size.value)


class _Out:
    """where a call's streams and answers go, and all of it read back"""

    def __init__(self, n, packed):
        self.n, self.packed = n, packed
        self.buf = torch.zeros(PACKED_CAP if packed else n * CAP, dtype=torch.uint8, device="cuda")
        self.sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        self.modes, self.q, self.value = (C.c_int * n)(*[-7] * n), (C.c_float * n)(*[-7.0] * n), (C.c_float * n)(*[-7.0] * n)

    def args(self, strided=False):
        tail = [self.sizes.data_ptr(), self.modes, self.q, self.value, sj.Engine._stream()]
        if self.packed:
            return [self.buf.data_ptr(), PACKED_CAP, self.offsets.data_ptr()] + tail
        return [self.buf.data_ptr()] + ([CAP] if strided else []) + tail

    def answer(self):
        torch.cuda.synchronize()
        sizes = self.sizes.cpu().numpy().tolist()
        offsets = self.offsets.cpu().numpy().tolist() if self.packed else [k * CAP for k in range(self.n)]
        buf = self.buf.cpu().numpy()
        assert all(0 < s <= CAP for s in sizes), sizes
        if self.packed:
            assert 0 < offsets[self.n] <= PACKED_CAP, "the packed buffer overflowed"
            streams = buf[:offsets[self.n]].tobytes()
        else:
            streams = [buf[k * CAP:k * CAP + sizes[k]].tobytes() for k in range(self.n)]
        return streams, sizes, offsets, list(self.modes), list(self.q), list(self.value)


def _check(rc, what):
    assert rc == 0, (what, sj.lib().sjpeg_hip_last_error().decode())


def _routes(family):
    """(label, {argument: value}) of every route of a family"""
    axes = FAMILIES[family][3]
    for combo in itertools.product(*[a.items() for a in axes.values()]):
        yield "".join(k for k, _ in combo), dict(zip(axes, [v for _, v in combo]))


def _run(engine, pictures, family, route, packed):
    """(fused answer, two-step answer) of one route"""
    L = sj.lib()
    shape_entry, fmt, order, _ = FAMILIES[family]
    frames = pictures[fmt][1]
    sheet_family = family in ("sheet", "sheet_flat")
    factors, sizes, orients = _u8(route.get("factors")), _i32(route.get("sizes")), _u8(route.get("orientations"))
    flatten = sj._FlattenStruct((C.c_uint8 * 3)(17, 128, 250), 0, 255.0, 0.0) if route.get("flatten") else None
    sheet = sj._SheetStruct(2, 2, CELL, CELL, 2, 2, (C.c_uint8 * 3)(10, 20, 30), 0)
    n = 1 if sheet_family else N
    p = _Params(n)
    for k in range(N):
        frames[k].out_offset, frames[k].out_capacity = (0 if packed else k * CAP), CAP
    # (the shape entries of reduce and resize refuse a NULL: they get its explicit equivalent)
    ones, own = _u8([1] * N), _i32([list(d) for d in DIMS])
    fused_args = {"factors": _ptr(factors), "sizes": _ptr(sizes), "orientations": _ptr(orients), "sheet": C.addressof(sheet),
                  "flatten": C.addressof(flatten) if flatten is not None else None}
    shape_args = dict(fused_args)
    if family == "reduced" and factors is None:
        shape_args["factors"] = _ptr(ones)
    if family == "resized" and sizes is None:
        shape_args["sizes"] = _ptr(own)
    shape_order = order
    if family in UNFLATTENED and flatten is None:
        shape_entry, shape_order = UNFLATTENED[family], tuple(name for name in order if name != "flatten")

    # ---- fused
    fused = _Out(n, packed)
    entry = "sjpeg_hip_encode_ragged_%s%s_src" % (family, "_packed" if packed else "")
    _check(getattr(L, entry)(engine._h, fmt, N, frames, C.byref(p.params), *[fused_args[name] for name in order], C.addressof(p.meta), 1,
                             *fused.args(strided=sheet_family)), entry)
    got = fused.answer()
    # ---- two steps: the shape entry into a caller's buffer ...
    made, nmade, made_fmt = (sj.RaggedFrame * N)(), C.c_int(N), C.c_int(-1)
    pictures_buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    args = [shape_args[name] for name in shape_order]
    tail = [pictures_buf.data_ptr(), pictures_buf.numel(), made] + ([C.byref(nmade)] if sheet_family else []) + [C.byref(made_fmt),
                                                                                                                 sj.Engine._stream()]
    _check(getattr(L, shape_entry)(engine._h, fmt, N, frames, *args, *tail), shape_entry)
    assert nmade.value == n
    # ... then the _full_meta_ call on the frames it reports, at the fused call's output ranges
    for k in range(n):
        made[k].out_offset = 0 if packed else k * CAP
        made[k].out_capacity = CAP
        if sheet_family and packed:
            made[k].out_capacity = L.sjpeg_hip_frame_bound(made[k].width, made[k].height, sj.YUV_444, 2048 + p.meta_sizes[k])
    two = _Out(n, packed)
    entry = "sjpeg_hip_encode_ragged_full_meta%s_src" % ("_packed" if packed else "")
    _check(getattr(L, entry)(engine._h, made_fmt.value, n, made, C.byref(p.params), C.addressof(p.meta), 1, *two.args()), entry)
    want = two.answer()
    return got, want


@pytest.mark.parametrize("packed", [False, True], ids=["unpacked", "packed"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_fused_entry_equals_shape_entry_then_full_meta(engine, pictures, family, packed):
    seen = 0
    for label, route in _routes(family):
        got, want = _run(engine, pictures, family, route, packed)
        for name, g, w in zip(("streams", "sizes", "offsets", "modes", "q_out", "value_out"), got, want):
            assert g == w, (family, label, name)
        assert got[4][0] > 0 and got[5][0] > 0, (family, label, "the search left no answer")
        seen += 1
    assert seen == int(np.prod([len(a) for a in FAMILIES[family][3].values()]))
