"""The shaped ragged entries of the C layer called directly through ctypes: for each of the nineteen families (reduced,
resized, oriented, flattened, YUV resized, sheets, flattened sheets; video colour, 16-bit planes and linear light with
their sheets, unsharp on either kind of format, the two resample families, Pillow's filters, compose) and each route of
it, the fused encode entry must
make byte for byte what the two-step call makes -- the family's SHAPE entry into a caller's buffer, then
sjpeg_hip_encode_ragged_full_meta_src (packed: _full_meta_packed_src) on the frames it reports.  Compared: the streams,
sizes, offsets, modes, q_out and value_out, unpacked and packed.

The batch is three pictures of odd, unequal sizes (33 x 17, 16 x 16, 8 x 50: the smallest at which a wrong frame count,
base, stride or sink shows); the shapes factor 2, a fit into 20 x 11, orientation 6 and a 2 x 2 sheet of 16 x 16 cells
(three pictures leave a cell empty); RGBA for the flattened entries, NV12 for the YUV ones, the same planes as 16-bit
words with the byte six bits up (P010) where a depth is given.  The resample families make 20 x 11, 16 x 16 and 8 x 20
from source boxes cut one pixel in on each side, the first turned by orientation 6; the filter is a Gaussian blur of
radius 1, the canvas 24 x 24 with the picture at (2, 3) under one overlay placed from the bottom-right corner.  What is
coded first (picture
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
from sjpeg_amd import resample, unsharp, video

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
    # ... and the same planes as 16-bit words, the byte six bits up: strides in bytes
    deep, frames16 = [(p.to(torch.int16) << 6).contiguous() for p in dev], (sj.RaggedFrame * N)()
    for k, (w, h) in enumerate(DIMS):
        frames16[k].width, frames16[k].height = w, h
        for i in range(2):
            frames16[k].plane[i], frames16[k].row_stride[i] = deep[2 * k + i].data_ptr(), 2 * frames[k].row_stride[i]
    out[P010] = (deep, frames16)
    logo = torch.from_numpy(np.ascontiguousarray(synth.g_noise(4, 4, 99))).cuda()
    logo = torch.cat([logo, torch.full((4, 4, 1), 160, dtype=torch.uint8, device="cuda")], dim=2).contiguous()
    out["logo"] = logo
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
# ... and the twelve newer families.  Their own arguments are the axes; sizes and orientations are one axis of two
# values (both NULL, or SIZES' fit and orientation 6) where a route can end in the _full_meta_ entries, else the second;
# the resample families have their own sizes, which may change a picture's proportions
P010 = "NV12 in 16-bit words"                    # (a key of `pictures`: the format is NV12, the depth says the rest)
SHAPED = {"p-": (None, None), "p<": (SIZES["s<"], ORIENTS["o6"])}
RESAMPLED = {"p<": ([[20, 11], [16, 16], [8, 20]], ORIENTS["o6"])}
UPRIGHT = [[11, 20], [16, 16], [8, 20]]          # (what RESAMPLED makes)
IN_CELL = {"p<": (SHEET_SIZES["s<"], ORIENTS["o6"])}
COLOUR = {"c-": None, "c=": [(0, 0)] * N, "c7": [(1, 1), (0, 0), (1, 0)]}                   # (matrix, range)
DEPTH = {"d-": None, "d+": (2, 6)}                                                           # (bytes, shift)
LIGHT = {"l0": 0, "l1": 1}
UNSHARP = {"u-": None, "u0": [(0, 0)] * N, "u+": [(128, 2), (0, 0), (64, 0)]}                # (amount, threshold)
FILTER = {"k-": None, "k0": [(0, 0.0)] * N, "kg": [(2, 1.0), (0, 0.0), (2, 1.0)]}            # (kind, radius)
COMPOSE = {"x-": None, "x=": [(w, h, 0, 0, 0) for w, h in UPRIGHT], "x+": [(24, 24, 2, 3, 1)] * N}     # (canvas, px, py, nplaces)
_YUV, _LIN, _RES = ("sizes", "orientations", "colour"), ("flatten", "light", "sizes", "orientations"), ("flatten", "sizes", "orientations", "resample")
FAMILIES.update({
    "yuv_converted": ("sjpeg_hip_convert_ragged_yuv_src", sj.SRC_NV12, _YUV, {"shape": SHAPED, "colour": COLOUR}),
    "sheet_yuv_colour": ("sjpeg_hip_sheet_ragged_yuv_colour_src", sj.SRC_NV12, ("sheet",) + _YUV, {"shape": IN_CELL, "colour": COLOUR}),
    "yuv16": ("sjpeg_hip_convert_ragged_yuv16_src", sj.SRC_NV12, _YUV + ("depth",), {"shape": SHAPED, "colour": COLOUR, "depth": {"d+": (2, 6)}}),
    "sheet_yuv16": ("sjpeg_hip_sheet_ragged_yuv16_src", sj.SRC_NV12, ("sheet",) + _YUV + ("depth",),
                    {"shape": IN_CELL, "colour": COLOUR, "depth": {"d+": (2, 6)}}),
    "linear": ("sjpeg_hip_linear_ragged_src", sj.SRC_RGBA, _LIN, {"shape": SHAPED, "flatten": FLATTEN, "light": LIGHT}),
    "sheet_linear": ("sjpeg_hip_sheet_ragged_linear_src", sj.SRC_RGBA, ("sheet",) + _LIN, {"shape": IN_CELL, "flatten": FLATTEN, "light": LIGHT}),
    "unsharp": ("sjpeg_hip_unsharp_ragged_src", sj.SRC_RGBA, _LIN + ("unsharp",),
                {"shape": SHAPED, "flatten": FLATTEN, "light": LIGHT, "unsharp": UNSHARP}),
    "yuv_unsharp": ("sjpeg_hip_unsharp_ragged_yuv_src", sj.SRC_NV12, _YUV + ("depth", "unsharp"),
                    {"shape": SHAPED, "colour": COLOUR, "depth": DEPTH, "unsharp": UNSHARP}),
    "resampled": ("sjpeg_hip_resample_ragged_src", sj.SRC_RGBA, _RES + ("unsharp",), {"shape": RESAMPLED, "flatten": FLATTEN, "unsharp": UNSHARP}),
    "resampled_box": ("sjpeg_hip_resample_box_ragged_src", sj.SRC_RGBA, _RES + ("box", "unsharp"),
                      {"shape": RESAMPLED, "flatten": FLATTEN, "unsharp": UNSHARP}),
    "filtered": ("sjpeg_hip_filter_ragged_src", sj.SRC_RGBA, _RES + ("box", "filter"), {"shape": RESAMPLED, "flatten": FLATTEN, "filter": FILTER}),
    "composed": ("sjpeg_hip_compose_ragged_src", sj.SRC_RGBA, _RES + ("box", "filter", "compose", "overlays", "places"),
                 {"shape": RESAMPLED, "flatten": FLATTEN, "filter": FILTER, "compose": COMPOSE}),
})
SHEET_FAMILIES = ("sheet", "sheet_flat", "sheet_yuv_colour", "sheet_yuv16", "sheet_linear")
# (no flatten: the route of the entry without one, so the two-step call starts with that entry's shape entry)
UNFLATTENED = {"flattened": "sjpeg_hip_orient_ragged_src", "sheet_flat": "sjpeg_hip_sheet_ragged_src"}


def _structs(cls, rows, write):
    arr = (cls * len(rows))()
    for st, row in zip(arr, rows):
        write(st, row)
    return arr


def _newer_args(route, logo):
    """name -> the C values of the newer families' segments on a route, and what keeps them alive"""
    def pair(arr, second=1):
        return (C.addressof(arr), second) if arr is not None else (None, 0)

    def fill(cls, rows, fields):
        return None if rows is None else _structs(cls, rows, lambda st, row: [setattr(st, f, v) for f, v in zip(fields, row)])

    def filt(st, row):
        st.kind, st.radius_x, st.radius_y = row[0], row[1], row[1]

    colour = fill(video._ColourStruct, route.get("colour"), ("matrix", "range"))
    depth = video._DepthStruct(*route["depth"]) if route.get("depth") else None
    sharp = fill(unsharp._UnsharpStruct, route.get("unsharp"), ("amount", "threshold"))
    lanczos = resample._ResampleStruct(4)
    boxes = _structs(resample._BoxStruct, [(1.0, 1.0, w - 1.0, h - 1.0) for w, h in DIMS], lambda st, row: st.box.__setitem__(slice(0, 4), row))
    filters = None if route.get("filter") is None else _structs(resample._FilterStruct, route["filter"], filt)
    compose = fill(resample._ComposeStruct, route.get("compose"), ("canvas_width", "canvas_height", "px", "py", "nplaces"))
    placed = compose is not None and compose[0].nplaces != 0
    overlay = resample._OverlayStruct(logo.data_ptr(), 4, 4, 16)
    place = resample._PlaceStruct(0, 1, 2, 3)    # (overlay 0, one in and two up from the bottom-right corner)
    for st in compose if compose is not None else ():
        st.colour[:] = (200, 30, 90)
    keep = (colour, depth, sharp, lanczos, boxes, filters, compose, overlay, place)
    return {"colour": pair(colour), "depth": C.addressof(depth) if depth is not None else None, "light": route.get("light", 0),
            "unsharp": pair(sharp), "resample": pair(lanczos, 0), "box": pair(boxes), "filter": pair(filters), "compose": pair(compose),
            "overlays": pair(overlay if placed else None), "places": pair(place if placed else None)}, keep


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


def _flat(values):
    """the positional arguments of segments that take one value or a tuple of two"""
    return [v for value in values for v in (value if isinstance(value, tuple) else (value,))]


def _routes(family):
    """(label, {argument: value}) of every route of a family"""
    axes = FAMILIES[family][3]
    for combo in itertools.product(*[a.items() for a in axes.values()]):
        yield "".join(k for k, _ in combo), dict(zip(axes, [v for _, v in combo]))


def _run(engine, pictures, family, route, packed):
    """(fused answer, two-step answer) of one route"""
    L = sj.lib()
    shape_entry, fmt, order, _ = FAMILIES[family]
    frames = pictures[P010 if route.get("depth") else fmt][1]
    sheet_family = family in SHEET_FAMILIES
    if "shape" in route:
        route = dict(route, sizes=route["shape"][0], orientations=route["shape"][1])
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
    newer, keep = _newer_args(route, pictures["logo"])
    fused_args.update(newer)
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
    _check(getattr(L, entry)(engine._h, fmt, N, frames, C.byref(p.params), *_flat(fused_args[name] for name in order), C.addressof(p.meta), 1,
                             *fused.args(strided=sheet_family)), entry)
    got = fused.answer()
    # ---- two steps: the shape entry into a caller's buffer ...
    made, nmade, made_fmt = (sj.RaggedFrame * N)(), C.c_int(N), C.c_int(-1)
    pictures_buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    args = _flat(shape_args[name] for name in shape_order)
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
