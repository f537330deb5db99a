"""Decoded video with its colour put right inside the ragged call (sjpeg_hip.h, "video colour converted inside the
ragged call").  A JFIF file is full-range BT.601 YCbCr; a decoded H.264 or HEVC frame is mostly BT.709 and nearly always
studio range.  encode_yuv_frames / encode_yuv_sheets code the samples as they are; the calls here say what the SOURCE
is -- a VideoColour, one for all frames or one per frame -- and the library converts the made thumbnails, not the
sources, by one more launch behind the resize launch.  The arithmetic is exact and in integers: yuv_colour_samples is
the formula on single samples."""
import ctypes as C

import numpy as np

import sjpeg_amd as sj
from sjpeg_amd import SRC_NV12, SRC_YUV444, YUV_420, YUV_444, RaggedFrame, SjpegError, lib

MATRIX_BT601, MATRIX_BT709 = 0, 1        # SJPEG_HIP_MATRIX_*
RANGE_FULL, RANGE_LIMITED = 0, 1         # SJPEG_HIP_RANGE_*
_MATRICES = {"bt601": MATRIX_BT601, "bt709": MATRIX_BT709}
_RANGES = {"full": RANGE_FULL, "limited": RANGE_LIMITED}


class _ColourStruct(C.Structure):
    """struct sjpeg_hip_yuv_colour"""
    _fields_ = [("matrix", C.c_uint8), ("range", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class VideoColour:
    """What a video source's samples mean: matrix "bt601" or "bt709" (the Kr, Kb of its Y'CbCr), range "full" (0..255)
    or "limited" (studio: Y 16..235, chroma 16..240); MATRIX_* / RANGE_* serve too.  The default is what an HD stream
    is.  VideoColour("bt601", "full") is JFIF's own colour: nothing is converted."""

    def __init__(self, matrix="bt709", range="limited"):
        self.matrix = _MATRICES.get(matrix.lower(), None) if isinstance(matrix, str) else matrix
        self.range = _RANGES.get(range.lower(), None) if isinstance(range, str) else range
        if self.matrix not in (MATRIX_BT601, MATRIX_BT709) or isinstance(self.matrix, bool):
            raise SjpegError(f"VideoColour: matrix {matrix!r} is not 'bt601' or 'bt709'")
        if self.range not in (RANGE_FULL, RANGE_LIMITED) or isinstance(self.range, bool):
            raise SjpegError(f"VideoColour: range {range!r} is not 'full' or 'limited'")

    @property
    def identity(self):
        return self.matrix == MATRIX_BT601 and self.range == RANGE_FULL

    def __eq__(self, other):
        return isinstance(other, VideoColour) and (self.matrix, self.range) == (other.matrix, other.range)

    def __hash__(self):
        return hash((self.matrix, self.range))

    def __repr__(self):
        return "VideoColour(%r, %r)" % ({v: k for k, v in _MATRICES.items()}[self.matrix], {v: k for k, v in _RANGES.items()}[self.range])

    def _struct(self):
        return _ColourStruct(self.matrix, self.range)


_bound = False


def _lib():
    """the library with the argument types of the entries this module binds"""
    global _bound
    L = lib()
    if _bound:
        return L
    L.sjpeg_hip_yuv_colour_samples.restype = C.c_int
    L.sjpeg_hip_yuv_colour_samples.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    colour = [C.c_void_p, C.c_int]
    plain = list(L.sjpeg_hip_resize_ragged_yuv_src.argtypes)            # (..., sizes, orientations, d_out, ...)
    L.sjpeg_hip_convert_ragged_yuv_src.restype = C.c_int
    L.sjpeg_hip_convert_ragged_yuv_src.argtypes = plain[:6] + colour + plain[6:]
    plain = list(L.sjpeg_hip_sheet_ragged_src.argtypes)                 # (..., sheet, sizes, orientations, d_out, ...)
    L.sjpeg_hip_sheet_ragged_yuv_colour_src.restype = C.c_int
    L.sjpeg_hip_sheet_ragged_yuv_colour_src.argtypes = plain[:7] + colour + plain[7:]
    for packed in ("", "_packed"):
        plain = list(getattr(L, f"sjpeg_hip_encode_ragged_yuv_resized{packed}_src").argtypes)    # (..., params, sizes, orientations, meta, ...)
        fn = getattr(L, f"sjpeg_hip_encode_ragged_yuv_converted{packed}_src")
        fn.restype, fn.argtypes = C.c_int, plain[:7] + colour + plain[7:]
        plain = list(getattr(L, f"sjpeg_hip_encode_ragged_sheet{packed}_src").argtypes)          # (..., params, sheet, sizes, orientations, meta, ...)
        fn = getattr(L, f"sjpeg_hip_encode_ragged_sheet_yuv_colour{packed}_src")
        fn.restype, fn.argtypes = C.c_int, plain[:8] + colour + plain[8:]
    _bound = True
    return L


def _colour_args(who, n, colour):
    """(the struct array, its address, whether there is one per frame) of one VideoColour or a sequence of one per frame;
    None: no colour at all, the entries' NULL"""
    if colour is None:
        return None, None, 0
    if isinstance(colour, VideoColour):
        arr = (_ColourStruct * 1)(colour._struct())
        return arr, C.addressof(arr), 0
    try:
        colours = list(colour)
    except TypeError:
        raise SjpegError(f"{who}: colour {colour!r} is not a VideoColour or a sequence of one per frame")
    if len(colours) != n or not all(isinstance(c, VideoColour) for c in colours):
        raise SjpegError(f"{who}: colour is one VideoColour or a sequence of one per frame ({n})")
    arr = (_ColourStruct * n)(*[c._struct() for c in colours])
    return arr, C.addressof(arr), 1


def yuv_colour_samples(yuv, colour=VideoColour()):
    """sjpeg_hip_yuv_colour_samples: the conversion's formula on single samples, host only.  yuv: uint8 [..., 3] of
    (Y, U, V) triples of a source of `colour`; returns the same shape in JFIF's colour -- each triple what the calls
    below make of a one-sample picture."""
    who = "yuv_colour_samples"
    if not isinstance(colour, VideoColour):
        raise SjpegError(f"{who}: colour {colour!r} is not a VideoColour")
    src = np.ascontiguousarray(yuv, dtype=np.uint8)
    if src.ndim < 1 or src.shape[-1] != 3:
        raise SjpegError(f"{who}: yuv is uint8 [..., 3] of (Y, U, V) triples")
    out = np.empty_like(src)
    st = colour._struct()
    if _lib().sjpeg_hip_yuv_colour_samples(C.addressof(st), src.size // 3, src.ctypes.data, out.ctypes.data) != 0:
        raise SjpegError(f"sjpeg_hip_yuv_colour_samples failed: {sj.last_error()}")
    return out


def _size_list(who, n, dims, sizes, box, orientations):
    """sizes, or the frames fitted into box (the UPRIGHT one), as encode_yuv_frames takes them"""
    if sizes is not None and box is not None:
        raise SjpegError(f"{who}: give sizes or box, not both")
    if box is None:
        return sizes
    try:
        bw, bh = box
    except (TypeError, ValueError):
        raise SjpegError(f"{who}: box {box!r} is not a pair (width, height)")
    return [sj.fit_size(w, h, (bh, bw) if orientations is not None and orientations[k] >= 5 else (bw, bh))
            for k, (w, h) in enumerate(dims)]


def convert_yuv_frames(frames, fmt=SRC_NV12, colour=VideoColour(), sizes=None, box=None, orientations=None, engine=None, out=None):
    """sjpeg_hip_convert_ragged_yuv_src: the planes Engine.resize_ragged_yuv makes of the frames (frames, fmt, sizes /
    box, orientations as encode_video_frames), converted from `colour` to JFIF's in place by one more launch.  Returns
    (out_fmt, pictures, buf) as resize_ragged_yuv: picture k a tuple (y, u, v) of uint8 views into buf, which any ragged
    entry takes as SRC_YUV420 / SRC_YUV444 planes.  Asynchronous on the current torch stream."""
    import torch
    who = "convert_yuv_frames"
    planes, dims, dev = sj._yuv_frames(who, frames, fmt)
    n = len(dims)
    orientations = sj._orientation_list(who, n, orientations)
    sizes = _size_list(who, n, dims, sizes, box, orientations)
    if sizes is not None and len(sizes) != n:
        raise SjpegError(f"{who}: one size per frame")
    keep, caddr, per_frame = _colour_args(who, n, colour)
    eng = sj._engine_for(engine, dev)
    L = _lib()
    with torch.cuda.device(dev):
        cframes, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
        arr, oarr = sj._shape_arrays(who, n, sizes, orientations)
        need = L.sjpeg_hip_resize_ragged_yuv_bytes(fmt, n, cframes, sj._address(arr), sj._address(oarr))
        out = sj._made_out(who, planes, need, out)
        made, rfmt = (RaggedFrame * n)(), C.c_int(-1)
        # (a batch the library refuses has need == 0: the call below says why)
        eng._chk(L.sjpeg_hip_convert_ragged_yuv_src(eng._h, fmt, n, cframes, sj._address(arr), sj._address(oarr), caddr, per_frame,
                                                    out.data_ptr(), int(out.numel()) if need else 0, made, C.byref(rfmt), eng._stream()),
                 "sjpeg_hip_convert_ragged_yuv_src")
    return int(rfmt.value), sj._frame_views(out, made, rfmt.value), out


def make_video_sheets(frames, fmt=SRC_NV12, sheet=None, colour=VideoColour(), sizes=None, orientations=None, engine=None, out=None):
    """sjpeg_hip_sheet_ragged_yuv_colour_src: the uint8 contact sheets Engine.sheet_ragged makes of the frames, the
    thumbnails' rectangles converted from `colour` to JFIF's, the background as given.  Returns (out_fmt, sheets, buf):
    sheet s a tuple (y, u, v) of uint8 views into buf."""
    import torch
    who = "make_video_sheets"
    planes, dims, dev = sj._yuv_frames(who, frames, fmt)
    n = len(dims)
    orientations = sj._orientation_list(who, n, orientations)
    if sizes is not None and len(sizes) != n:
        raise SjpegError(f"{who}: one size per frame")
    keep, caddr, per_frame = _colour_args(who, n, colour)
    eng = sj._engine_for(engine, dev)
    L = _lib()
    with torch.cuda.device(dev):
        cframes, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
        st = sj._sheet_struct(who, sheet)
        arr, oarr = sj._shape_arrays(who, n, sizes, orientations)
        need = L.sjpeg_hip_sheet_ragged_bytes(fmt, n, cframes, C.addressof(st), sj._address(arr), sj._address(oarr))
        out = sj._made_out(who, planes, need, out)
        per = max(int(sheet.cols) * int(sheet.rows), 1)
        made = (RaggedFrame * max((n + per - 1) // per, 1))()
        ns, rfmt = C.c_int(0), C.c_int(-1)
        # (a batch the library refuses has need == 0: the call below says why)
        eng._chk(L.sjpeg_hip_sheet_ragged_yuv_colour_src(eng._h, fmt, n, cframes, C.addressof(st), sj._address(arr), sj._address(oarr), caddr,
                                                         per_frame, out.data_ptr(), int(out.numel()) if need else 0, made, C.byref(ns),
                                                         C.byref(rfmt), eng._stream()), "sjpeg_hip_sheet_ragged_yuv_colour_src")
    return int(rfmt.value), sj._frame_views(out, list(made)[:ns.value], rfmt.value), out


def encode_video_frames(frames, fmt=SRC_NV12, colour=VideoColour(), sizes=None, box=None, orientations=None, quality=75.0,
                        method=4, target_size=None, target_psnr=None, packed=False, metadata=None, engine=None):
    """The thumbnail call for decoded video WITH its colour put right: encode_yuv_frames' arguments plus colour, one
    VideoColour (default: BT.709, limited range) or one per frame -- what the SOURCE is (None: no conversion).  Every frame is resized, turned
    upright and converted to JFIF's full-range BT.601 inside the one ragged call; frame k's JPEG is byte for byte what
    encode_yuv_frames makes of the planes convert_yuv_frames returns.  VideoColour("bt601", "full") for every frame is
    exactly encode_yuv_frames.  Returns the JPEGs (list of bytes)."""
    import torch
    who = "encode_video_frames"
    planes, dims, dev = sj._yuv_frames(who, frames, fmt)
    n = len(dims)
    orientations = sj._orientation_list(who, n, orientations)
    sizes = _size_list(who, n, dims, sizes, box, orientations)
    keep, caddr, per_frame = _colour_args(who, n, colour)
    sj._one_target(who, target_size, target_psnr)
    search = sj._target_search(who, "frame", n, target_size, target_psnr)
    qs = sj._per_picture(quality, n)
    if len(qs) != n:
        raise SjpegError(f"{who}: one quality per frame")
    yuv_mode = YUV_444 if fmt == SRC_YUV444 else YUV_420
    eng = sj._engine_for(engine, dev)
    L = _lib()
    with torch.cuda.device(dev):
        call = eng._oriented_call(who, planes, dims, sizes, orientations, yuv_mode, sj._quality_quant(qs), method, None, 0x78, 12, 1,
                                  search, None, metadata)
        special = (call.sizes, call.orientations, caddr, per_frame)
        if packed:
            out, packed_capacity, meta = sj._packed_out(who, n, planes, call.capacities, None, None)
            eng._packed("sjpeg_hip_encode_ragged_yuv_converted_packed_src", fmt, planes, dims, call, special, out, packed_capacity, meta)
            eng.wait()
            return sj._fetch_packed(out, meta[:n], meta[n:], n, "frame")
        cframes, out, sizes_out, offsets = sj._ragged_frames(planes, dims, call.capacities, None, None, None)
        out, sz, offs = eng._unpacked("sjpeg_hip_encode_ragged_yuv_converted_src", fmt, cframes, call, special, out, sizes_out, offsets)[:3]
        eng.wait()                               # (pipelined mode: the output is complete after this)
        return sj._fetch_ragged(out, sz, offs)


def encode_video_sheets(frames, fmt=SRC_NV12, sheet=None, colour=VideoColour(), sizes=None, orientations=None, quality=75.0,
                        method=4, target_size=None, target_psnr=None, packed=False, metadata=None, engine=None):
    """encode_yuv_sheets WITH the colour put right: its arguments plus colour, one VideoColour or one per frame.  Only
    the thumbnails' rectangles are converted; the Sheet's background stays as given, (Y, U, V) in JFIF's colour.
    Returns (JPEGs, places) as encode_yuv_sheets."""
    import torch
    who = "encode_video_sheets"
    planes, dims, dev = sj._yuv_frames(who, frames, fmt)
    n = len(dims)
    orientations = sj._orientation_list(who, n, orientations)
    keep, caddr, per_frame = _colour_args(who, n, colour)
    eng = sj._engine_for(engine, dev)
    places = sj.sheet_places(sheet, dims, fmt, sizes, orientations)
    ns = places[-1][0] + 1
    qs = sj._per_picture(quality, ns)
    if len(qs) != ns:
        raise SjpegError(f"{who}: one quality per sheet")
    sj._one_target(who, target_size, target_psnr)
    search = sj._target_search(who, "sheet", ns, target_size, target_psnr)
    yuv_mode = YUV_444 if fmt == SRC_YUV444 else YUV_420
    L = _lib()
    with torch.cuda.device(dev):
        ns, call, special = eng._sheet_call(who, fmt, planes, dims, sheet, sizes, orientations, yuv_mode, sj._quality_quant(qs), int(method),
                                            None, 0x78, 12, 1, search, metadata)
        special += [caddr, per_frame]
        cframes, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
        if packed:
            out, packed_capacity, meta = sj._packed_out(who, ns, planes, call.capacities, None, None)
            eng._chk(L.sjpeg_hip_encode_ragged_sheet_yuv_colour_packed_src(
                eng._h, fmt, n, cframes, call.params, *special, *call.meta, out.data_ptr(), packed_capacity, meta.data_ptr() + 8 * ns,
                meta.data_ptr(), *call.results, eng._stream()), "sjpeg_hip_encode_ragged_sheet_yuv_colour_packed_src")
            eng.wait()
            return sj._fetch_packed(out, meta[:ns], meta[ns:], ns, "sheet"), places
        out_stride = (call.capacities[0] + 15) & ~15
        out = torch.empty(max(out_stride * ns, 1), dtype=torch.uint8, device=dev)
        sizes_out = torch.zeros(ns, dtype=torch.int64, device=dev)
        eng._chk(L.sjpeg_hip_encode_ragged_sheet_yuv_colour_src(
            eng._h, fmt, n, cframes, call.params, *special, *call.meta, out.data_ptr(), out_stride, sizes_out.data_ptr(), *call.results,
            eng._stream()), "sjpeg_hip_encode_ragged_sheet_yuv_colour_src")
        eng.wait()                               # (pipelined mode: the output is complete after this)
        return sj._fetch_ragged(out, sizes_out, [s * out_stride for s in range(ns)]), places
