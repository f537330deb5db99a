"""Decoded video with its colour put right inside the ragged call (sjpeg_hip.h, "video colour converted inside the
ragged call").  A JFIF file is full-range BT.601 YCbCr; a decoded H.264 or HEVC frame is mostly BT.709 and nearly always
studio range.  encode_yuv_frames / encode_yuv_sheets code the samples as they are; the calls here say what the SOURCE
is -- a VideoColour, one for all frames or one per frame -- and the library converts the made thumbnails, not the
sources, by one more launch behind the resize launch.  The arithmetic is exact and in integers: yuv_colour_samples is
the formula on single samples.

10-bit video: convert_deep_frames, encode_deep_video_frames, make_deep_video_sheets and encode_deep_video_sheets are
the same four calls on frames of 16-bit samples -- P010 as a GPU decoder writes HEVC Main10, AV1 10-bit and VP9
profile 2, yuv420p10le / 12le as a software decoder does -- described by a VideoDepth.  The resize kernel reads the
words, sums them exactly and rounds once into the 8-bit planes everything else works on; yuv16_samples is that formula
on single samples.  No BT.2020 matrix and no PQ / HLG tone mapping: HDR frames are coded by their code values."""
import ctypes as C

import numpy as np

import sjpeg_amd as sj
from sjpeg_amd import SRC_NV12, SRC_YUV444, YUV_420, YUV_444, SjpegError, lib

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


class _DepthStruct(C.Structure):
    """struct sjpeg_hip_yuv_depth"""
    _fields_ = [("bytes", C.c_uint8), ("shift", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class VideoDepth:
    """How the 16-bit samples of a deep frame carry their value: `bits` significant bits (8..16), align "msb" -- in the
    word's high bits, as P010 / P012 / P016 -- or "lsb" -- in its low bits, as yuv420p10le.  The library is told bytes
    = 2 and shift = the low bits of a word that lie below the made byte: 8 for "msb", bits - 8 for "lsb".
    VideoDepth.P010, .P016, .YUV10 and .YUV12 are the usual four."""

    def __init__(self, bits=10, align="msb"):
        if isinstance(bits, bool) or not isinstance(bits, int) or not 8 <= bits <= 16:
            raise SjpegError(f"VideoDepth: bits {bits!r} is not one of 8..16")
        if align not in ("msb", "lsb"):
            raise SjpegError(f"VideoDepth: align {align!r} is not 'msb' or 'lsb'")
        self.bits, self.align = bits, align
        self.bytes, self.shift = 2, 8 if align == "msb" else bits - 8

    def __eq__(self, other):
        return isinstance(other, VideoDepth) and (self.bits, self.align) == (other.bits, other.align)

    def __hash__(self):
        return hash((self.bits, self.align))

    def __repr__(self):
        return "VideoDepth(%d, %r)" % (self.bits, self.align)

    def _struct(self):
        return _DepthStruct(self.bytes, self.shift)


VideoDepth.P010, VideoDepth.P016 = VideoDepth(10, "msb"), VideoDepth(16, "msb")
VideoDepth.YUV10, VideoDepth.YUV12 = VideoDepth(10, "lsb"), VideoDepth(12, "lsb")

_lib = lib                               # (the one table of sjpeg_amd._binding binds every entry when the library loads)


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


def _deep_frames(who, frames, fmt):
    """sj._yuv_frames for frames of 16-bit samples: every plane a CUDA tensor of a 2-byte integer dtype (the bits are read
    as unsigned) [rows, samples] with stride 1 along a row; the UV plane of SRC_NV12 / SRC_NV21 may be [rows, pairs, 2]"""
    import torch
    frames = [tuple(fr) for fr in frames]
    if not frames:
        raise SjpegError(f"{who}: no frames")
    nplanes = 2 if fmt in (SRC_NV12, sj.SRC_NV21) else 3 if fmt in (sj.SRC_YUV420, SRC_YUV444) else 0
    if nplanes == 0:
        raise SjpegError(f"{who}: fmt {fmt} is not SRC_NV12, SRC_NV21, SRC_YUV420 or SRC_YUV444")
    for k, fr in enumerate(frames):
        if len(fr) != nplanes:
            raise SjpegError(f"{who}: frame {k} has {len(fr)} planes, the format takes {nplanes}")
        for i, p in enumerate(fr):
            ok = isinstance(p, torch.Tensor) and p.is_cuda and p.element_size() == 2 and not p.is_floating_point() and not p.is_complex()
            pair = ok and nplanes == 2 and i == 1 and p.dim() == 3 and p.shape[2] == 2 and p.stride(2) == 1 and p.stride(1) == 2
            if not ok or not (pair or (p.dim() == 2 and p.stride(1) == 1)):
                raise SjpegError(f"{who}: frame {k}: a plane is a CUDA tensor of a 2-byte integer dtype [rows, samples] with stride 1 along "
                                 "a row (the UV plane of a semi-planar format may be [rows, pairs, 2])")
    return [list(fr) for fr in frames], [(int(fr[0].shape[1]), int(fr[0].shape[0])) for fr in frames], frames[0][0].device


def _read_frames(who, frames, fmt, depth):
    """(planes, dims, device, the depth's struct or None, the `depth` segment of the C call where it has one) of a call's
    frames: bytes (depth None) or 16-bit samples"""
    if depth is None:
        return sj._yuv_frames(who, frames, fmt) + (None, {})
    if not isinstance(depth, VideoDepth):
        raise SjpegError(f"{who}: depth {depth!r} is not a VideoDepth")
    st = depth._struct()
    return _deep_frames(who, frames, fmt) + (st, {"depth": C.addressof(st)})


def yuv16_samples(words, depth=VideoDepth.P010):
    """sjpeg_hip_yuv16_samples: what a deep call makes of a sample at the frame's own size, host only: words, an array
    of a 2-byte integer dtype (the bits are read as unsigned), to uint8 of the same shape: min(255, (x + 2^(s-1)) >> s)."""
    who = "yuv16_samples"
    if not isinstance(depth, VideoDepth):
        raise SjpegError(f"{who}: depth {depth!r} is not a VideoDepth")
    src = np.ascontiguousarray(words)
    if src.dtype.kind not in "iu" or src.dtype.itemsize != 2:
        raise SjpegError(f"{who}: words is an array of a 2-byte integer dtype")
    src = src.view(np.uint16)
    out = np.empty(src.shape, np.uint8)
    st = depth._struct()
    if _lib().sjpeg_hip_yuv16_samples(C.addressof(st), src.size, src.ctypes.data, out.ctypes.data) != 0:
        raise SjpegError(f"sjpeg_hip_yuv16_samples failed: {sj.last_error()}")
    return out


def convert_yuv_frames(frames, fmt=SRC_NV12, colour=VideoColour(), sizes=None, box=None, orientations=None, engine=None, out=None):
    """sjpeg_hip_convert_ragged_yuv_src: the planes Engine.resize_ragged_yuv makes of the frames (frames, fmt, sizes /
    box, orientations as encode_video_frames), converted from `colour` to JFIF's in place by one more launch.  Returns
    (out_fmt, pictures, buf) as resize_ragged_yuv: picture k a tuple (y, u, v) of uint8 views into buf, which any ragged
    entry takes as SRC_YUV420 / SRC_YUV444 planes.  Asynchronous on the current torch stream."""
    return _convert("convert_yuv_frames", frames, fmt, colour, sizes, box, orientations, engine, out, None)


def convert_deep_frames(frames, fmt=SRC_NV12, colour=VideoColour(), sizes=None, box=None, orientations=None, engine=None, out=None,
                        depth=VideoDepth.P010):
    """sjpeg_hip_convert_ragged_yuv16_src: convert_yuv_frames of frames of 16-bit samples (depth: a VideoDepth) -- planes
    of any 2-byte integer dtype, the UV plane of P010 [rows, pairs, 2] or [rows, 2 * pairs].  The made planes are uint8:
    every sample the exact area average of the words, divided by 2^shift and rounded half up once, clamped to 255; then
    converted from `colour` (None: not at all).  Every frame goes through the kernel, at its own size too."""
    return _convert("convert_deep_frames", frames, fmt, colour, sizes, box, orientations, engine, out, depth)


def _convert(who, frames, fmt, colour, sizes, box, orientations, engine, out, depth):
    import torch
    planes, dims, dev, dkeep, deep = _read_frames(who, frames, fmt, depth)
    stem = "convert_ragged_yuv16" if deep else "convert_ragged_yuv"
    n = len(dims)
    orientations = sj._orientation_list(who, n, orientations)
    sizes = _size_list(who, n, dims, sizes, box, orientations)
    if sizes is not None and len(sizes) != n:
        raise SjpegError(f"{who}: one size per frame")
    keep, caddr, per_frame = _colour_args(who, n, colour)
    eng = sj._engine_for(engine, dev)
    with torch.cuda.device(dev):
        cframes, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
        arr, oarr = sj._shape_arrays(who, n, sizes, orientations)
        return eng._make_pictures(who, stem, "resize_ragged_yuv", fmt, planes, cframes, {"sizes": sj._address(arr), "orientations": sj._address(oarr)},
                                  dict(deep, colour=(caddr, per_frame)), out)


def make_video_sheets(frames, fmt=SRC_NV12, sheet=None, colour=VideoColour(), sizes=None, orientations=None, engine=None, out=None):
    """sjpeg_hip_sheet_ragged_yuv_colour_src: the uint8 contact sheets Engine.sheet_ragged makes of the frames, the
    thumbnails' rectangles converted from `colour` to JFIF's, the background as given.  Returns (out_fmt, sheets, buf):
    sheet s a tuple (y, u, v) of uint8 views into buf."""
    return _make_sheets("make_video_sheets", frames, fmt, sheet, colour, sizes, orientations, engine, out, None)


def make_deep_video_sheets(frames, fmt=SRC_NV12, sheet=None, colour=VideoColour(), sizes=None, orientations=None, engine=None, out=None,
                           depth=VideoDepth.P010):
    """sjpeg_hip_sheet_ragged_yuv16_src: make_video_sheets of frames of 16-bit samples, as convert_deep_frames reads them."""
    return _make_sheets("make_deep_video_sheets", frames, fmt, sheet, colour, sizes, orientations, engine, out, depth)


def _make_sheets(who, frames, fmt, sheet, colour, sizes, orientations, engine, out, depth):
    import torch
    planes, dims, dev, dkeep, deep = _read_frames(who, frames, fmt, depth)
    stem = "sheet_ragged_yuv16" if deep else "sheet_ragged_yuv_colour"
    n = len(dims)
    orientations = sj._orientation_list(who, n, orientations)
    if sizes is not None and len(sizes) != n:
        raise SjpegError(f"{who}: one size per frame")
    keep, caddr, per_frame = _colour_args(who, n, colour)
    eng = sj._engine_for(engine, dev)
    with torch.cuda.device(dev):
        cframes, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
        shape, nsheets, skeep = sj._sheet_shape(who, n, sheet, sizes, orientations)
        return eng._make_pictures(who, stem, "sheet_ragged", fmt, planes, cframes, shape, dict(deep, colour=(caddr, per_frame)), out, nsheets)


def encode_video_frames(frames, fmt=SRC_NV12, colour=VideoColour(), sizes=None, box=None, orientations=None, quality=75.0,
                        method=4, target_size=None, target_psnr=None, packed=False, metadata=None, engine=None):
    """The thumbnail call for decoded video WITH its colour put right: encode_yuv_frames' arguments plus colour, one
    VideoColour (default: BT.709, limited range) or one per frame -- what the SOURCE is (None: no conversion).  Every frame is resized, turned
    upright and converted to JFIF's full-range BT.601 inside the one ragged call; frame k's JPEG is byte for byte what
    encode_yuv_frames makes of the planes convert_yuv_frames returns.  VideoColour("bt601", "full") for every frame is
    exactly encode_yuv_frames.  Returns the JPEGs (list of bytes)."""
    return _encode_frames("encode_video_frames", frames, fmt, colour, sizes, box, orientations, quality, method, target_size, target_psnr,
                          packed, metadata, engine, None)


def encode_deep_video_frames(frames, fmt=SRC_NV12, colour=VideoColour(), sizes=None, box=None, orientations=None, quality=75.0,
                             method=4, target_size=None, target_psnr=None, packed=False, metadata=None, engine=None,
                             depth=VideoDepth.P010):
    """The thumbnail call for 10-bit video: encode_video_frames of frames of 16-bit samples as the decoder wrote them
    (depth: a VideoDepth; planes as convert_deep_frames takes them), with no narrowing pass in front.  Frame k's JPEG is
    byte for byte what encode_yuv_frames makes of the planes convert_deep_frames returns.  colour None: no conversion."""
    return _encode_frames("encode_deep_video_frames", frames, fmt, colour, sizes, box, orientations, quality, method, target_size,
                          target_psnr, packed, metadata, engine, depth)


def _encode_frames(who, frames, fmt, colour, sizes, box, orientations, quality, method, target_size, target_psnr, packed, metadata, engine,
                   depth):
    import torch
    planes, dims, dev, dkeep, deep = _read_frames(who, frames, fmt, depth)
    stem = "yuv16" if deep else "yuv_converted"
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
    with torch.cuda.device(dev):
        call = eng._oriented_call(who, planes, dims, sizes, orientations, yuv_mode, sj._quality_quant(qs), method, None, 0x78, 12, 1,
                                  search, None, metadata)
        res = eng._encode_shaped(who, stem, fmt, planes, dims, call,
                                 dict(deep, sizes=call.sizes, orientations=call.orientations, colour=(caddr, per_frame)), packed)
        eng.wait()                               # (pipelined mode: the output is complete after this)
        return sj._fetch_packed(res[0], res[1], res[2], n, "frame") if packed else sj._fetch_ragged(res[0], res[1], res[2])


def encode_video_sheets(frames, fmt=SRC_NV12, sheet=None, colour=VideoColour(), sizes=None, orientations=None, quality=75.0,
                        method=4, target_size=None, target_psnr=None, packed=False, metadata=None, engine=None):
    """encode_yuv_sheets WITH the colour put right: its arguments plus colour, one VideoColour or one per frame.  Only
    the thumbnails' rectangles are converted; the Sheet's background stays as given, (Y, U, V) in JFIF's colour.
    Returns (JPEGs, places) as encode_yuv_sheets."""
    return _encode_sheets("encode_video_sheets", frames, fmt, sheet, colour, sizes, orientations, quality, method, target_size, target_psnr,
                          packed, metadata, engine, None)


def encode_deep_video_sheets(frames, fmt=SRC_NV12, sheet=None, colour=VideoColour(), sizes=None, orientations=None, quality=75.0,
                             method=4, target_size=None, target_psnr=None, packed=False, metadata=None, engine=None,
                             depth=VideoDepth.P010):
    """encode_video_sheets of frames of 16-bit samples, as encode_deep_video_frames reads them."""
    return _encode_sheets("encode_deep_video_sheets", frames, fmt, sheet, colour, sizes, orientations, quality, method, target_size,
                          target_psnr, packed, metadata, engine, depth)


def _encode_sheets(who, frames, fmt, sheet, colour, sizes, orientations, quality, method, target_size, target_psnr, packed, metadata, engine,
                   depth):
    import torch
    planes, dims, dev, dkeep, deep = _read_frames(who, frames, fmt, depth)
    stem = "sheet_yuv16" if deep else "sheet_yuv_colour"
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
    with torch.cuda.device(dev):
        ns, call, segments = eng._sheet_call(who, fmt, planes, dims, sheet, sizes, orientations, yuv_mode, sj._quality_quant(qs), int(method),
                                             None, 0x78, 12, 1, search, metadata)
        res = eng._encode_sheets_shaped(who, stem, fmt, planes, dims, ns, call, dict(segments, **deep, colour=(caddr, per_frame)), packed)
        eng.wait()                               # (pipelined mode: the output is complete after this)
        jpegs = sj._fetch_packed(res[0], res[1], res[2], ns, "sheet") if packed else sj._fetch_ragged(res[0], res[1], res[2])
    return jpegs, places
