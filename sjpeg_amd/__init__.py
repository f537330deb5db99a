"""sjpeg_amd -- Python binding (ctypes) of the MI355X-native sjpeg-compatible JPEG encoder.

The product is the C/C++ library ``sjpeg_amd/csrc/libsjpeg_amd.so`` (public API
``include/sjpeg.h``, device C-ABI ``include/sjpeg_hip.h``).  This module only binds those
symbols -- it contains no encoder logic and no CPU fallback: if the shared library is not
built, importing the binding raises; if no gfx950 device is present, every encode call fails.

torch is used (optionally) for device memory and streams only.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("SJPEG_AMD_LIB") or os.path.join(CSRC, "libsjpeg_amd.so")   # (override: A/B builds in tools/)

YUV_AUTO, YUV_420, YUV_SHARP, YUV_444, YUV_400 = range(5)

_u8p = C.POINTER(C.c_uint8)


class ScanTables(C.Structure):
    """struct sjpeg_hip_scan_tables (include/sjpeg_hip.h)."""
    _fields_ = [("iquant", (C.c_uint16 * 64) * 2),
                ("bias", (C.c_uint16 * 64) * 2),
                ("dc_codes", (C.c_uint32 * 12) * 2),
                ("ac_codes", (C.c_uint32 * 256) * 2),
                ("quant", (C.c_uint8 * 64) * 2),
                ("trellis_len", (C.c_uint8 * 256) * 2),
                ("flags", C.c_uint32)]


QUANT_TRELLIS = 1
QUANT_KEEP = 2
QUANT_REPLAY = 4
RESTART_MARKERS = 8      # optional restart-marker mode (sjpeg_hip.h): not the reference's bytes, the same pixels


SRC_RGB, SRC_BGRA, SRC_RGBA, SRC_GRAY, SRC_YUV444, SRC_YUV420, SRC_NV12, SRC_NV21 = range(8)
SRC_RGB_PLANAR = 8       # R, G and B planes of one pitch (channel-first pictures): sjpeg_hip.h
# ... and the same planes of float elements, turned into bytes by the engine's pixel transform as they are read
SRC_RGB_PLANAR_F32, SRC_RGB_PLANAR_F16, SRC_RGB_PLANAR_BF16 = 9, 10, 11
# ONE plane of float elements: interleaved pixels of 3 (R, G, B) or 4 elements (R, G, B and one that is never read) --
# channels-last tensors, [H, W, 3] and [H, W, 4] float arrays --, and gray pictures ([1, H, W], [H, W]; YUV_400)
SRC_RGB_F32, SRC_RGB_F16, SRC_RGB_BF16 = 12, 13, 14
SRC_RGBA_F32, SRC_RGBA_F16, SRC_RGBA_BF16 = 15, 16, 17
SRC_GRAY_F32, SRC_GRAY_F16, SRC_GRAY_BF16 = 18, 19, 20
# What a format is, once (the library's table: sjpeg_amd/csrc/source_layout.h) -- format: (planes read, elements from a
# pixel to the next, how many of them are read, the elements' torch dtype by name or None for bytes, the yuv_mode the
# format implies or None, the name layout="chw" pictures of that memory layout go by or None)
_FORMATS = {SRC_RGB: (1, 3, 3, None, None, "rgb"), SRC_BGRA: (1, 4, 4, None, None, None), SRC_RGBA: (1, 4, 4, None, None, "rgba"),
            SRC_GRAY: (1, 1, 1, None, YUV_400, None), SRC_YUV444: (3, 1, 1, None, YUV_444, None), SRC_YUV420: (3, 1, 1, None, YUV_420, None),
            SRC_NV12: (2, 1, 1, None, YUV_420, None), SRC_NV21: (2, 1, 1, None, YUV_420, None), SRC_RGB_PLANAR: (3, 1, 1, None, None, "planar")}
for _k, _dt in enumerate(("float32", "float16", "bfloat16")):
    _FORMATS.update({(SRC_RGB_PLANAR_F32, SRC_RGB_PLANAR_F16, SRC_RGB_PLANAR_BF16)[_k]: (3, 1, 1, _dt, None, "planar"),
                     (SRC_RGB_F32, SRC_RGB_F16, SRC_RGB_BF16)[_k]: (1, 3, 3, _dt, None, "rgb"),
                     (SRC_RGBA_F32, SRC_RGBA_F16, SRC_RGBA_BF16)[_k]: (1, 4, 3, _dt, None, "rgba"),
                     (SRC_GRAY_F32, SRC_GRAY_F16, SRC_GRAY_BF16)[_k]: (1, 1, 1, _dt, YUV_400, "gray")})
_DTYPE_BYTES = {"float32": 4, "float16": 2, "bfloat16": 2}
_PLANAR_RGB = tuple(f for f, row in _FORMATS.items() if row[5] == "planar")
_FLOAT_ELEMENT_BYTES = {f: _DTYPE_BYTES[row[3]] for f, row in _FORMATS.items() if row[3] is not None}
_GRAY_FLOAT = tuple(f for f, row in _FORMATS.items() if row[5] == "gray")
_IMPLIED_MODE = {f: row[4] for f, row in _FORMATS.items() if row[4] is not None}
# (chw name, dtype name or None) -> format
_CHW_FORMAT = {(row[5], row[3]): f for f, row in _FORMATS.items() if row[5] is not None}


class Source(C.Structure):
    """struct sjpeg_hip_source (include/sjpeg_hip.h)."""
    _fields_ = [("format", C.c_int32), ("reserved", C.c_int32), ("plane", C.c_void_p * 3),
                ("row_stride", C.c_int64 * 3), ("frame_stride", C.c_int64 * 3)]


def sharp_yuv(fmt, frames):
    """SJPEG_YUV_SHARP conversion of device-resident packed frames [F, H, row_bytes] (fmt = SRC_RGB /
    SRC_BGRA / SRC_RGBA) -> (y [F, H, W], u [F, ch, cw], v [F, ch, cw]) uint8 CUDA tensors."""
    import torch
    assert frames.is_cuda and frames.dim() == 3
    f, h, row_bytes = frames.shape
    bpp = _FORMATS[fmt][1]
    w = row_bytes // bpp
    cw, ch = (w + 1) // 2, (h + 1) // 2
    src, _ = make_source(fmt, [frames])
    y = torch.empty((f, h, w), dtype=torch.uint8, device=frames.device)
    u = torch.empty((f, ch, cw), dtype=torch.uint8, device=frames.device)
    v = torch.empty((f, ch, cw), dtype=torch.uint8, device=frames.device)
    L = lib()
    wsz = L.sjpeg_hip_sharp_workspace(w, h, f)
    work = torch.empty(max(wsz, 16), dtype=torch.uint8, device=frames.device)
    rc = L.sjpeg_hip_sharp_yuv(C.byref(src), w, h, f, y.data_ptr(), u.data_ptr(), v.data_ptr(), h * w, ch * cw,
                               work.data_ptr(), wsz, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise SjpegError("sjpeg_hip_sharp_yuv failed (%d)" % rc)
    return y, u, v


def segment_count(w, h, yuv_mode):
    n = lib().sjpeg_hip_segment_count(w, h, yuv_mode)
    if n <= 0:
        raise SjpegError("sjpeg_hip_segment_count: " + lib().sjpeg_hip_last_error().decode())
    return n


def band_bound(w, h, yuv_mode, seg_begin, seg_end):
    n = lib().sjpeg_hip_band_bound(w, h, yuv_mode, seg_begin, seg_end)
    if n == 0:
        raise SjpegError("sjpeg_hip_band_bound: bad arguments")
    return n


def make_source(fmt, planes):
    """planes: CUDA uint8 tensors [F, rows, row_bytes] (one per plane of the layout).
    Returns (Source, nframes); the tensors must outlive the calls that use it.
    SRC_RGB_PLANAR_F32 / _F16 / _BF16: planes = (R, G, B) as for SRC_RGB_PLANAR, of torch.float32 / float16 / bfloat16;
    the strides go in as bytes, and the engine's pixel transform (Engine.set_pixel_transform) makes the bytes.
    SRC_RGB_F* / SRC_RGBA_F* / SRC_GRAY_F*: one plane [F, H, W * step] of the float dtype (step 3, 4 or 1 elements a
    pixel), stride(2) == 1; the strides go in as bytes.
    SRC_RGB_PLANAR: planes = (R, G, B), the [N, H, W] views x[:, 0], x[:, 1], x[:, 2] of an [N, 3, H, W] tensor (or of
    any crop of one): the three share their row and frame strides.
    With that layout a dimension of size 1 is never stepped over, so whatever stride torch reports for it is not looked
    at: a one-pixel-wide plane passes with any stride(2), and a one-row plane is handed over with its width as the row
    stride (the views of a 1 x 1 batch made from a transposed array report such strides).  The other layouts are
    checked and handed over as they always were."""
    s = Source()
    s.format = fmt
    planar = fmt in _PLANAR_RGB
    esz = _FLOAT_ELEMENT_BYTES.get(fmt, 1)
    for i, t in enumerate(planes):
        assert t.is_cuda and t.dim() == 3 and (t.stride(2) == 1 or (planar and t.shape[2] == 1))
        assert esz == 1 or t.dtype == _float_dtypes()[fmt]
        s.plane[i] = t.data_ptr()
        s.row_stride[i] = (t.shape[2] if planar and t.shape[1] == 1 else t.stride(1)) * esz
        s.frame_stride[i] = t.stride(0) * esz
    return s, planes[0].shape[0]


def _float_dtypes():
    import torch
    return {f: getattr(torch, _FORMATS[f][3]) for f in _FLOAT_ELEMENT_BYTES}


def _three(who, what, v):
    """v as three floats: one value for the three channels alike, or a sequence of three (R, G, B)"""
    vs = [v] * 3 if isinstance(v, (int, float, np.floating, np.integer)) else list(v)
    if len(vs) != 3:
        raise SjpegError(f"{who}: {what} is one value or a sequence of three (R, G, B), not of {len(vs)}")
    vs = [float(x) for x in vs]
    if not all(np.isfinite(x) for x in vs):
        raise SjpegError(f"{who}: scale and bias must be finite" if what in ("scale", "bias") else f"{who}: {what} must be finite")
    return tuple(vs)


class FloatPixels:
    """Float pictures for the calls that take layout="chw" (encode_images, compress_images, riskiness_images) and for
    encode_images_full_chw, as their `images`: a sequence of CUDA tensors [3, H_k, W_k] of ONE dtype -- torch.float32,
    float16 or bfloat16 --, any row stride.  The pictures are LOGICALLY channel-first; their strides choose the format,
    one per call:
      stride(2) == 1                           planes (SRC_RGB_PLANAR_F32 / _F16 / _BF16): a contiguous [3, H, W]
      stride(0) == 1, stride(2) == 3 or 4      interleaved (SRC_RGB_F* / SRC_RGBA_F*): a slice of a channels_last
                                               batch, hwc.permute(2, 0, 1), rgba.permute(2, 0, 1)[:3]
      [1, H, W] or [H, W], stride(-1) == 1     gray (SRC_GRAY_F*): YUV_400 only
    A sample x of channel c is coded as the byte rint(clamp(fma(x, scale[c], bias[c]), 0, 255)) (ties to even, NaN ->
    0): scale 255, bias 0 for values in 0..1, 127.5 and 127.5 for -1..1; scale and bias are one value each or three
    (R, G, B; gray uses the first) -- FloatPixels.normalized makes them from a mean and a std.  The conversion happens
    inside the encoder's loader -- no uint8 copy of the batch is made, no .contiguous() --, and the JPEGs are those of
    the uint8 pictures so defined.  The call sets the engine's pixel transform (it stays set)."""

    def __init__(self, images, scale=255.0, bias=0.0):
        self.images = list(images)
        self.scale3, self.bias3 = _three("FloatPixels", "scale", scale), _three("FloatPixels", "bias", bias)
        # (one value given: one value kept, as ever)
        self.scale = self.scale3[0] if self.scale3 == (self.scale3[0],) * 3 else self.scale3
        self.bias = self.bias3[0] if self.bias3 == (self.bias3[0],) * 3 else self.bias3

    @classmethod
    def normalized(cls, images, mean, std):
        """Pictures normalised as (u8 / 255 - mean[c]) / std[c], the way classification pipelines store them: coded
        with scale[c] = 255 * std[c] and bias[c] = 255 * mean[c], computed in float64 and rounded once to float32.
        mean and std: one value each, or three."""
        mean, std = _three("FloatPixels.normalized", "mean", mean), _three("FloatPixels.normalized", "std", std)
        return cls(images, [float(np.float32(255.0 * s)) for s in std], [float(np.float32(255.0 * m)) for m in mean])


def _float_pixels(who, images, chw):
    """(the images of a call, its FloatPixels or None)"""
    if not isinstance(images, FloatPixels):
        return images, None
    if not chw:
        raise SjpegError(f"{who}: FloatPixels are channel-first pictures [3, H, W]: pass layout='chw'")
    return images.images, images


REDUCE_MAX = 8                   # SJPEG_HIP_REDUCE_MAX


def _per_picture(value, n):
    """one value for all n pictures, or one per picture: the list"""
    return list(value) if isinstance(value, (list, tuple, np.ndarray)) else [value] * n


def _wrapper_of(images):
    """the name of the wrapper the images of a call are in already -- Reduced, Resized, Oriented, Flattened --, or None"""
    return next((c.__name__ for c in (Reduced, Resized, Oriented, Flattened) if isinstance(images, c)), None)


def _wrapped(images):
    """The opening the wrapper classes share: (what a wrapper keeps as its images -- a FloatPixels as it is, anything
    else as a list --, the inner list of pictures, their number)"""
    inner = images.images if isinstance(images, FloatPixels) else list(images)
    return (images if isinstance(images, FloatPixels) else inner), inner, len(inner)


class Reduced:
    """Pictures to be coded at 1/factor of their size -- thumbnails, the levels of a srcset or DeepZoom pyramid, dataset
    previews -- as the `images` of encode_images, compress_images, encode_images_full, encode_images_full_chw and
    encode_images_full_meta: Reduced(images, factor) with `images` what those calls take (a sequence of CUDA tensors, or
    a FloatPixels with layout="chw") and `factor` one int in 1..8 or one per picture.  Picture k becomes
    (W + s - 1) // s by (H + s - 1) // s: every sample the average of an s x s box of the bytes the encoder sees today
    (float pictures: after the pixel transform), rounded half up, the last column and row replicated at the edges -- one
    launch of the reduce kernel for the whole batch, no torch call and no float intermediate per picture -- and its JPEG
    is byte for byte that of the uint8 picture so defined (reduce_images returns those).  Everything else of the call
    -- layout, packed, metadata, targets, the trellis, YUV_AUTO -- works on the reduced pictures.  Factors that are all 1
    change nothing.  A pyramid is the same picture listed several times: Reduced([im] * 4, [1, 2, 4, 8])."""

    def __init__(self, images, factor):
        already = _wrapper_of(images)
        if already == "Resized":
            raise SjpegError("Reduced: the pictures are Resized already: resize the pictures themselves, once")
        if already in ("Oriented", "Flattened"):
            raise SjpegError(f"Reduced: the pictures are {already} already: {already} takes the sizes itself")
        self.images, _, n = _wrapped(images)
        fs = _per_picture(factor, n)
        if len(fs) != n:
            raise SjpegError(f"Reduced: {len(fs)} factors for {n} pictures: one factor, or one per picture")
        for k, f in enumerate(fs):
            if not isinstance(f, (int, np.integer)) or f < 1 or f > REDUCE_MAX:
                raise SjpegError(f"Reduced: picture {k}: factor {f!r} is not an int in 1..{REDUCE_MAX}")
        self.factors = [int(f) for f in fs]


def _reduced(images):
    """(the images of a call without their Reduced wrapper, the factors or None when there is nothing to reduce)"""
    if not isinstance(images, Reduced):
        return images, None
    return images.images, (images.factors if any(f != 1 for f in images.factors) else None)


def reduced_size(w, h, factor):
    """sjpeg_hip_reduced_size: (w', h') of a w x h picture reduced by factor (1..8)."""
    rw, rh = C.c_int(0), C.c_int(0)
    if lib().sjpeg_hip_reduced_size(int(w), int(h), int(factor), C.byref(rw), C.byref(rh)) != 0:
        raise SjpegError("sjpeg_hip_reduced_size: " + lib().sjpeg_hip_last_error().decode())
    return int(rw.value), int(rh.value)


def fit_size(w, h, box):
    """sjpeg_hip_fit_size: the size of a w x h picture fitted into box = (bw, bh) with its shape kept, in integers; a
    picture that fits already keeps its size (never larger)."""
    try:
        bw, bh = box
    except (TypeError, ValueError):
        raise SjpegError(f"fit_size: box {box!r} is not a pair (width, height)")
    fw, fh = C.c_int(0), C.c_int(0)
    if lib().sjpeg_hip_fit_size(int(w), int(h), int(bw), int(bh), C.byref(fw), C.byref(fh)) != 0:
        raise SjpegError("sjpeg_hip_fit_size: " + lib().sjpeg_hip_last_error().decode())
    return int(fw.value), int(fh.value)


def _picture_size(im, chw):
    """(w, h) of a picture as a call with this layout reads its shape (gray float pictures: [H, W])"""
    shape = tuple(getattr(im, "shape", ()))
    if len(shape) == 2:
        return int(shape[1]), int(shape[0])
    if len(shape) != 3:
        raise SjpegError("Resized.fit: a picture is a tensor [H, W, 3], [3, H, W] or [H, W]")
    return (int(shape[2]), int(shape[1])) if chw else (int(shape[1]), int(shape[0]))


class Resized:
    """Pictures to be coded at a size of the caller's choice, each side at most the source's -- thumbnails that fit a
    box, "320 wide", "the longer side 1024" -- wherever Reduced is taken: Resized(images, sizes) with `images` what
    encode_images, compress_images, encode_images_full, encode_images_full_chw and encode_images_full_meta take and
    `sizes` one (w, h) or one per picture.  Picture k becomes w x h: every sample the exact area average of the bytes
    the encoder sees today (float pictures: after the pixel transform), in integers, rounded half up -- one launch of
    the resize kernel for the whole batch, no torch call and no float intermediate per picture -- and its JPEG is byte
    for byte that of the uint8 picture so defined (resize_images returns those).  Sizes equal to the pictures' own
    change nothing.  Resized.fit(images, box) fits every picture into one box."""

    def __init__(self, images, sizes):
        self._refuse_wrapped(images)
        self.images, _, n = _wrapped(images)
        one = isinstance(sizes, (list, tuple, np.ndarray)) and len(sizes) == 2 and \
            all(isinstance(v, (int, np.integer)) for v in sizes)
        ss = [tuple(sizes)] * n if one else list(sizes) if isinstance(sizes, (list, tuple, np.ndarray)) else None
        if ss is None or len(ss) != n:
            raise SjpegError(f"Resized: sizes for {n} pictures: one (w, h), or one per picture")
        self.sizes = []
        for k, wh in enumerate(ss):
            if not isinstance(wh, (list, tuple, np.ndarray)) or len(wh) != 2 or \
                    not all(isinstance(v, (int, np.integer)) and 1 <= v <= 65535 for v in wh):
                raise SjpegError(f"Resized: picture {k}: size {wh!r} is not a pair of ints (w, h) in 1..65535")
            self.sizes.append((int(wh[0]), int(wh[1])))

    @staticmethod
    def _refuse_wrapped(images):
        already = _wrapper_of(images)
        if already in ("Reduced", "Resized"):
            raise SjpegError("Resized: the pictures are Reduced or Resized already: resize the pictures themselves, once")
        if already is not None:
            raise SjpegError(f"Resized: the pictures are {already} already: {already} takes the sizes itself")

    @classmethod
    def fit(cls, images, box, layout="hwc"):
        """Resized(images, sizes) with every picture fitted into box = (bw, bh) by fit_size; layout says how the
        pictures' shapes are read ("hwc": [H, W, 3]; "chw": [3, H, W]; a FloatPixels is read as "chw")."""
        cls._refuse_wrapped(images)
        chw = isinstance(images, FloatPixels) or _check_layout("Resized.fit", layout)
        return cls(images, [fit_size(*_picture_size(im, chw), box) for im in _wrapped(images)[1]])


def _resized(images):
    """(the images of a call without their Resized wrapper, the sizes or None for pictures that are not Resized)"""
    if not isinstance(images, Resized):
        return images, None
    return images.images, images.sizes


def _sizes_array(who, sizes):
    """sizes as the C entries take them: int32 [n][2], values clamped into int32 (the library names a bad one)"""
    try:
        arr = np.asarray([[int(w), int(h)] for (w, h) in sizes], dtype=np.int64).reshape(len(sizes), 2)
    except (TypeError, ValueError):
        raise SjpegError(f"{who}: sizes are pairs of ints (w, h), one per frame")
    return np.ascontiguousarray(np.clip(arr, -2**31, 2**31 - 1).astype(np.int32))


def oriented_size(w, h, orientation):
    """sjpeg_hip_oriented_size: (w, h) of the upright picture of a stored w x h one with EXIF orientation 1..8: swapped
    for 5..8."""
    ow, oh = C.c_int(0), C.c_int(0)
    if lib().sjpeg_hip_oriented_size(int(w), int(h), int(orientation), C.byref(ow), C.byref(oh)) != 0:
        raise SjpegError("sjpeg_hip_oriented_size: " + lib().sjpeg_hip_last_error().decode())
    return int(ow.value), int(oh.value)


def yuv_plane_size(fmt, w, h, plane):
    """sjpeg_hip_yuv_plane_size: (w, h) of plane 0..2 (Y, U, V) of a w x h picture in SRC_YUV444, SRC_YUV420, SRC_NV12
    or SRC_NV21, as the encoder reads it: the chroma planes of the 4:2:0 formats are (w + 1) // 2 by (h + 1) // 2."""
    pw, ph = C.c_int(0), C.c_int(0)
    if lib().sjpeg_hip_yuv_plane_size(int(fmt), int(w), int(h), int(plane), C.byref(pw), C.byref(ph)) != 0:
        raise SjpegError("sjpeg_hip_yuv_plane_size: " + lib().sjpeg_hip_last_error().decode())
    return int(pw.value), int(ph.value)


def exif_orientation(exif) -> int:
    """sjpeg_hip_exif_orientation: 1..8 from IFD0 tag 0x0112 of an EXIF payload as PictureMetadata.exif holds it (a
    leading b"Exif\\0\\0" is skipped; both byte orders); 0 for anything else -- no tag, not one SHORT, a value outside
    1..8, truncated or malformed bytes."""
    b = bytes(exif)
    return int(lib().sjpeg_hip_exif_orientation(b, len(b)))


def exif_reset_orientation(exif) -> bytes:
    """sjpeg_hip_exif_reset_orientation on a copy: the payload with its Orientation set to 1 (unchanged where
    exif_orientation is 0) -- for pictures whose rotation is baked in and whose EXIF is kept."""
    b = bytes(exif)
    if not b:
        return b
    buf = (C.c_uint8 * len(b)).from_buffer_copy(b)
    lib().sjpeg_hip_exif_reset_orientation(buf, len(b))
    return bytes(buf)


class Oriented:
    """Pictures to be coded upright -- and, with `sizes`, resized in the same launch -- wherever Resized is taken:
    Oriented(images, orientations, sizes=None) with `images` what encode_images, compress_images, encode_images_full,
    encode_images_full_chw and encode_images_full_meta take, `orientations` one EXIF Orientation (tag 0x0112, 1..8) or
    one per picture, and `sizes` None (every picture at its own size), one (w, h) or one per picture, in the STORED
    orientation as Resized takes them.  Picture k is resized as Resized defines it and every finished tile stored where
    it lands in the upright picture (w x h for 1..4, h x w for 5..8): one launch for the batch, no rot90 / flip /
    contiguous() per picture, and its JPEG is byte for byte that of the upright uint8 picture (orient_images returns
    those).  Orientations that are all 1 are Resized(images, sizes)."""

    def __init__(self, images, orientations, sizes=None):
        already = _wrapper_of(images)
        if already == "Flattened":
            raise SjpegError("Oriented: the pictures are Flattened already: Flattened takes the orientations and the sizes itself")
        if already is not None:
            raise SjpegError("Oriented: the pictures are Reduced, Resized or Oriented already: Oriented takes the sizes itself, once")
        self.images, _, n = _wrapped(images)
        os_ = _per_picture(orientations, n)
        if len(os_) != n:
            raise SjpegError(f"Oriented: {len(os_)} orientations for {n} pictures: one orientation, or one per picture")
        for k, o in enumerate(os_):
            if not isinstance(o, (int, np.integer)) or o < 1 or o > 8:
                raise SjpegError(f"Oriented: picture {k}: orientation {o!r} is not an int in 1..8 (EXIF tag 0x0112)")
        self.orientations = [int(o) for o in os_]
        self.sizes = None if sizes is None else Resized(images, sizes).sizes

    @classmethod
    def fit(cls, images, orientations, box, layout="hwc"):
        """Oriented(images, orientations, sizes) with every UPRIGHT picture fitted into box = (bw, bh) by fit_size: for
        the orientations 5..8 the stored picture is fitted into (bh, bw).  layout as Resized.fit."""
        plain = cls(images, orientations)
        chw = isinstance(images, FloatPixels) or _check_layout("Oriented.fit", layout)
        try:
            bw, bh = box
        except (TypeError, ValueError):
            raise SjpegError(f"fit_size: box {box!r} is not a pair (width, height)")
        sizes = [fit_size(*_picture_size(im, chw), (bh, bw) if o >= 5 else (bw, bh))
                 for im, o in zip(_wrapped(images)[1], plain.orientations)]
        return cls(images, plain.orientations, sizes)

    @classmethod
    def from_metadata(cls, images, metadata, box=None, layout="hwc"):
        """(Oriented, metadata): every picture's orientation read from its PictureMetadata.exif (exif_orientation; 0 --
        no tag, no EXIF, no entry -- is taken as 1), the pictures fitted into `box` as Oriented.fit does when one is
        given; the metadata returned are copies whose Orientation is reset to 1, to be handed to the encode with the
        Oriented: a viewer must not turn the upright picture a second time.  metadata: one PictureMetadata for all
        pictures or one per picture (None entries: none)."""
        n = _wrapped(images)[2]
        items = [metadata] * n if isinstance(metadata, PictureMetadata) or metadata is None else list(metadata)
        if len(items) != n:
            raise SjpegError("Oriented.from_metadata: one metadata entry per image")
        orientations, reset = [], []
        for k, m in enumerate(items):
            if m is None:
                orientations.append(1); reset.append(None)
                continue
            if not isinstance(m, PictureMetadata):
                raise SjpegError(f"Oriented.from_metadata: metadata entry {k} is not a PictureMetadata")
            orientations.append(exif_orientation(m.exif) or 1)
            reset.append(PictureMetadata(m.app_markers, exif_reset_orientation(m.exif), m.iccp, m.xmp, m.xmp_split_point))
        made = cls(images, orientations) if box is None else cls.fit(images, orientations, box, layout)
        return made, reset


def _oriented(images):
    """(the images of a call without their Oriented wrapper -- a Resized where it has sizes --, the orientations or None
    when nothing is turned)"""
    if not isinstance(images, Oriented):
        return images, None
    turned = images.orientations if any(o != 1 for o in images.orientations) else None
    return (images.images if images.sizes is None else Resized(images.images, images.sizes)), turned


def _orientations_array(who, n, orientations):
    """orientations as the C entries take them: uint8 [n], values clamped into a byte (the library names a bad one)"""
    try:
        vals = [int(o) for o in orientations]
    except (TypeError, ValueError):
        raise SjpegError(f"{who}: orientations are ints 1..8, one per frame")
    if len(vals) != n:
        raise SjpegError(f"{who}: one orientation per frame")
    return np.ascontiguousarray(np.clip(np.asarray(vals, dtype=np.int64), 0, 255).astype(np.uint8))


class _FlattenStruct(C.Structure):
    """struct sjpeg_hip_flatten (include/sjpeg_hip.h)"""
    _fields_ = [("background", C.c_uint8 * 3), ("premultiplied", C.c_uint8), ("alpha_scale", C.c_float), ("alpha_bias", C.c_float)]


class Flatten:
    """How pictures with an alpha channel are laid over a background (struct sjpeg_hip_flatten): `background` three
    bytes (R, G, B) as the encoder sees them; premultiplied False for straight alpha -- b = (a s + (255 - a) bg + 127)
    // 255 --, True where the colour samples are multiplied by alpha already -- b = min(255, s + ((255 - a) bg + 127)
    // 255); alpha_scale and alpha_bias turn a float picture's alpha sample into the byte a as FloatPixels turns a
    colour sample into s (255 and 0 for alpha in 0..1; bytes ignore them)."""

    def __init__(self, background=(255, 255, 255), premultiplied=False, alpha_scale=255.0, alpha_bias=0.0):
        try:
            bg = [int(b) for b in background]
        except (TypeError, ValueError):
            raise SjpegError(f"Flatten: background {background!r} is not three bytes 0..255")
        if len(bg) != 3 or any(b < 0 or b > 255 for b in bg):
            raise SjpegError(f"Flatten: background {background!r} is not three bytes 0..255")
        if not isinstance(premultiplied, (bool, int, np.integer)) or int(premultiplied) not in (0, 1):
            raise SjpegError(f"Flatten: premultiplied {premultiplied!r} is not False (straight alpha) or True")
        try:
            sc, bi = float(alpha_scale), float(alpha_bias)
        except (TypeError, ValueError):
            raise SjpegError("Flatten: alpha_scale and alpha_bias are floats")
        if not (np.isfinite(sc) and np.isfinite(bi)):
            raise SjpegError("Flatten: alpha_scale and alpha_bias must be finite")
        self.background, self.premultiplied, self.alpha_scale, self.alpha_bias = tuple(bg), bool(premultiplied), sc, bi

    def _struct(self):
        return _FlattenStruct((C.c_uint8 * 3)(*self.background), int(self.premultiplied), self.alpha_scale, self.alpha_bias)


def _flatten_struct(who, flatten):
    if not isinstance(flatten, Flatten):
        raise SjpegError(f"{who}: flatten is not a Flatten")
    return flatten._struct()


def _flatten_segment(who, flatten, keep):
    """what a shaped call takes for its `flatten`: {"flatten": the address of the Flatten's struct sjpeg_hip_flatten, or
    None for None}; the struct goes into the list `keep`, which has to outlive the call"""
    if flatten is None:
        return {"flatten": None}
    keep.append(_flatten_struct(who, flatten))
    return {"flatten": C.addressof(keep[-1])}


class Flattened:
    """Pictures with an alpha channel to be coded over a background -- PNG and WebP uploads, logos, cut-outs, a
    renderer's RGBA16F, a matting network's colour plus matte -- wherever Oriented is taken: Flattened(images,
    background=(255, 255, 255), premultiplied=False, alpha_scale=255.0, alpha_bias=0.0, orientations=None, sizes=None)
    with `images` a sequence of CUDA uint8 tensors [H_k, W_k, 4] (R, G, B, alpha; stride 1 over the channels, 4 over x,
    any row stride) or a FloatPixels of float tensors [H_k, W_k, 4] laid out the same way, and layout="hwc" (there is
    no channel-first alpha format).  Every pixel is laid over `background` as Flatten defines it, inside the resize
    kernel's loader; the picture is then resized to sizes[k] and turned upright by orientations[k] as Oriented defines
    it, in the same ONE launch, and its JPEG is byte for byte that of the flattened, resized, upright uint8 picture
    (flatten_images returns those).  Flatten comes first: "composite, then thumbnail"."""

    def __init__(self, images, background=(255, 255, 255), premultiplied=False, alpha_scale=255.0, alpha_bias=0.0,
                 orientations=None, sizes=None):
        if _wrapper_of(images) is not None:
            raise SjpegError("Flattened: the pictures are Reduced, Resized, Oriented or Flattened already: Flattened takes the "
                             "orientations and the sizes itself, once")
        self.flatten = Flatten(background, premultiplied, alpha_scale, alpha_bias)
        self.fp = images if isinstance(images, FloatPixels) else None
        self.images = list(images.images if self.fp is not None else images)
        shaped = Oriented(self.images, 1 if orientations is None else orientations, sizes)
        self.orientations = None if orientations is None else shaped.orientations
        self.sizes = shaped.sizes

    @classmethod
    def fit(cls, images, box, background=(255, 255, 255), premultiplied=False, alpha_scale=255.0, alpha_bias=0.0,
            orientations=None, layout="hwc"):
        """Flattened(images, ..., sizes) with every UPRIGHT picture fitted into box = (bw, bh) by fit_size, as
        Oriented.fit does."""
        if _check_layout("Flattened.fit", layout):
            raise SjpegError("Flattened.fit: layout='chw' has no alpha format: Flattened takes [H, W, 4] pictures, layout='hwc'")
        plain = cls(images, background, premultiplied, alpha_scale, alpha_bias, orientations)
        sizes = Oriented.fit(plain.images, 1 if orientations is None else plain.orientations, box).sizes
        return cls(images, background, premultiplied, alpha_scale, alpha_bias, orientations, sizes)


def _flattened(who, images, chw):
    """(the pictures of a call without their Flattened wrapper, the Flattened or None)"""
    if not isinstance(images, Flattened):
        return images, None
    if chw:
        raise SjpegError(f"{who}: layout='chw' has no alpha format: Flattened takes [H, W, 4] pictures, layout='hwc'")
    return images.images, images


def _alpha_pictures(who, images, fp):
    """(planes, dims, device, format) of pictures with an alpha channel: CUDA uint8 tensors [H, W, 4] -- SRC_RGBA -- or,
    with fp (the call's FloatPixels), float tensors [H, W, 4] of one dtype -- SRC_RGBA_F32 / _F16 / _BF16; stride 1 over
    the channels and 4 over x, any row stride (crops of a wider tensor, bottom-up views)"""
    import torch
    images = list(images)
    if not images:
        raise SjpegError(f"{who}: no images")
    by_dtype = {getattr(torch, name): name for name in _DTYPE_BYTES}
    planes, dims = [], []
    for k, im in enumerate(images):
        if not isinstance(im, torch.Tensor) or not im.is_cuda:
            raise SjpegError(f"{who}: image {k} is not a CUDA tensor")
        if fp is None and im.dtype != torch.uint8:
            raise SjpegError(f"{who}: image {k} is {im.dtype}, not torch.uint8 (float pictures: a FloatPixels)")
        if fp is not None and (im.dtype not in by_dtype or im.dtype != images[0].dtype):
            raise SjpegError(f"{who}: image {k} is {im.dtype}: FloatPixels take torch.float32, torch.float16 or torch.bfloat16, "
                             f"one dtype per call")
        if im.dim() != 3 or im.shape[2] != 4 or im.shape[0] < 1 or im.shape[1] < 1 or im.stride(2) != 1 or \
                (im.stride(1) != 4 and im.shape[1] > 1):
            raise SjpegError(f"{who}: image {k} must be [H, W, 4] packed RGBA (stride 1 over the channels, 4 over x): a "
                             f"flattened picture has an alpha channel")
        if im.device != images[0].device:
            raise SjpegError(f"{who}: image {k} is on {im.device}, image 0 on {images[0].device}")
        esz = im.element_size()
        planes.append([(im.data_ptr(), (im.stride(0) if im.shape[0] > 1 else im.shape[1] * 4) * esz)])
        dims.append((int(im.shape[1]), int(im.shape[0])))
    fmt = SRC_RGBA if fp is None else _CHW_FORMAT[("rgba", by_dtype[images[0].dtype])]
    return planes, dims, images[0].device, fmt


class _SheetStruct(C.Structure):
    """struct sjpeg_hip_sheet (include/sjpeg_hip.h)"""
    _fields_ = [("cols", C.c_int32), ("rows", C.c_int32), ("cell_width", C.c_int32), ("cell_height", C.c_int32),
                ("gutter", C.c_int32), ("margin", C.c_int32), ("background", C.c_uint8 * 3), ("reserved", C.c_uint8)]


class Sheet:
    """A contact sheet's grid (struct sjpeg_hip_sheet): cols x rows cells of cell = (cell_width, cell_height), `gutter`
    samples between cells and `margin` around them, `background` three bytes as the encoder sees them -- (R, G, B); gray
    pictures: [0]; YUV frames: (Y, U, V).  Frame f of a call goes to sheet f // (cols * rows), cell f % (cols * rows) in
    row-major order, centred in its cell (the spare sample on the right and at the bottom)."""

    def __init__(self, cols, rows, cell, gutter=0, margin=0, background=(0, 0, 0)):
        try:
            cw, ch = cell
            bg = [int(b) for b in background]
        except (TypeError, ValueError):
            raise SjpegError("Sheet: cell is a pair (width, height), background three bytes")
        if len(bg) != 3 or any(b < 0 or b > 255 for b in bg):
            raise SjpegError(f"Sheet: background {background!r} is not three bytes 0..255")
        self.cols, self.rows, self.cell, self.gutter, self.margin = int(cols), int(rows), (int(cw), int(ch)), int(gutter), int(margin)
        self.background = tuple(bg)

    def _struct(self):
        clamp = lambda v: min(max(int(v), -2**31), 2**31 - 1)        # (the library names a bad value)
        return _SheetStruct(clamp(self.cols), clamp(self.rows), clamp(self.cell[0]), clamp(self.cell[1]), clamp(self.gutter),
                            clamp(self.margin), (C.c_uint8 * 3)(*self.background), 0)


def _sheet_struct(who, sheet):
    if not isinstance(sheet, Sheet):
        raise SjpegError(f"{who}: sheet is not a Sheet")
    return sheet._struct()


def sheet_size(sheet, fmt=SRC_RGB):
    """sjpeg_hip_sheet_size: (SW, SH) of a Sheet for pictures of format fmt, after its checks (the 4:2:0 formats take
    even cells, gutter and margin)."""
    w, h = C.c_int(0), C.c_int(0)
    st = _sheet_struct("sheet_size", sheet)
    if lib().sjpeg_hip_sheet_size(C.byref(st), int(fmt), C.byref(w), C.byref(h)) != 0:
        raise SjpegError(lib().sjpeg_hip_last_error().decode())
    return int(w.value), int(h.value)


def sheet_places(sheet, dims, fmt=SRC_RGB, sizes=None, orientations=None):
    """sjpeg_hip_sheet_places: [(sheet, x0, y0, uw, uh)] of pictures of dims[k] = (w, h) -- the #xywh= numbers of a
    storyboard.  sizes[k] = (w, h) in the STORED orientation (None: every picture fitted into its cell), orientations
    EXIF 1..8 (None: all 1).  Host only: no device memory is read."""
    n = len(dims)
    if n == 0:
        raise SjpegError("sheet_places: no pictures")
    frames = (RaggedFrame * n)()
    for k, (w, h) in enumerate(dims):
        frames[k].width, frames[k].height = int(w), int(h)
    arr = None if sizes is None else _sizes_array("sheet_places", sizes)
    oarr = None if orientations is None else _orientations_array("sheet_places", n, orientations)
    if arr is not None and len(arr) != n:
        raise SjpegError("sheet_places: one size per picture")
    st = _sheet_struct("sheet_places", sheet)
    out = np.zeros((n, 5), np.int32)
    if lib().sjpeg_hip_sheet_places(int(fmt), n, frames, C.addressof(st), None if arr is None else arr.ctypes.data,
                                    None if oarr is None else oarr.ctypes.data, out.ctypes.data) != 0:
        raise SjpegError(lib().sjpeg_hip_last_error().decode())
    return [tuple(int(v) for v in row) for row in out]


class RaggedFrame(C.Structure):
    """struct sjpeg_hip_ragged_frame (include/sjpeg_hip.h): one picture of a ragged batch."""
    _fields_ = [("plane", C.c_void_p * 3), ("row_stride", C.c_int64 * 3), ("width", C.c_int32),
                ("height", C.c_int32), ("out_offset", C.c_uint64), ("out_capacity", C.c_uint64)]


class SearchParams(C.Structure):
    """struct sjpeg_hip_search (include/sjpeg_hip.h): the multi-pass search of one picture of a ragged batch --
    target_mode 1 (size in bytes) or 2 (PSNR in dB), target_value, passes (1..20; <= 1: no search), tolerance (percent),
    qmin, qmax."""
    _fields_ = [("target_mode", C.c_int32), ("target_value", C.c_float), ("passes", C.c_int32),
                ("tolerance", C.c_float), ("qmin", C.c_float), ("qmax", C.c_float)]


class RaggedParams(C.Structure):
    """struct sjpeg_hip_ragged_params (include/sjpeg_hip.h): what sjpeg_hip_encode_ragged_packed_src codes its frames
    with -- the arguments of the unpacked ragged encodes in one structure."""
    _fields_ = [("yuv_mode", C.c_int32), ("method", C.c_int32), ("quant", C.c_void_p), ("quant_per_frame", C.c_int32),
                ("min_quant", C.c_void_p), ("q_bias", C.c_int32), ("qdelta_max_luma", C.c_int32),
                ("qdelta_max_chroma", C.c_int32), ("search", C.POINTER(SearchParams)), ("search_per_frame", C.c_int32)]


PACKED_OVERFLOW = 1 << 63        # SJPEG_HIP_PACKED_OVERFLOW: bit 63 of offsets[nframes]


class HuffmanSpec(C.Structure):
    """struct sjpeg_hip_huffman_spec (include/sjpeg_hip.h)."""
    _fields_ = [("bits", C.c_uint8 * 16), ("syms", C.c_uint8 * 256), ("nsyms", C.c_int32)]


class SjpegError(RuntimeError):
    pass


def build(verbose: bool = False) -> str:
    """Compile the HIP/C++ library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", CSRC] + ([] if verbose else ["-s"]))
    return LIB_PATH


from sjpeg_amd import _binding  # noqa: E402  (it takes the structures above)

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    try:
        # When torch is around it must come first: it ships its own HIP runtime, and one
        # process must hold exactly one (device pointers and streams are shared with torch).
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `make -C sjpeg_amd/csrc` "
                          "(or __graft_entry__.build()); there is no pure-Python fallback")
    L = C.CDLL(LIB_PATH, mode=os.RTLD_LOCAL | os.RTLD_NOW)
    _binding.apply(L, EXPORTED_C_SYMBOLS)
    _lib = L
    return L


EXPORTED_C_SYMBOLS = [
    # include/sjpeg.h (extern "C" part)
    "SjpegVersion", "SjpegCompress", "SjpegEncode", "SjpegFreeBuffer", "SjpegDimensions",
    "SjpegFindQuantizer", "SjpegEstimateQuality", "SjpegQuantMatrix", "SjpegRiskiness", "SjpegHipLastError",
    # include/sjpeg_hip.h
    "sjpeg_hip_abi_version", "sjpeg_hip_device_count", "sjpeg_hip_last_error",
    "sjpeg_hip_engine_create", "sjpeg_hip_engine_destroy", "sjpeg_hip_frame_bound",
    "sjpeg_hip_encode_scan", "sjpeg_hip_scan_coeffs", "sjpeg_hip_quality_matrices",
    "sjpeg_hip_finalize_quant", "sjpeg_hip_default_huffman", "sjpeg_hip_make_header",
    "sjpeg_hip_scan_histogram", "sjpeg_hip_scan_symbol_stats", "sjpeg_hip_adapt_quant",
    "sjpeg_hip_adapt_sums", "sjpeg_hip_adapt_quant_sums", "sjpeg_hip_adapt_decide",
    "sjpeg_hip_encode_scan_src", "sjpeg_hip_scan_coeffs_src", "sjpeg_hip_scan_histogram_src",
    "sjpeg_hip_scan_symbol_stats_src", "sjpeg_hip_scan_quant_error_src", "sjpeg_hip_engine_entropy_bits",
    "sjpeg_hip_engine_trim", "sjpeg_hip_host_trim",
    "sjpeg_hip_encode_scan_multi", "sjpeg_hip_scan_symbol_stats_multi",
    "sjpeg_hip_engine_set_pipelined", "sjpeg_hip_engine_set_pixel_transform", "sjpeg_hip_engine_get_pixel_transform",
    "sjpeg_hip_engine_set_pixel_transform3", "sjpeg_hip_engine_get_pixel_transform3",
    "sjpeg_hip_engine_wait", "sjpeg_hip_encode_batch_src",
    "sjpeg_hip_optimize_huffman", "sjpeg_hip_make_header_ex", "sjpeg_hip_make_header_meta",
    "sjpeg_hip_sharp_workspace", "sjpeg_hip_sharp_yuv",
    "sjpeg_hip_set_riskiness_table", "sjpeg_hip_has_riskiness_table", "sjpeg_hip_riskiness_sums",
    "sjpeg_hip_segment_count", "sjpeg_hip_band_bound", "sjpeg_hip_encode_band_src", "sjpeg_hip_stitch_bands",
    "sjpeg_hip_engine_set_timing", "sjpeg_hip_engine_last_scan_ms",
    "sjpeg_hip_engine_last_total_ms", "sjpeg_hip_engine_scratch_bytes", "sjpeg_hip_compact_streams",
    "sjpeg_hip_debug_stream_read", "sjpeg_hip_debug_valu_rate", "sjpeg_hip_debug_shader_clock",
    "sjpeg_hip_restart_interval", "sjpeg_hip_header_add_restart", "sjpeg_hip_encode_intervals_src",
    "sjpeg_hip_comm_unique_id", "sjpeg_hip_comm_create", "sjpeg_hip_comm_create_local", "sjpeg_hip_comm_adopt", "sjpeg_hip_comm_destroy",
    "sjpeg_hip_comm_rank", "sjpeg_hip_comm_world", "sjpeg_hip_gather_rows", "sjpeg_hip_gather_bytes",
    "sjpeg_hip_gather_streams", "sjpeg_hip_encode_scan_packed_src", "sjpeg_hip_encode_ragged_src",
    "sjpeg_hip_scan_histogram_ragged_src", "sjpeg_hip_scan_symbol_stats_ragged_src", "sjpeg_hip_encode_ragged_batch_src",
    "sjpeg_hip_riskiness_ragged_src", "sjpeg_hip_riskiness_verdict", "sjpeg_hip_sharp_ragged_workspace",
    "sjpeg_hip_sharp_yuv_ragged", "sjpeg_hip_encode_ragged_auto_src",
    "sjpeg_hip_scan_quant_error_ragged_src", "sjpeg_hip_scan_counted_bits_ragged_src", "sjpeg_hip_encode_ragged_search_src",
    "sjpeg_hip_encode_ragged_trellis_src", "sjpeg_hip_encode_ragged_packed_src",
    "sjpeg_hip_encode_ragged_full_src", "sjpeg_hip_encode_ragged_full_packed_src", "sjpeg_hip_engine_search_stats",
    "sjpeg_hip_metadata_size", "sjpeg_hip_encode_ragged_full_meta_src", "sjpeg_hip_encode_ragged_full_meta_packed_src",
    "sjpeg_hip_reduced_size", "sjpeg_hip_reduce_ragged_bytes", "sjpeg_hip_reduce_ragged_src",
    "sjpeg_hip_encode_ragged_reduced_src", "sjpeg_hip_encode_ragged_reduced_packed_src",
    "sjpeg_hip_fit_size", "sjpeg_hip_resize_ragged_bytes", "sjpeg_hip_resize_ragged_src",
    "sjpeg_hip_encode_ragged_resized_src", "sjpeg_hip_encode_ragged_resized_packed_src",
    "sjpeg_hip_oriented_size", "sjpeg_hip_orient_ragged_bytes", "sjpeg_hip_orient_ragged_src",
    "sjpeg_hip_encode_ragged_oriented_src", "sjpeg_hip_encode_ragged_oriented_packed_src",
    "sjpeg_hip_exif_orientation", "sjpeg_hip_exif_reset_orientation",
    "sjpeg_hip_yuv_plane_size", "sjpeg_hip_resize_ragged_yuv_bytes", "sjpeg_hip_resize_ragged_yuv_src",
    "sjpeg_hip_encode_ragged_yuv_resized_src", "sjpeg_hip_encode_ragged_yuv_resized_packed_src",
    "sjpeg_hip_sheet_size", "sjpeg_hip_sheet_places", "sjpeg_hip_sheet_ragged_bytes", "sjpeg_hip_sheet_ragged_src",
    "sjpeg_hip_encode_ragged_sheet_src", "sjpeg_hip_encode_ragged_sheet_packed_src",
    "sjpeg_hip_flatten_ragged_src", "sjpeg_hip_encode_ragged_flattened_src", "sjpeg_hip_encode_ragged_flattened_packed_src",
    "sjpeg_hip_sheet_ragged_flat_src", "sjpeg_hip_encode_ragged_sheet_flat_src", "sjpeg_hip_encode_ragged_sheet_flat_packed_src",
    # (called from sjpeg_amd/video.py)
    "sjpeg_hip_yuv_colour_samples", "sjpeg_hip_convert_ragged_yuv_src",
    "sjpeg_hip_encode_ragged_yuv_converted_src", "sjpeg_hip_encode_ragged_yuv_converted_packed_src",
    "sjpeg_hip_sheet_ragged_yuv_colour_src", "sjpeg_hip_encode_ragged_sheet_yuv_colour_src",
    "sjpeg_hip_encode_ragged_sheet_yuv_colour_packed_src",
    "sjpeg_hip_yuv16_samples", "sjpeg_hip_convert_ragged_yuv16_src",
    "sjpeg_hip_encode_ragged_yuv16_src", "sjpeg_hip_encode_ragged_yuv16_packed_src",
    "sjpeg_hip_sheet_ragged_yuv16_src", "sjpeg_hip_encode_ragged_sheet_yuv16_src",
    "sjpeg_hip_encode_ragged_sheet_yuv16_packed_src",
    # (called from sjpeg_amd/light.py)
    "sjpeg_hip_light_table", "sjpeg_hip_light_round", "sjpeg_hip_linear_ragged_src",
    "sjpeg_hip_encode_ragged_linear_src", "sjpeg_hip_encode_ragged_linear_packed_src",
    "sjpeg_hip_sheet_ragged_linear_src", "sjpeg_hip_encode_ragged_sheet_linear_src",
    "sjpeg_hip_encode_ragged_sheet_linear_packed_src",
    # (called from sjpeg_amd/unsharp.py)
    "sjpeg_hip_unsharp_sample", "sjpeg_hip_unsharp_ragged_src", "sjpeg_hip_encode_ragged_unsharp_src",
    "sjpeg_hip_encode_ragged_unsharp_packed_src", "sjpeg_hip_unsharp_ragged_yuv_src",
    "sjpeg_hip_encode_ragged_yuv_unsharp_src", "sjpeg_hip_encode_ragged_yuv_unsharp_packed_src",
    # (called from sjpeg_amd/resample.py)
    "sjpeg_hip_resample_ksize", "sjpeg_hip_resample_table", "sjpeg_hip_resample_ragged_bytes", "sjpeg_hip_resample_ragged_src",
    "sjpeg_hip_encode_ragged_resampled_src", "sjpeg_hip_encode_ragged_resampled_packed_src",
    "sjpeg_hip_thumbnail_size", "sjpeg_hip_fit_crop", "sjpeg_hip_resample_box_decide", "sjpeg_hip_resample_box_ksize",
    "sjpeg_hip_resample_box_table", "sjpeg_hip_resample_box_ragged_bytes", "sjpeg_hip_resample_box_ragged_src",
    "sjpeg_hip_encode_ragged_resampled_box_src", "sjpeg_hip_encode_ragged_resampled_box_packed_src",
    "sjpeg_hip_pillow_filter_weights", "sjpeg_hip_filter_ragged_src", "sjpeg_hip_encode_ragged_filtered_src",
    "sjpeg_hip_encode_ragged_filtered_packed_src",
    "sjpeg_hip_contain_size", "sjpeg_hip_pad_place", "sjpeg_hip_compose_sample", "sjpeg_hip_compose_ragged_bytes",
    "sjpeg_hip_compose_ragged_src", "sjpeg_hip_encode_ragged_composed_src", "sjpeg_hip_encode_ragged_composed_packed_src",
]


def restart_interval(yuv_mode: int) -> int:
    """MCUs per restart interval of the optional restart mode = per K1 segment (41 / 82 / 246)."""
    return int(lib().sjpeg_hip_restart_interval(int(yuv_mode)))


def header_add_restart(header: bytes, yuv_mode: int) -> bytes:
    """The header with the DRI segment of the restart mode in front of SOS."""
    buf = (C.c_uint8 * (len(header) + 6)).from_buffer_copy(header + b"\0" * 6)
    n = lib().sjpeg_hip_header_add_restart(buf, C.c_size_t(len(header)), C.c_size_t(len(header) + 6), int(yuv_mode))
    if n == 0:
        raise SjpegError("sjpeg_hip_header_add_restart failed")
    return bytes(buf[:n])


def compact_streams(out, sizes, nframes=None, capacity=None, packed=None, offsets=None):
    """sjpeg_hip_compact_streams: the first `nframes` coded frames of `out` ([F, stride] uint8 CUDA,
    stride a multiple of 16) / `sizes` ([F] int64 CUDA) back to back, every frame at a multiple of 16.
    Returns (packed uint8 [capacity], offsets int64 [nframes + 1]); offsets[nframes] = bytes needed.
    One launch on the current stream, no synchronisation."""
    import torch
    n = int(out.shape[0] if nframes is None else nframes)
    stride = int(out.stride(0))
    if capacity is None:
        capacity = n * stride
    if packed is None:
        packed = torch.empty(int(capacity), dtype=torch.uint8, device=out.device)
    if offsets is None:
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=out.device)
    rc = lib().sjpeg_hip_compact_streams(C.c_void_p(out.data_ptr()), C.c_size_t(stride), C.c_void_p(sizes.data_ptr()), n,
                                         C.c_void_p(packed.data_ptr()), C.c_size_t(int(packed.numel())),
                                         C.c_void_p(offsets.data_ptr()),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise SjpegError(f"sjpeg_hip_compact_streams: {lib().sjpeg_hip_last_error().decode()}")
    return packed, offsets


def comm_unique_id() -> bytes:
    """sjpeg_hip_comm_unique_id: the 128 bytes rank 0 hands to the other ranks."""
    buf = (C.c_uint8 * 128)()
    if lib().sjpeg_hip_comm_unique_id(buf) != 0:
        raise SjpegError(f"sjpeg_hip_comm_unique_id: {lib().sjpeg_hip_last_error().decode()}")
    return bytes(buf)


class Comm:
    """The library's RCCL communicator (sjpeg_hip_comm_create): one per process, the device current."""

    def __init__(self, unique_id: bytes, rank: int, world: int, local: bool = False):
        """local: the ranks are threads of THIS process (sjpeg_hip_comm_create_local; any 128 bytes as the id)."""
        self._c = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        make = lib().sjpeg_hip_comm_create_local if local else lib().sjpeg_hip_comm_create
        if make(buf, int(rank), int(world), C.byref(self._c)) != 0:
            raise SjpegError(f"sjpeg_hip_comm_create{'_local' if local else ''}: {lib().sjpeg_hip_last_error().decode()}")
        self.rank, self.world = int(rank), int(world)

    def close(self):
        if self._c:
            lib().sjpeg_hip_comm_destroy(self._c)
            self._c = C.c_void_p()

    def gather_rows(self, offsets, sizes, n_local, per_max, rows_dev):
        """sjpeg_hip_gather_rows on the current stream (waits for it).  Returns (rows [world][per_max + 2]
        numpy uint64, rank_offsets [world + 1] numpy uint64) on every rank."""
        import torch
        rows = np.zeros((self.world, per_max + 2), np.uint64)
        offs = np.zeros(self.world + 1, np.uint64)
        rc = lib().sjpeg_hip_gather_rows(
            self._c, C.c_void_p(offsets.data_ptr()), C.c_void_p(sizes.data_ptr() if n_local > 0 else 0),
            int(n_local), int(per_max), C.c_void_p(rows_dev.data_ptr()), C.c_void_p(rows.ctypes.data),
            C.c_void_p(offs.ctypes.data), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise SjpegError(f"sjpeg_hip_gather_rows: {lib().sjpeg_hip_last_error().decode()}")
        return rows, offs

    def gather_bytes(self, root, packed, per_max, rows, offs, gathered):
        """sjpeg_hip_gather_bytes on the current stream: enqueues the exact-length transfers."""
        import torch
        rc = lib().sjpeg_hip_gather_bytes(
            self._c, int(root), C.c_void_p(packed.data_ptr()), int(per_max), C.c_void_p(rows.ctypes.data),
            C.c_void_p(offs.ctypes.data), C.c_void_p(gathered.data_ptr() if gathered is not None else 0),
            C.c_size_t(int(gathered.numel()) if gathered is not None else 0),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise SjpegError(f"sjpeg_hip_gather_bytes: {lib().sjpeg_hip_last_error().decode()}")

    def gather_streams(self, root, packed, offsets, sizes, n_local, per_max, rows_dev, gathered):
        """sjpeg_hip_gather_streams: rows + the capacity check on EVERY rank + the transfers, one call.
        gathered (the root's buffer; its numel() is the capacity every rank passes) may be a tensor or an int
        capacity on the ranks that are not the root.  Returns (rows, rank_offsets) like gather_rows."""
        import torch
        rows = np.zeros((self.world, per_max + 2), np.uint64)
        offs = np.zeros(self.world + 1, np.uint64)
        is_t = hasattr(gathered, "data_ptr")
        rc = lib().sjpeg_hip_gather_streams(
            self._c, int(root), C.c_void_p(packed.data_ptr() if packed is not None else 0),
            C.c_void_p(offsets.data_ptr()), C.c_void_p(sizes.data_ptr() if n_local > 0 else 0), int(n_local),
            int(per_max), C.c_void_p(rows_dev.data_ptr()), C.c_void_p(gathered.data_ptr() if is_t else 0),
            C.c_size_t(int(gathered.numel()) if is_t else int(gathered)), C.c_void_p(rows.ctypes.data),
            C.c_void_p(offs.ctypes.data), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise SjpegError(f"sjpeg_hip_gather_streams: {lib().sjpeg_hip_last_error().decode()}")
        return rows, offs


# ---------------------------------------------------------------- host API (sjpeg.h)

def last_error() -> str:
    return (lib().SjpegHipLastError() or b"").decode()


def host_trim() -> int:
    """Releases the device memory the host API caches for the calling thread (sjpeg_hip_host_trim);
    returns the number of bytes given back."""
    return int(lib().sjpeg_hip_host_trim())


def set_riskiness_table(table: bytes) -> None:
    """Installs the reference's riskiness score table (117649 bytes) for SJPEG_YUV_AUTO."""
    buf = (C.c_uint8 * len(table)).from_buffer_copy(table)
    if lib().sjpeg_hip_set_riskiness_table(buf, len(table)) != 0:
        raise SjpegError("sjpeg_hip_set_riskiness_table: wrong size")


def SjpegRiskiness(rgb: np.ndarray):
    """(SjpegYUVMode, risk) like the reference's SjpegRiskiness; (YUV_AUTO, -1.0) if the table is missing."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[0], rgb.shape[1]
    risk = C.c_float(0)
    mode = lib().SjpegRiskiness(rgb.ctypes.data, w, h, 3 * w, C.byref(risk))
    return int(mode), float(risk.value)


def SjpegCompress(rgb: np.ndarray, quality: float = 75.0):
    """SjpegCompress() of include/sjpeg.h (method 4, SJPEG_YUV_AUTO).  Returns bytes or None."""
    return SjpegEncode(rgb, quality, 4, YUV_AUTO)


def SjpegEncode(rgb: np.ndarray, quality: float = 75.0, method: int = 0,
                yuv_mode: int = YUV_420, stride=None):
    """SjpegEncode() of include/sjpeg.h on a host image (H, W, 3) uint8.  Returns bytes or None."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[0], rgb.shape[1]
    out = _u8p()
    base = rgb.ctypes.data
    if stride is None:
        stride = rgb.strides[0]
    elif stride < 0:
        base = rgb.ctypes.data + (h - 1) * (-stride)     # first row = last in memory
    n = lib().SjpegEncode(base, w, h, stride, C.byref(out), quality, method, yuv_mode)
    if n == 0:
        return None
    data = bytes((C.c_ubyte * n).from_address(C.addressof(out.contents)))   # (string_at: 2 GiB limit)
    lib().SjpegFreeBuffer(out)
    return data


# ---------------------------------------------------------------- device C-ABI (sjpeg_hip.h)

def device_count() -> int:
    return lib().sjpeg_hip_device_count()


def make_tables(quality=None, quant=None, min_quant=None, q_bias=0x78):
    """(ScanTables, final quant[2][64]) exactly as the reference's host code prepares them."""
    L = lib()
    q = np.zeros((2, 64), np.uint8)
    if quant is None:
        L.sjpeg_hip_quality_matrices(float(quality), q.ctypes.data)
    else:
        q[:] = np.asarray(quant, np.uint8).reshape(2, 64)
    t = ScanTables()
    mq = None
    if min_quant is not None:
        mq = np.ascontiguousarray(min_quant, np.uint8).reshape(2, 64)
    L.sjpeg_hip_finalize_quant(q.ctypes.data, mq.ctypes.data if mq is not None else None, q_bias,
                               C.byref(t))
    L.sjpeg_hip_default_huffman(C.byref(t))
    return t, q


def make_header(w, h, yuv_mode, quant) -> bytes:
    buf = np.zeros(2048, np.uint8)
    q = np.ascontiguousarray(quant, np.uint8).reshape(2, 64)
    n = lib().sjpeg_hip_make_header(w, h, yuv_mode, q.ctypes.data, buf.ctypes.data, buf.size)
    if n == 0:
        raise SjpegError("sjpeg_hip_make_header failed")
    return buf[:n].tobytes()


def adapt_quant(hist: np.ndarray, yuv_mode, quant, min_quant=None, q_bias=0x78, dmax_luma=12,
                dmax_chroma=1):
    """Host AnalyseHisto on one frame's histogram [2][64][128]; returns (ScanTables, new quant)."""
    h = np.ascontiguousarray(hist, np.uint32).reshape(2, 64, 128)
    q = np.ascontiguousarray(quant, np.uint8).reshape(2, 64).copy()
    mq = None if min_quant is None else np.ascontiguousarray(min_quant, np.uint8).reshape(2, 64)
    t = ScanTables()
    lib().sjpeg_hip_finalize_quant(q.ctypes.data, mq.ctypes.data if mq is not None else None, q_bias,
                                   C.byref(t))
    lib().sjpeg_hip_adapt_quant(h.ctypes.data, yuv_mode, q.ctypes.data,
                                mq.ctypes.data if mq is not None else None, q_bias, dmax_luma,
                                dmax_chroma, C.byref(t))
    lib().sjpeg_hip_default_huffman(C.byref(t))
    return t, q


def adapt_quant_device_batch(hists_dev, yuv_mode, quant, min_quant=None, q_bias=0x78, dmax_luma=12,
                             dmax_chroma=1):
    """AnalyseHisto for a batch with the bin loops on the GPU: hists_dev = CUDA int32 tensor
    [F, 2, 64, 128] (Engine.scan_histogram()); ONE launch, the sums come back (52 KB per frame),
    the float half runs on the host per frame.  Returns [(ScanTables, quant[2][64])] * F."""
    import torch
    q0 = np.ascontiguousarray(quant, np.uint8).reshape(2, 64).copy()
    mq = None if min_quant is None else np.ascontiguousarray(min_quant, np.uint8).reshape(2, 64)
    mqp = mq.ctypes.data if mq is not None else None
    f = hists_dev.shape[0]
    sums = torch.zeros((f, 2, 64, 25, 2), dtype=torch.int64, device=hists_dev.device)
    totlast = torch.zeros((f, 2, 64, 2), dtype=torch.int32, device=hists_dev.device)
    L = lib()
    rc = L.sjpeg_hip_adapt_sums(hists_dev.contiguous().data_ptr(), f, q0.ctypes.data, mqp, sums.data_ptr(),
                                totlast.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise SjpegError("sjpeg_hip_adapt_sums: " + L.sjpeg_hip_last_error().decode())
    s_host = np.ascontiguousarray(sums.cpu().numpy())
    t_host = np.ascontiguousarray(totlast.cpu().numpy())
    res = []
    for k in range(f):
        q = q0.copy()
        t = ScanTables()
        L.sjpeg_hip_finalize_quant(q.ctypes.data, mqp, q_bias, C.byref(t))
        L.sjpeg_hip_adapt_quant_sums(s_host[k].ctypes.data, t_host[k].ctypes.data, yuv_mode, q.ctypes.data, mqp,
                                     q_bias, dmax_luma, dmax_chroma, C.byref(t))
        L.sjpeg_hip_default_huffman(C.byref(t))
        res.append((t, q))
    return res


def adapt_quant_on_device(hists_dev, yuv_mode, quant, min_quant=None, dmax_luma=12, dmax_chroma=1, q_bias=0x78):
    """AnalyseHisto for a batch with BOTH halves on the GPU (sjpeg_hip_adapt_sums + sjpeg_hip_adapt_decide): hists_dev =
    CUDA int32 tensor [F, 2, 64, 128]; returns the adapted matrices, uint8 [F, 2, 64] (4:0:0: table 1 = quant's).  The
    starting matrices are finalized first (raised to min_quant), as adapt_quant() and the batch path do."""
    import torch
    q0 = np.ascontiguousarray(quant, np.uint8).reshape(2, 64).copy()
    mq = None if min_quant is None else np.ascontiguousarray(min_quant, np.uint8).reshape(2, 64)
    mqp = mq.ctypes.data if mq is not None else None
    lib().sjpeg_hip_finalize_quant(q0.ctypes.data, mqp, q_bias, C.byref(ScanTables()))
    f = hists_dev.shape[0]
    sums = torch.zeros((f, 2, 64, 25, 2), dtype=torch.int64, device=hists_dev.device)
    totlast = torch.zeros((f, 2, 64, 2), dtype=torch.int32, device=hists_dev.device)
    out = torch.from_numpy(np.broadcast_to(q0, (f, 2, 64)).copy()).to(hists_dev.device)
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    rc = L.sjpeg_hip_adapt_sums(hists_dev.contiguous().data_ptr(), f, q0.ctypes.data, mqp, sums.data_ptr(), totlast.data_ptr(), st)
    if rc == 0:
        rc = L.sjpeg_hip_adapt_decide(sums.data_ptr(), totlast.data_ptr(), f, q0.ctypes.data, yuv_mode, dmax_luma, dmax_chroma,
                                      out.data_ptr(), st)
    if rc != 0:
        raise SjpegError("sjpeg_hip_adapt_sums / _decide: " + L.sjpeg_hip_last_error().decode())
    return out.cpu().numpy()


def adapt_quant_device(hist_dev, yuv_mode, quant, min_quant=None, q_bias=0x78, dmax_luma=12, dmax_chroma=1):
    """One frame of adapt_quant_device_batch(): hist_dev = CUDA int32 tensor [2, 64, 128]."""
    return adapt_quant_device_batch(hist_dev.unsqueeze(0), yuv_mode, quant, min_quant, q_bias, dmax_luma,
                                    dmax_chroma)[0]


def optimize_huffman(freq: np.ndarray, yuv_mode, tables: ScanTables):
    """Host BuildOptimalTable on one frame's symbol statistics [2][272]; installs the codes into
    `tables` and returns the four HuffmanSpec (DC luma, DC chroma, AC luma, AC chroma)."""
    f = np.ascontiguousarray(freq, np.uint32).reshape(2, 272)
    specs = (HuffmanSpec * 4)()
    lib().sjpeg_hip_optimize_huffman(f.ctypes.data, yuv_mode, specs, C.byref(tables))
    return specs


def make_header_ex(w, h, yuv_mode, quant, specs) -> bytes:
    buf = np.zeros(4096, np.uint8)
    q = np.ascontiguousarray(quant, np.uint8).reshape(2, 64)
    n = lib().sjpeg_hip_make_header_ex(w, h, yuv_mode, q.ctypes.data, specs, buf.ctypes.data, buf.size)
    if n == 0:
        raise SjpegError("sjpeg_hip_make_header_ex failed")
    return buf[:n].tobytes()


class Metadata(C.Structure):
    """struct sjpeg_hip_metadata (include/sjpeg_hip.h)."""
    _fields_ = [("app_markers", C.c_char_p), ("app_markers_size", C.c_size_t),
                ("exif", C.c_char_p), ("exif_size", C.c_size_t),
                ("iccp", C.c_char_p), ("iccp_size", C.c_size_t),
                ("xmp", C.c_char_p), ("xmp_size", C.c_size_t),
                ("xmp_split_point", C.c_uint16)]


def make_header_meta(w, h, yuv_mode, quant, specs=None, app_markers=b"", exif=b"", iccp=b"", xmp=b"",
                     xmp_split_point=0):
    """Header bytes SOI..SOS with metadata segments; None if the metadata is invalid."""
    m = Metadata(app_markers or None, len(app_markers), exif or None, len(exif), iccp or None, len(iccp),
                 xmp or None, len(xmp), xmp_split_point)
    cap = 4096 + len(app_markers) + len(exif) + len(iccp) + len(xmp) + 64 * (len(iccp) // 65000 + len(xmp) // 65000 + 4)
    buf = np.zeros(cap, np.uint8)
    q = np.ascontiguousarray(quant, np.uint8).reshape(2, 64)
    n = lib().sjpeg_hip_make_header_meta(w, h, yuv_mode, q.ctypes.data, specs, C.byref(m), buf.ctypes.data, cap)
    return buf[:n].tobytes() if n else None


class PictureMetadata:
    """The metadata one picture carries into its JPEG, as the reference's EncoderParam holds it: raw application
    markers (verbatim), EXIF, an ICC profile, XMP, and where a long XMP packet is split (0: the default)."""

    def __init__(self, app_markers=b"", exif=b"", iccp=b"", xmp=b"", xmp_split_point=0):
        self.app_markers, self.exif, self.iccp, self.xmp = bytes(app_markers), bytes(exif), bytes(iccp), bytes(xmp)
        self.xmp_split_point = int(xmp_split_point)
        self._size = None

    def _struct(self):
        return Metadata(self.app_markers or None, len(self.app_markers), self.exif or None, len(self.exif),
                        self.iccp or None, len(self.iccp), self.xmp or None, len(self.xmp), self.xmp_split_point)

    def size(self) -> int:
        """sjpeg_hip_metadata_size: the bytes these segments take behind SOI + APP0; SjpegError for metadata the
        reference refuses.  Worked out once: the object's bytes do not change."""
        if self._size is None:
            n = C.c_size_t(0)
            m = self._struct()
            if lib().sjpeg_hip_metadata_size(C.byref(m), C.byref(n)) != 0:
                raise SjpegError(lib().sjpeg_hip_last_error().decode())
            self._size = int(n.value)
        return self._size


def _metadata_args(who, n, metadata):
    """What a ragged call hands to the library for `metadata` -- None, one PictureMetadata for all n pictures or a
    sequence of one per picture (None entries: no metadata): (the sjpeg_hip_metadata array or None, whether there is one
    per frame, every frame's metadata size, every frame's PictureMetadata or None).  The array points into the objects'
    bytes: they stay alive in the fourth result."""
    if metadata is None:
        return None, 0, [0] * n, [None] * n
    if isinstance(metadata, (str, bytes)):
        raise SjpegError(f"{who}: metadata is a PictureMetadata or a sequence of them (layout is passed by keyword)")
    per_frame = not isinstance(metadata, PictureMetadata)
    items = list(metadata) if per_frame else [metadata]
    if per_frame and len(items) != n:
        raise SjpegError(f"{who}: one metadata entry per image")
    items = [PictureMetadata() if m is None else m for m in items]
    for k, m in enumerate(items):
        if not isinstance(m, PictureMetadata):
            raise SjpegError(f"{who}: metadata entry {k} is not a PictureMetadata")
    sizes = []
    for k, m in enumerate(items):
        try:
            sizes.append(m.size())
        except SjpegError as e:
            raise SjpegError(f"{who}: metadata entry {k}: {e}") from None
    arr = (Metadata * len(items))(*[m._struct() for m in items])
    if not per_frame:
        sizes, items = sizes * n, items * n
    return arr, int(per_frame), sizes, items


def frame_bound(w, h, yuv_mode, header_size) -> int:
    return lib().sjpeg_hip_frame_bound(w, h, yuv_mode, header_size)


class Engine:
    """sjpeg_hip_engine bound to one device; drives device-resident (torch) frames."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        rc = lib().sjpeg_hip_engine_create(device, C.byref(self._h))
        if rc != 0:
            raise SjpegError(f"sjpeg_hip_engine_create: {lib().sjpeg_hip_last_error().decode()}")
        self.device = device

    def close(self):
        if self._h:
            lib().sjpeg_hip_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_timing(self, on: bool):
        lib().sjpeg_hip_engine_set_timing(self._h, int(on))

    def set_pipelined(self, on: bool):
        """Back-to-back encode calls overlap (stitch of call i under K1 of call i + 1); outputs are
        complete after wait() or a device synchronisation (include/sjpeg_hip.h)."""
        self._chk(lib().sjpeg_hip_engine_set_pipelined(self._h, int(on)), "sjpeg_hip_engine_set_pipelined")

    def set_pixel_transform(self, scale=255.0, bias=0.0):
        """The transform of the float source formats: a sample x of channel c is coded as the byte
        rint(clamp(fma(x, scale[c], bias[c]), 0, 255)).  scale and bias: one value each for the three channels alike,
        or a sequence of three (R, G, B; gray pictures use the first).  Sticky: it holds until it is set again."""
        s3, b3 = _three("Engine.set_pixel_transform", "scale", scale), _three("Engine.set_pixel_transform", "bias", bias)
        self._chk(lib().sjpeg_hip_engine_set_pixel_transform3(self._h, (C.c_float * 3)(*s3), (C.c_float * 3)(*b3)),
                  "sjpeg_hip_engine_set_pixel_transform3")

    def pixel_transform3(self):
        """((scale R, G, B), (bias R, G, B)) as the engine holds them"""
        s, b = (C.c_float * 3)(), (C.c_float * 3)()
        self._chk(lib().sjpeg_hip_engine_get_pixel_transform3(self._h, s, b), "sjpeg_hip_engine_get_pixel_transform3")
        return tuple(s), tuple(b)

    def pixel_transform(self):
        s, b = C.c_float(), C.c_float()
        self._chk(lib().sjpeg_hip_engine_get_pixel_transform(self._h, C.byref(s), C.byref(b)),
                  "sjpeg_hip_engine_get_pixel_transform")
        return s.value, b.value

    def wait(self):
        """Makes the current torch stream wait for everything the engine has in flight."""
        self._chk(lib().sjpeg_hip_engine_wait(self._h, self._stream()), "sjpeg_hip_engine_wait")

    def last_scan_ms(self) -> float:
        return lib().sjpeg_hip_engine_last_scan_ms(self._h)

    def last_total_ms(self) -> float:
        return lib().sjpeg_hip_engine_last_total_ms(self._h)

    def scratch_bytes(self) -> int:
        """Device memory the engine holds right now (sjpeg_hip_engine_scratch_bytes)."""
        return int(lib().sjpeg_hip_engine_scratch_bytes(self._h))

    def trim(self) -> None:
        """Give the engine's scratch back to the device (sjpeg_hip_engine_trim); the next call
        allocates what it needs again."""
        self._chk(lib().sjpeg_hip_engine_trim(self._h), "sjpeg_hip_engine_trim")

    @staticmethod
    def _stream():
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _check_frames(frames):
        """The C-ABI takes only a row and a frame stride: pixels must be packed RGB, 3 bytes apart."""
        import torch
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
                and frames.stride(3) == 1 and frames.stride(2) == 3):
            raise SjpegError("frames must be a CUDA uint8 tensor [F, H, W, 3] of packed RGB pixels "
                             "(stride 1 over the channels, 3 over x); call .contiguous() on a permuted or sliced view")

    def encode_frames(self, frames, tables: ScanTables, header: bytes, yuv_mode: int,
                      out=None, sizes=None, out_stride=None, append_eoi=True):
        """frames: torch.uint8 CUDA tensor [F, H, W, 3] (contiguous rows).  Returns
        (out [F, out_stride] uint8 CUDA tensor, sizes [F] int64 CUDA tensor).  Asynchronous
        on the current torch stream."""
        import torch
        self._check_frames(frames)
        f, h, w, _ = frames.shape
        # header None: the C-ABI's NULL / 0 -- every stream starts directly with its entropy-coded data (the call
        # shape of INTEGRATION.md section B, where the reference has written SOI..SOS itself)
        hdr_len = 0 if header is None else len(header)
        if out_stride is None:
            out_stride = frame_bound(w, h, yuv_mode, hdr_len)
        if out is None:
            out = torch.empty((f, out_stride), dtype=torch.uint8, device=frames.device)
        if sizes is None:
            sizes = torch.zeros(f, dtype=torch.int64, device=frames.device)
        rc = lib().sjpeg_hip_encode_scan(self._h, frames.data_ptr(), frames.stride(1),
                                         frames.stride(0), w, h, yuv_mode, f, C.byref(tables),
                                         header, hdr_len, int(append_eoi), out.data_ptr(),
                                         out_stride, sizes.data_ptr(), self._stream())
        if rc != 0:
            raise SjpegError(f"sjpeg_hip_encode_scan: {lib().sjpeg_hip_last_error().decode()}")
        return out, sizes

    def encode_frames_packed(self, frames, tables: ScanTables, header: bytes, yuv_mode: int,
                             out, sizes, offsets, out_stride, append_eoi=True):
        """sjpeg_hip_encode_scan_packed_src: like encode_frames(), but frame k is written at out + offsets[k], the
        frames back to back at multiples of 16 (what compact_streams() makes of a strided batch, without the extra
        pass).  out: flat uint8 CUDA tensor of at least F * out_stride bytes (16-byte aligned; it may be longer --
        the root of an exchange codes straight into the buffer the other ranks' streams are gathered behind),
        sizes [F] int64, offsets [F + 1] int64, out_stride a multiple of 16 = what one frame may take."""
        self._check_frames(frames)
        f, h, w, _ = frames.shape
        assert out.is_cuda and out.dtype.itemsize == 1 and out.numel() >= f * out_stride and offsets.numel() >= f + 1
        src, _ = make_source(SRC_RGB, [frames.view(f, h, w * 3)])
        rc = lib().sjpeg_hip_encode_scan_packed_src(self._h, C.byref(src), w, h, yuv_mode, f, C.byref(tables), header,
                                                    len(header), int(append_eoi), out.data_ptr(), int(out_stride),
                                                    sizes.data_ptr(), offsets.data_ptr(), self._stream())
        if rc != 0:
            raise SjpegError(f"sjpeg_hip_encode_scan_packed_src: {lib().sjpeg_hip_last_error().decode()}")
        return out, sizes, offsets

    # ---- any pixel source (sjpeg_hip_source) -------------------------------------------------
    def _chk(self, rc, what):
        if rc != 0:
            raise SjpegError(f"{what}: {lib().sjpeg_hip_last_error().decode()}")

    def encode_source(self, src: Source, nframes, w, h, tables: ScanTables, header: bytes, yuv_mode,
                      out_stride=None, append_eoi=True, device="cuda"):
        import torch
        if out_stride is None:
            out_stride = frame_bound(w, h, yuv_mode, len(header))
        out = torch.empty((nframes, out_stride), dtype=torch.uint8, device=device)
        sizes = torch.zeros(nframes, dtype=torch.int64, device=device)
        self._chk(lib().sjpeg_hip_encode_scan_src(self._h, C.byref(src), w, h, yuv_mode, nframes,
                                                  C.byref(tables), header, len(header),
                                                  int(append_eoi), out.data_ptr(), out_stride,
                                                  sizes.data_ptr(), self._stream()),
                  "sjpeg_hip_encode_scan_src")
        return out, sizes

    def scan_histogram_source(self, src: Source, nframes, w, h, yuv_mode, device="cuda"):
        import torch
        out = torch.zeros((nframes, 2, 64, 128), dtype=torch.int32, device=device)
        self._chk(lib().sjpeg_hip_scan_histogram_src(self._h, C.byref(src), w, h, yuv_mode, nframes,
                                                     out.data_ptr(), self._stream()),
                  "sjpeg_hip_scan_histogram_src")
        return out

    def scan_symbol_stats_source(self, src: Source, nframes, w, h, tables, yuv_mode, device="cuda"):
        import torch
        out = torch.zeros((nframes, 2, 272), dtype=torch.int32, device=device)
        self._chk(lib().sjpeg_hip_scan_symbol_stats_src(self._h, C.byref(src), w, h, yuv_mode, nframes,
                                                        C.byref(tables), out.data_ptr(), self._stream()),
                  "sjpeg_hip_scan_symbol_stats_src")
        return out

    def encode_source_multi(self, src: Source, nframes, w, h, tables_list, headers, yuv_mode,
                            out_stride=None, append_eoi=True, device="cuda"):
        """Frame f is coded with tables_list[f] and gets headers[f] in front (one launch)."""
        import torch
        assert len(tables_list) == nframes and len(headers) == nframes
        arr = (ScanTables * nframes)(*tables_list)
        offs = (C.c_size_t * (nframes + 1))()
        for i, hd in enumerate(headers):
            offs[i + 1] = offs[i] + len(hd)
        blob = b"".join(headers)
        if out_stride is None:
            out_stride = frame_bound(w, h, yuv_mode, max(len(hd) for hd in headers))
        out = torch.empty((nframes, out_stride), dtype=torch.uint8, device=device)
        sizes = torch.zeros(nframes, dtype=torch.int64, device=device)
        self._chk(lib().sjpeg_hip_encode_scan_multi(self._h, C.byref(src), w, h, yuv_mode, nframes,
                                                    C.cast(arr, C.c_void_p), blob, offs, int(append_eoi),
                                                    out.data_ptr(), out_stride, sizes.data_ptr(),
                                                    self._stream()),
                  "sjpeg_hip_encode_scan_multi")
        return out, sizes

    def scan_symbol_stats_multi(self, src: Source, nframes, w, h, tables_list, yuv_mode, device="cuda"):
        import torch
        assert len(tables_list) == nframes
        arr = (ScanTables * nframes)(*tables_list)
        out = torch.zeros((nframes, 2, 272), dtype=torch.int32, device=device)
        self._chk(lib().sjpeg_hip_scan_symbol_stats_multi(self._h, C.byref(src), w, h, yuv_mode, nframes,
                                                          C.cast(arr, C.c_void_p), out.data_ptr(),
                                                          self._stream()),
                  "sjpeg_hip_scan_symbol_stats_multi")
        return out

    def encode_batch(self, src: Source, nframes, w, h, yuv_mode, quant, method=4, min_quant=None, q_bias=0x78,
                     dmax_luma=12, dmax_chroma=1, out_stride=None, device="cuda", out=None, sizes=None):
        """The reference's per-picture analysis (methods 0..6) for a whole batch in one C call
        (sjpeg_hip_encode_batch_src).  Returns (out [F, stride] uint8, sizes [F] int64)."""
        import torch
        q = np.ascontiguousarray(quant, np.uint8).reshape(2, 64)
        mq = None if min_quant is None else np.ascontiguousarray(min_quant, np.uint8).reshape(2, 64)
        if out_stride is None:
            out_stride = frame_bound(w, h, yuv_mode, 2048)
        if out is None:
            out = torch.empty((nframes, out_stride), dtype=torch.uint8, device=device)
        if sizes is None:
            sizes = torch.zeros(nframes, dtype=torch.int64, device=device)
        self._chk(lib().sjpeg_hip_encode_batch_src(self._h, C.byref(src), w, h, yuv_mode, nframes, q.ctypes.data,
                                                   mq.ctypes.data if mq is not None else None, q_bias, int(method),
                                                   dmax_luma, dmax_chroma, out.data_ptr(), out_stride,
                                                   sizes.data_ptr(), self._stream()),
                  "sjpeg_hip_encode_batch_src")
        return out, sizes

    def scan_quant_error_source(self, src: Source, nframes, w, h, tables, yuv_mode, device="cuda"):
        import torch
        out = torch.zeros(nframes, dtype=torch.int64, device=device)
        self._chk(lib().sjpeg_hip_scan_quant_error_src(self._h, C.byref(src), w, h, yuv_mode, nframes,
                                                       C.byref(tables), out.data_ptr(), self._stream()),
                  "sjpeg_hip_scan_quant_error_src")
        return out

    def encode_band(self, src: Source, w, h, tables: ScanTables, yuv_mode, seg_begin, seg_end,
                    cap_words=None, device="cuda"):
        """One band of a frame shared between GPUs (include/sjpeg_hip.h): un-stuffed bit string
        (int32 tensor of MSB-first words) + its length in bits (int64 tensor [1])."""
        import torch
        need = band_bound(w, h, yuv_mode, seg_begin, seg_end)
        cap_words = need if cap_words is None else cap_words
        words = torch.zeros(cap_words, dtype=torch.int32, device=device)
        nbits = torch.zeros(1, dtype=torch.int64, device=device)
        self._chk(lib().sjpeg_hip_encode_band_src(self._h, C.byref(src), w, h, yuv_mode, C.byref(tables),
                                                  seg_begin, seg_end, words.data_ptr(), cap_words,
                                                  nbits.data_ptr(), self._stream()),
                  "sjpeg_hip_encode_band_src")
        return words, nbits

    def encode_intervals(self, src: Source, w, h, tables: ScanTables, yuv_mode, seg_begin, seg_end,
                         out_cap=None, device="cuda"):
        """Restart mode: the restart intervals [seg_begin, seg_end) of one frame as stuffed bytes with
        their RSTn markers (sjpeg_hip_encode_intervals_src).  Returns (out uint8 [out_cap], size int64 [1])."""
        import torch
        if out_cap is None:
            out_cap = 4 * band_bound(w, h, yuv_mode, seg_begin, seg_end) * 2 + 4096
        out = torch.empty(int(out_cap), dtype=torch.uint8, device=device)
        size = torch.zeros(1, dtype=torch.int64, device=device)
        self._chk(lib().sjpeg_hip_encode_intervals_src(self._h, C.byref(src), w, h, yuv_mode, C.byref(tables),
                                                       seg_begin, seg_end, C.c_void_p(out.data_ptr()),
                                                       C.c_size_t(int(out_cap)), C.c_void_p(size.data_ptr()),
                                                       self._stream()),
                  "sjpeg_hip_encode_intervals_src")
        return out, size

    def stitch_bands(self, words, nbits, header: bytes, append_eoi=True, out_cap=None):
        """words [nbands, stride] int32, nbits [nbands] int64 (this engine's device) -> JPEG bytes."""
        import torch
        assert words.dim() == 2 and words.is_contiguous() and nbits.numel() == words.shape[0]
        nb, stride = words.shape
        if out_cap is None:
            out_cap = len(header) + 2 * 4 * nb * stride + 4096
        out = torch.empty(out_cap, dtype=torch.uint8, device=words.device)
        size = torch.zeros(1, dtype=torch.int64, device=words.device)
        self._chk(lib().sjpeg_hip_stitch_bands(self._h, nb, words.data_ptr(), stride, nbits.data_ptr(),
                                               header, len(header), int(append_eoi), out.data_ptr(),
                                               out_cap, size.data_ptr(), self._stream()),
                  "sjpeg_hip_stitch_bands")
        n = int(size.item())
        if n == 0:
            raise SjpegError("sjpeg_hip_stitch_bands: output buffer too small")
        return bytes(out[:n].cpu().numpy())

    def entropy_bits(self, nframes):
        bits = np.zeros(nframes, np.uint64)
        self._chk(lib().sjpeg_hip_engine_entropy_bits(self._h, bits.ctypes.data, nframes),
                  "sjpeg_hip_engine_entropy_bits")
        return bits

    def scan_histogram(self, frames, yuv_mode: int):
        """[F, 2, 64, 128] uint32 (as int32 tensor) coefficient histograms (adaptive quantization)."""
        import torch
        f, h, w, _ = frames.shape
        out = torch.zeros((f, 2, 64, 128), dtype=torch.int32, device=frames.device)
        self._check_frames(frames)
        rc = lib().sjpeg_hip_scan_histogram(self._h, frames.data_ptr(), frames.stride(1),
                                            frames.stride(0), w, h, yuv_mode, f, out.data_ptr(),
                                            self._stream())
        if rc != 0:
            raise SjpegError(f"sjpeg_hip_scan_histogram: {lib().sjpeg_hip_last_error().decode()}")
        return out

    def scan_symbol_stats(self, frames, tables: ScanTables, yuv_mode: int):
        """[F, 2, 272] symbol counts (256 AC + 16 DC per table) for Huffman optimisation."""
        import torch
        f, h, w, _ = frames.shape
        out = torch.zeros((f, 2, 272), dtype=torch.int32, device=frames.device)
        self._check_frames(frames)
        rc = lib().sjpeg_hip_scan_symbol_stats(self._h, frames.data_ptr(), frames.stride(1),
                                               frames.stride(0), w, h, yuv_mode, f, C.byref(tables),
                                               out.data_ptr(), self._stream())
        if rc != 0:
            raise SjpegError(f"sjpeg_hip_scan_symbol_stats: {lib().sjpeg_hip_last_error().decode()}")
        return out

    def scan_coeffs(self, frames, tables: ScanTables, yuv_mode: int):
        import torch
        f, h, w, _ = frames.shape
        px = 16 if yuv_mode == YUV_420 else 8
        per = {YUV_420: 6, YUV_444: 3, YUV_400: 1}[yuv_mode]
        nb = ((w + px - 1) // px) * ((h + px - 1) // px) * per
        coeffs = torch.zeros((f, nb, 64), dtype=torch.int16, device=frames.device)
        self._check_frames(frames)
        rc = lib().sjpeg_hip_scan_coeffs(self._h, frames.data_ptr(), frames.stride(1),
                                         frames.stride(0), w, h, yuv_mode, f, C.byref(tables),
                                         coeffs.data_ptr(), self._stream())
        if rc != 0:
            raise SjpegError(f"sjpeg_hip_scan_coeffs: {lib().sjpeg_hip_last_error().decode()}")
        return coeffs

    def encode_ragged(self, fmt, planes_per_frame, dims, yuv_mode, tables, headers=None, append_eoi=True,
                      capacities=None, out=None, offsets=None, sizes=None):
        """sjpeg_hip_encode_ragged_src: pictures of different sizes in one call.  planes_per_frame[k]: the CUDA uint8
        tensors of frame k laid out as `fmt` says ([rows, row_bytes] each, any row stride), or (device address of
        row 0, row stride in bytes) pairs -- a negative stride codes rows stored bottom-up;
        dims[k] = (w, h).  tables: one ScanTables for every frame, or a list of one per frame (per-frame quality).
        headers: None or one header (bytes) per frame.  capacities[k] (default: frame_bound) are the bytes frame k may
        take.  Returns (out, sizes, offsets): out a flat uint8 CUDA tensor, frame k's JPEG at out[offsets[k]:
        offsets[k] + sizes[k]], sizes an int64 CUDA tensor (0: the frame did not fit), offsets a list of ints.
        Asynchronous on the current torch stream."""
        n = len(dims)
        if n == 0 or len(planes_per_frame) != n:
            raise SjpegError("encode_ragged: one entry of planes_per_frame and dims per frame, at least one frame")
        per_frame = isinstance(tables, (list, tuple))
        if per_frame and len(tables) != n:
            raise SjpegError("encode_ragged: one ScanTables per frame")
        if headers is not None and len(headers) != n:
            raise SjpegError("encode_ragged: one header per frame")
        if capacities is None:
            capacities = [frame_bound(w, h, yuv_mode, 0 if headers is None else len(headers[k]))
                          for k, (w, h) in enumerate(dims)]
        frames, out, sizes, offsets = _ragged_frames(planes_per_frame, dims, capacities, out, offsets, sizes)
        if per_frame:
            tarr = (ScanTables * n)(*tables)
        else:
            tarr = (ScanTables * 1)(tables)
        if headers is not None:
            hoffs = (C.c_size_t * (n + 1))()
            for i, hd in enumerate(headers):
                hoffs[i + 1] = hoffs[i] + len(hd)
            blob, hp = b"".join(headers), hoffs
        else:
            blob, hp = None, None
        self._chk(lib().sjpeg_hip_encode_ragged_src(self._h, fmt, yuv_mode, n, frames, C.cast(tarr, C.c_void_p),
                                                    int(per_frame), blob, C.cast(hp, C.c_void_p) if hp else None,
                                                    int(append_eoi), out.data_ptr(), sizes.data_ptr(),
                                                    self._stream()),
                  "sjpeg_hip_encode_ragged_src")
        return out, sizes, list(offsets)

    def scan_histogram_ragged(self, fmt, planes_per_frame, dims, yuv_mode):
        """sjpeg_hip_scan_histogram_ragged_src: the adaptive-quantization histograms of pictures of different sizes in
        one call (planes_per_frame, dims as encode_ragged).  Returns an int32 CUDA tensor [F, 2, 64, 128] (uint32 counts),
        frame k's what scan_histogram_source makes of it alone.  Asynchronous on the current torch stream."""
        import torch
        frames, _, _, _ = _ragged_frames(planes_per_frame, dims, None, None, None, None)
        out = torch.zeros((len(dims), 2, 64, 128), dtype=torch.int32, device=_ragged_device(planes_per_frame))
        self._chk(lib().sjpeg_hip_scan_histogram_ragged_src(self._h, fmt, yuv_mode, len(dims), frames, out.data_ptr(),
                                                            self._stream()),
                  "sjpeg_hip_scan_histogram_ragged_src")
        return out

    def scan_symbol_stats_ragged(self, fmt, planes_per_frame, dims, yuv_mode, tables):
        """sjpeg_hip_scan_symbol_stats_ragged_src: the symbol counts of pictures of different sizes in one call, with one
        ScanTables for every frame or a list of one per frame.  Returns an int32 CUDA tensor [F, 2, 272] (uint32 counts),
        frame k's what scan_symbol_stats_source makes of it alone.  Asynchronous on the current torch stream."""
        import torch
        n = len(dims)
        per_frame = isinstance(tables, (list, tuple))
        if per_frame and len(tables) != n:
            raise SjpegError("scan_symbol_stats_ragged: one ScanTables per frame")
        tarr = (ScanTables * n)(*tables) if per_frame else (ScanTables * 1)(tables)
        frames, _, _, _ = _ragged_frames(planes_per_frame, dims, None, None, None, None)
        out = torch.zeros((n, 2, 272), dtype=torch.int32, device=_ragged_device(planes_per_frame))
        self._chk(lib().sjpeg_hip_scan_symbol_stats_ragged_src(self._h, fmt, yuv_mode, n, frames, C.cast(tarr, C.c_void_p),
                                                               int(per_frame), out.data_ptr(), self._stream()),
                  "sjpeg_hip_scan_symbol_stats_ragged_src")
        return out

    def encode_ragged_batch(self, fmt, planes_per_frame, dims, yuv_mode, quant, method=4, min_quant=None, q_bias=0x78,
                            dmax_luma=12, dmax_chroma=1, capacities=None, out=None, offsets=None, sizes=None):
        """sjpeg_hip_encode_ragged_batch_src: the reference's per-picture analysis (methods 0..6) over pictures of
        different sizes in one call -- complete JPEGs.  planes_per_frame, dims, capacities, offsets, out, sizes as
        encode_ragged (capacities default: frame_bound(w, h, yuv_mode, 2048)); quant: one [2][64] starting matrix for
        every frame or a list of one per frame.  Frame k's bytes are what encode_batch makes of it alone.  Returns (out,
        sizes, offsets) as encode_ragged; the host waits inside for the analysis, the encode is asynchronous."""
        n = len(dims)
        if n == 0 or len(planes_per_frame) != n:
            raise SjpegError("encode_ragged_batch: one entry of planes_per_frame and dims per frame, at least one frame")
        q, per_frame, mq, _, _, capacities = _ragged_args("encode_ragged_batch", n, quant, min_quant, None, yuv_mode,
                                                          capacities, dims)
        frames, out, sizes, offsets = _ragged_frames(planes_per_frame, dims, capacities, out, offsets, sizes)
        self._chk(lib().sjpeg_hip_encode_ragged_batch_src(self._h, fmt, yuv_mode, n, frames, q.ctypes.data, int(per_frame),
                                                          mq.ctypes.data if mq is not None else None, q_bias, int(method),
                                                          dmax_luma, dmax_chroma, out.data_ptr(), sizes.data_ptr(),
                                                          self._stream()),
                  "sjpeg_hip_encode_ragged_batch_src")
        return out, sizes, list(offsets)

    def _ragged_tables(self, n, tables, what):
        per_frame = isinstance(tables, (list, tuple))
        if per_frame and len(tables) != n:
            raise SjpegError(f"{what}: one ScanTables per frame")
        return ((ScanTables * n)(*tables) if per_frame else (ScanTables * 1)(tables)), per_frame

    def scan_quant_error_ragged(self, fmt, planes_per_frame, dims, yuv_mode, tables):
        """sjpeg_hip_scan_quant_error_ragged_src: the quantization error of pictures of different sizes in one call, with
        one ScanTables for every frame or a list of one per frame.  Returns an int64 CUDA tensor [F] (uint64 totals),
        frame k's what scan_quant_error_source makes of it alone.  Asynchronous on the current torch stream."""
        import torch
        n = len(dims)
        tarr, per_frame = self._ragged_tables(n, tables, "scan_quant_error_ragged")
        frames, _, _, _ = _ragged_frames(planes_per_frame, dims, None, None, None, None)
        out = torch.zeros(n, dtype=torch.int64, device=_ragged_device(planes_per_frame))
        self._chk(lib().sjpeg_hip_scan_quant_error_ragged_src(self._h, fmt, yuv_mode, n, frames, C.cast(tarr, C.c_void_p),
                                                              int(per_frame), out.data_ptr(), self._stream()),
                  "sjpeg_hip_scan_quant_error_ragged_src")
        return out

    def scan_counted_bits_ragged(self, fmt, planes_per_frame, dims, yuv_mode, tables):
        """sjpeg_hip_scan_counted_bits_ragged_src: what the reference's BitCounter reports for the scan of each picture
        with its tables (entropy bits + 8 per 0xFF among the completed bytes), pictures of different sizes in one call.
        Returns an int64 CUDA tensor [F].  The host waits inside once (which frames overflowed the first plan)."""
        import torch
        n = len(dims)
        tarr, per_frame = self._ragged_tables(n, tables, "scan_counted_bits_ragged")
        frames, _, _, _ = _ragged_frames(planes_per_frame, dims, None, None, None, None)
        out = torch.zeros(n, dtype=torch.int64, device=_ragged_device(planes_per_frame))
        self._chk(lib().sjpeg_hip_scan_counted_bits_ragged_src(self._h, fmt, yuv_mode, n, frames, C.cast(tarr, C.c_void_p),
                                                               int(per_frame), out.data_ptr(), self._stream()),
                  "sjpeg_hip_scan_counted_bits_ragged_src")
        return out

    def encode_ragged_search(self, fmt, planes_per_frame, dims, yuv_mode, quant, search, method=4, min_quant=None,
                             q_bias=0x78, dmax_luma=12, dmax_chroma=1, capacities=None, out=None, offsets=None,
                             sizes=None):
        """sjpeg_hip_encode_ragged_search_src: encode_ragged_batch with the reference's multi-pass search to a target
        size (bytes) or PSNR (dB) per picture.  search: one SearchParams (or dict of its fields) for every frame, or a
        list of one per frame.  Frame k's bytes are what sjpeg::Encode makes of it alone with its starting matrix,
        Huffman_compress = method not in (0, 3), adaptive_quantization = method >= 3 and its search fields.  Returns
        (out, sizes, offsets, q, value): q[k] / value[k] the SearchHook's best q and result, -1 where the frame was not
        searched (passes <= 1).  The host waits inside once or twice per pass; the final encode is asynchronous."""
        n = len(dims)
        if n == 0 or len(planes_per_frame) != n:
            raise SjpegError("encode_ragged_search: one entry of planes_per_frame and dims per frame, at least one frame")
        q, per_frame, mq, sarr, search_per_frame, capacities = _ragged_args("encode_ragged_search", n, quant, min_quant,
                                                                            search, yuv_mode, capacities, dims)
        frames, out, sizes, offsets = _ragged_frames(planes_per_frame, dims, capacities, out, offsets, sizes)
        q_out, v_out = (C.c_float * n)(), (C.c_float * n)()
        self._chk(lib().sjpeg_hip_encode_ragged_search_src(self._h, fmt, int(yuv_mode), n, frames, q.ctypes.data,
                                                           int(per_frame), mq.ctypes.data if mq is not None else None,
                                                           q_bias, int(method), dmax_luma, dmax_chroma, sarr,
                                                           int(search_per_frame), q_out, v_out, out.data_ptr(),
                                                           sizes.data_ptr(), self._stream()),
                  "sjpeg_hip_encode_ragged_search_src")
        return out, sizes, list(offsets), [float(x) for x in q_out], [float(x) for x in v_out]

    def riskiness_ragged(self, fmt, planes_per_frame, dims, table=None):
        """sjpeg_hip_riskiness_ragged_src: the three riskiness sums of pictures of different sizes in one call (fmt:
        SRC_RGB / SRC_BGRA / SRC_RGBA; planes_per_frame, dims as encode_ragged).  table: the 117649-byte score table
        (bytes or a CUDA uint8 tensor; default None: the table SjpegRiskiness uses -- set_riskiness_table,
        SJPEG_HIP_RISKINESS_TABLE, riskiness.bin beside the library).  Returns an int64 CUDA tensor [F, 3],
        frame k's what sjpeg_hip_riskiness_sums makes of it alone.  Asynchronous on the current torch stream."""
        import torch
        dev = _ragged_device(planes_per_frame)
        d_table = None
        if table is not None:
            d_table = table if isinstance(table, torch.Tensor) else \
                torch.frombuffer(bytearray(table), dtype=torch.uint8).to(dev)
        frames, _, _, _ = _ragged_frames(planes_per_frame, dims, None, None, None, None)
        sums = torch.zeros((len(dims), 3), dtype=torch.int64, device=dev)
        self._chk(lib().sjpeg_hip_riskiness_ragged_src(self._h, fmt, len(dims), frames,
                                                       d_table.data_ptr() if d_table is not None else None,
                                                       sums.data_ptr(), self._stream()),
                  "sjpeg_hip_riskiness_ragged_src")
        return sums

    def sharp_yuv_ragged(self, fmt, planes_per_frame, dims):
        """sjpeg_hip_sharp_yuv_ragged: the sharp conversion of pictures of different sizes in one call.  Returns a list
        of (y [H, W], u [ch, cw], v [ch, cw]) uint8 CUDA tensors, frame k's what sharp_yuv makes of it alone.
        Asynchronous on the current torch stream."""
        import torch
        n = len(dims)
        dev = _ragged_device(planes_per_frame)
        frames, _, _, _ = _ragged_frames(planes_per_frame, dims, None, None, None, None)
        planes = []
        for (w, h) in dims:
            cw, ch = (w + 1) // 2, (h + 1) // 2
            planes.append((torch.empty((h, w), dtype=torch.uint8, device=dev),
                           torch.empty((ch, cw), dtype=torch.uint8, device=dev),
                           torch.empty((ch, cw), dtype=torch.uint8, device=dev)))
        ptrs = [(C.c_void_p * n)(*[p[i].data_ptr() for p in planes]) for i in range(3)]
        wsz = lib().sjpeg_hip_sharp_ragged_workspace(n, frames)
        work = torch.empty(max(int(wsz), 16), dtype=torch.uint8, device=dev)
        self._chk(lib().sjpeg_hip_sharp_yuv_ragged(self._h, fmt, n, frames, ptrs[0], ptrs[1], ptrs[2], work.data_ptr(),
                                                   wsz, self._stream()),
                  "sjpeg_hip_sharp_yuv_ragged")
        self._keep = (work, planes)                  # (alive until the stream has used them)
        return planes

    def encode_ragged_auto(self, fmt, planes_per_frame, dims, yuv_mode, quant, method=4, min_quant=None, q_bias=0x78,
                           dmax_luma=12, dmax_chroma=1, capacities=None, out=None, offsets=None, sizes=None):
        """sjpeg_hip_encode_ragged_auto_src: encode_ragged_batch with the SjpegYUVMode of EncoderParam -- YUV_AUTO (the
        riskiness of every frame decides), YUV_SHARP, or YUV_420 / 444 / 400 (= encode_ragged_batch).  Frame k's bytes
        are what SjpegEncode(picture, q, method, yuv_mode) makes of it alone.  capacities default:
        frame_bound(w, h, YUV_444, 2048).  Returns (out, sizes, offsets, modes): modes[k] the SjpegYUVMode frame k was
        coded with (YUV_SHARP for sharp frames).  The host waits inside for the analysis; the encode is asynchronous."""
        return self._encode_ragged_modes("encode_ragged_auto", "sjpeg_hip_encode_ragged_auto_src", fmt, planes_per_frame,
                                         dims, yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma,
                                         capacities, out, offsets, sizes)

    def encode_ragged_trellis(self, fmt, planes_per_frame, dims, yuv_mode, quant, method=7, min_quant=None, q_bias=0x78,
                              dmax_luma=12, dmax_chroma=1, capacities=None, out=None, offsets=None, sizes=None):
        """sjpeg_hip_encode_ragged_trellis_src: the reference's trellis methods 7 (= 4 + trellis) and 8 (= 6 + trellis)
        over a ragged batch.  Arguments and result as encode_ragged_auto: any SjpegYUVMode (YUV_AUTO and YUV_SHARP for
        RGB / BGRA / RGBA sources), frame k's bytes what SjpegEncode(picture, q, method, yuv_mode) makes of it alone.
        The trellis runs once per picture: the statistics pass keeps its quantized blocks in the engine's scratch
        (36 864 bytes a segment, counted against SJPEG_HIP_SCRATCH_LIMIT_BYTES) and the encode pass replays them."""
        return self._encode_ragged_modes("encode_ragged_trellis", "sjpeg_hip_encode_ragged_trellis_src", fmt,
                                         planes_per_frame, dims, yuv_mode, quant, method, min_quant, q_bias, dmax_luma,
                                         dmax_chroma, capacities, out, offsets, sizes)

    def _encode_ragged_modes(self, who, symbol, fmt, planes_per_frame, dims, yuv_mode, quant, method, min_quant, q_bias,
                             dmax_luma, dmax_chroma, capacities, out, offsets, sizes):
        n = len(dims)
        if n == 0 or len(planes_per_frame) != n:
            raise SjpegError(f"{who}: one entry of planes_per_frame and dims per frame, at least one frame")
        q, per_frame, mq, _, _, capacities = _ragged_args(who, n, quant, min_quant, None, YUV_444, capacities, dims)
        frames, out, sizes, offsets = _ragged_frames(planes_per_frame, dims, capacities, out, offsets, sizes)
        modes = (C.c_int * n)()
        self._chk(getattr(lib(), symbol)(self._h, fmt, int(yuv_mode), n, frames, q.ctypes.data, int(per_frame),
                                         mq.ctypes.data if mq is not None else None, q_bias, int(method), dmax_luma,
                                         dmax_chroma, out.data_ptr(), sizes.data_ptr(), modes, self._stream()),
                  symbol)
        return out, sizes, list(offsets), [int(m) for m in modes]

    def encode_ragged_packed(self, fmt, planes_per_frame, dims, yuv_mode, quant, method=4, min_quant=None, q_bias=0x78,
                             dmax_luma=12, dmax_chroma=1, search=None, capacities=None, packed_capacity=None, out=None):
        """sjpeg_hip_encode_ragged_packed_src: any ragged encode (encode_ragged_batch / _auto / _trellis / _search by
        the same arguments) with the frames written back to back into ONE buffer -- each at a multiple of 16, zero
        padding, the format Comm.gather_streams takes.  capacities: the most each frame may take (default:
        frame_bound(w, h, mode, 2048), mode YUV_444 for YUV_AUTO / YUV_SHARP); packed_capacity: bytes of `out`
        (default: len(out), or the capacities' sum, which always fits); out: a uint8 CUDA tensor at a multiple of 16.
        Returns (out, sizes, offsets, modes) -- sizes [n] and offsets [n + 1] int64 CUDA tensors (views of one tensor)
        by the caller's frame numbers, offsets[n] the bytes used, or with PACKED_OVERFLOW (bit 63: the int64 is
        negative) the bytes a second try needs; a frame that was dropped has size 0 -- and, with a search,
        (..., q, value) as encode_ragged_search.  The encode is asynchronous on the current torch stream."""
        res = self._encode_ragged_packed(fmt, planes_per_frame, dims, yuv_mode, quant, method, min_quant, q_bias, dmax_luma,
                                         dmax_chroma, search, capacities, packed_capacity, out)
        return res[:4] if search is None else res

    def _full_call(self, who, n, dims, yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search, capacities,
                   metadata, factors=None, sizes=None, orientations=None, resized=False):
        """What every full-style entry hands to the library, built once: the metadata array, the arrays of the factors,
        sizes and orientations an entry takes, the default capacities -- the bounds of the pictures as they are CODED
        (reduced by factors[k]; sizes[k], for an entry that resizes clamped into 1..65535; swapped for the orientations
        5..8), each with room for its metadata; or what the function `capacities` makes of the metadata sizes --, the
        quant, min_quant and search arrays, sjpeg_hip_ragged_params and the three result arrays.  n and dims count what
        is coded with params (the sheets of a sheet entry).  The result keeps alive what the structures point into."""
        bound_mode = _bound_mode(yuv_mode)
        marr, meta_per_frame, msizes, mkeep = _metadata_args(who, n, metadata)
        fac = None if factors is None else (C.c_uint8 * n)(*[min(max(int(f), 0), 255) for f in factors])
        arr, oarr = _shape_arrays(who, n, sizes, orientations)
        if callable(capacities):
            capacities = capacities(msizes)
        if capacities is None:
            capacities = []
            for k, (w, h) in enumerate(dims if arr is None else arr.tolist()):
                if factors is not None:
                    f = max(min(int(factors[k]), REDUCE_MAX), 1)
                    w, h = -(-w // f), -(-h // f)
                if resized:
                    w, h = min(max(int(w), 1), 65535), min(max(int(h), 1), 65535)
                if oarr is not None and oarr[k] >= 5:
                    w, h = h, w
                capacities.append(frame_bound(w, h, bound_mode, 2048 + msizes[k]))
        q, per_frame, mq, sarr, search_per_frame, capacities = _ragged_args(who, n, quant, min_quant, search, bound_mode,
                                                                            capacities, dims)
        params = RaggedParams(int(yuv_mode), int(method), q.ctypes.data, int(per_frame),
                              mq.ctypes.data if mq is not None else None, int(q_bias), int(dmax_luma), int(dmax_chroma),
                              sarr, int(search_per_frame))
        return _FullCall(C.byref(params), None if fac is None else C.cast(fac, C.c_void_p), _address(arr), _address(oarr),
                         (None if marr is None else C.cast(marr, C.c_void_p), meta_per_frame), capacities,
                         ((C.c_int * n)(), (C.c_float * n)(), (C.c_float * n)()), (params, q, mq, sarr, marr, mkeep, fac, arr, oarr))

    def _call_shaped(self, symbol, fmt, frames, call, segments, tail, outs):
        """the C call of a shaped encode: the head, params, the entry's segments by name, the call's metadata and the
        tail `tail` -- outs, then the result arrays and the stream"""
        values = dict(segments() if callable(segments) else segments, head=(self._h, fmt, len(frames), frames), params=call.params)
        values[tail] = outs + call.results + (self._stream(),)
        if call.meta != ():
            values["meta"] = call.meta
        self._chk(_binding.call(lib(), symbol, values), symbol)

    def _encode_shaped(self, who, stem, fmt, planes_per_frame, dims, call, segments, packed, out=None, offsets=None,
                       sizes_out=None, packed_capacity=None, one_tensor=False):
        """The one body of "encode shaped pictures": sjpeg_hip_encode_ragged_<stem>_src, or packed its _packed_src twin
        (stem "": sjpeg_hip_encode_ragged_packed_src, the one entry without a family's name), with the call
        Engine._full_call built and the family's segments by name (a function of no arguments where they are to be made
        once the output stands).  Returns (out, sizes, offsets, modes, q, value) -- unpacked: offsets a list; packed:
        sizes [n] and offsets [n + 1] views of ONE int64 device tensor (one_tensor: that tensor in their place)."""
        n = len(dims)
        symbol = "sjpeg_hip_encode_ragged" + (f"_{stem}" if stem else "") + ("_packed_src" if packed else "_src")
        if not packed:
            frames, out, sizes_out, offsets = _ragged_frames(planes_per_frame, dims, call.capacities, out, offsets, sizes_out)
            self._call_shaped(symbol, fmt, frames, call, segments, "unpacked", (out.data_ptr(), sizes_out.data_ptr()))
            return (out, sizes_out, list(offsets)) + call.answers()
        out, packed_capacity, meta = _packed_out(who, n, planes_per_frame, call.capacities, packed_capacity, out)
        frames, _, _, _ = _ragged_frames(planes_per_frame, dims, call.capacities, out, [0] * n, meta)   # (out_offset ignored)
        self._call_shaped(symbol, fmt, frames, call, segments, "packed",
                          (out.data_ptr(), packed_capacity, meta.data_ptr() + 8 * n, meta.data_ptr()))
        return ((out, meta) if one_tensor else (out, meta[:n], meta[n:])) + call.answers()

    def _encode_sheets_shaped(self, who, stem, fmt, planes_per_frame, dims, ns, call, segments, packed, out_stride=None, out=None,
                              packed_capacity=None):
        """... and of "encode contact sheets": sjpeg_hip_encode_ragged_<stem>_src / _packed_src with what Engine._sheet_call
        built.  params, the metadata and the results count the ns SHEETS; the unpacked form writes sheet s at s * out_stride."""
        import torch
        frames, _, _, _ = _ragged_frames(planes_per_frame, dims, None, None, None, None)
        if packed:
            out, packed_capacity, meta = _packed_out(who, ns, planes_per_frame, call.capacities, packed_capacity, out)
            self._call_shaped(f"sjpeg_hip_encode_ragged_{stem}_packed_src", fmt, frames, call, segments, "packed",
                              (out.data_ptr(), packed_capacity, meta.data_ptr() + 8 * ns, meta.data_ptr()))
            return (out, meta[:ns], meta[ns:]) + call.answers()
        out_stride = (call.capacities[0] + 15) & ~15 if out_stride is None else int(out_stride)
        dev = _ragged_device(planes_per_frame)
        if out is None:
            out = torch.empty(max(out_stride * ns, 1), dtype=torch.uint8, device=dev)
        if out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.numel() < out_stride * ns:
            raise SjpegError(f"{who}: out must be a contiguous uint8 CUDA tensor of out_stride bytes a sheet")
        sizes_out = torch.zeros(ns, dtype=torch.int64, device=dev)
        self._call_shaped(f"sjpeg_hip_encode_ragged_{stem}_src", fmt, frames, call, segments, "strided",
                          (out.data_ptr(), out_stride, sizes_out.data_ptr()))
        return (out, sizes_out, [s * out_stride for s in range(ns)]) + call.answers()

    def _encode_ragged_packed(self, fmt, planes_per_frame, dims, yuv_mode, quant, method, min_quant, q_bias, dmax_luma,
                              dmax_chroma, search, capacities, packed_capacity, out, stem="", metadata=None, one_tensor=False):
        """encode_ragged_packed (one_tensor: sizes and offsets as ONE int64 tensor [2 n + 1], which one copy brings home).
        stem "": that entry point; "full": its twin sjpeg_hip_encode_ragged_full_packed_src (the same arguments); with
        metadata (as encode_ragged_full takes it) the twin's sjpeg_hip_encode_ragged_full_meta_packed_src."""
        n = len(dims)
        if n == 0 or len(planes_per_frame) != n:
            raise SjpegError("encode_ragged_packed: one entry of planes_per_frame and dims per frame, at least one frame")
        call = self._full_call("encode_ragged_packed", n, dims, yuv_mode, quant, method, min_quant, q_bias, dmax_luma,
                               dmax_chroma, search, capacities, metadata)
        if len(call.capacities) != n:
            raise SjpegError("encode_ragged_packed: one capacity per frame")
        if call.meta[0] is None:
            call.meta = ()                       # (these entries have a form without the metadata arguments)
        else:
            stem = "full_meta"
        return self._encode_shaped("encode_ragged_packed", stem, fmt, planes_per_frame, dims, call, {}, True, out=out,
                                   packed_capacity=packed_capacity, one_tensor=one_tensor)

    def encode_ragged_full(self, fmt, planes_per_frame, dims, yuv_mode, quant, method=4, min_quant=None, q_bias=0x78,
                           dmax_luma=12, dmax_chroma=1, search=None, capacities=None, out=None, offsets=None, sizes=None,
                           metadata=None):
        """sjpeg_hip_encode_ragged_full_src: every combination of SjpegYUVMode 0..4, method 0..8 and a search (None, one
        SearchParams / dict, or a list of one per frame) in one ragged call.  Frame k's bytes are what the reference's
        sjpeg::Encode() makes of that picture alone.  What encode_ragged_batch / _auto / _trellis / _search take goes to
        their flows; a search with YUV_AUTO / YUV_SHARP, with method 7 or 8, or both, is this call's own.  Returns
        (out, sizes, offsets, modes, q, value): q / value -1 for a frame that was not searched (passes <= 1).
        metadata: None, one PictureMetadata for every picture or a sequence of one per picture (None entries: none) --
        sjpeg_hip_encode_ragged_full_meta_src: each JPEG carries its EXIF, ICC profile, XMP and APP markers as the
        reference writes them, a size search counts them, and the default capacities make room for them."""
        n = len(dims)
        if n == 0 or len(planes_per_frame) != n:
            raise SjpegError("encode_ragged_full: one entry of planes_per_frame and dims per frame, at least one frame")
        call = self._full_call("encode_ragged_full", n, dims, yuv_mode, quant, method, min_quant, q_bias, dmax_luma,
                               dmax_chroma, search, capacities, metadata)
        stem = "full_meta"
        if call.meta[0] is None:
            stem, call.meta = "full", ()         # (the form without the metadata arguments)
        return self._encode_shaped("encode_ragged_full", stem, fmt, planes_per_frame, dims, call, {}, False, out, offsets, sizes)

    def encode_ragged_full_packed(self, fmt, planes_per_frame, dims, yuv_mode, quant, method=4, min_quant=None,
                                  q_bias=0x78, dmax_luma=12, dmax_chroma=1, search=None, capacities=None,
                                  packed_capacity=None, out=None, metadata=None):
        """sjpeg_hip_encode_ragged_full_packed_src: encode_ragged_full into ONE packed buffer, with the arguments and
        the layout of encode_ragged_packed.  Returns (out, sizes, offsets, modes, q, value).  metadata: as
        encode_ragged_full (sjpeg_hip_encode_ragged_full_meta_packed_src)."""
        return self._encode_ragged_packed(fmt, planes_per_frame, dims, yuv_mode, quant, method, min_quant, q_bias, dmax_luma,
                                          dmax_chroma, search, capacities, packed_capacity, out, stem="full", metadata=metadata)

    def reduce_ragged(self, fmt, planes_per_frame, dims, factors, out=None):
        """sjpeg_hip_reduce_ragged_src: the pictures of a ragged batch (fmt, planes_per_frame, dims as encode_ragged; any
        RGB-like or gray format) reduced by factors[k] (1..8) in one launch.  Returns (reduced_fmt, pictures, buf):
        SRC_RGB with uint8 CUDA tensors [h', w', 3], or SRC_GRAY with [h', w'] -- views of the one buffer buf (rows
        padded to a multiple of 4 bytes, pictures at multiples of 16), which any ragged entry takes as its planes.  out:
        a uint8 CUDA tensor to reduce into (at a multiple of 16, at least the bytes needed).  Asynchronous on the current
        torch stream."""
        n = len(dims)
        if len(factors) != n:
            raise SjpegError("reduce_ragged: one factor per frame")
        frames, _, _, _ = _ragged_frames(planes_per_frame, dims, None, None, None, None)
        fac = (C.c_uint8 * n)(*[min(max(int(f), 0), 255) for f in factors])
        return self._make_pictures("reduce_ragged", "reduce_ragged", "reduce_ragged", fmt, planes_per_frame, frames,
                                   {"factors": C.cast(fac, C.c_void_p)}, {}, out)

    def _make_pictures(self, who, stem, bytes_stem, fmt, planes_per_frame, frames, shape, more, out, nsheets=None):
        """The one body of "make pictures": sjpeg_hip_<bytes_stem>_bytes on the segments `shape`, the buffer, then
        sjpeg_hip_<stem>_src on `shape` and `more` -- the segments the bytes do not depend on; a function of no arguments
        where they are to be made once the buffer stands --, and the return tuple
        (format, views, buffer).  nsheets: the most contact sheets a sheet entry may make (None: one picture a frame)."""
        n = len(frames)
        need = _binding.call(lib(), f"sjpeg_hip_{bytes_stem}_bytes", dict(shape, bytes_head=(fmt, n, frames)))
        out = _made_out(who, planes_per_frame, need, out)
        more = more() if callable(more) else more
        made, ns, rfmt = (RaggedFrame * (n if nsheets is None else nsheets))(), C.c_int(0), C.c_int(-1)
        # (a batch the library refuses has need == 0: the call below says why)
        tail = (out.data_ptr(), int(out.numel()) if need else 0, made) + (() if nsheets is None else (C.byref(ns),)) + \
            (C.byref(rfmt), self._stream())
        values = dict(shape, **more, head=(self._h, fmt, n, frames))
        values["pictures" if nsheets is None else "sheets"] = tail
        self._chk(_binding.call(lib(), f"sjpeg_hip_{stem}_src", values), f"sjpeg_hip_{stem}_src")
        return int(rfmt.value), _frame_views(out, made if nsheets is None else list(made)[:ns.value], rfmt.value), out

    def _encode_sized(self, who, stem, lists, fmt, planes_per_frame, dims, enc, packed, factors=None, sizes=None, orientations=None,
                      flatten=None, **outs):
        """The reduced, resized, oriented, flattened and YUV-resized encodes and their packed forms: the check of the
        per-frame lists (named `lists` in its text), the call with the bounds of the pictures as they are CODED, and the
        segments the entry takes.  enc: (yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search,
        capacities, metadata) as Engine._full_call takes them; outs: the caller's out, offsets, sizes_out, packed_capacity."""
        n = len(dims)
        given = factors if stem == "reduced" else sizes
        if n == 0 or len(planes_per_frame) != n or (given is not None and len(given) != n):
            raise SjpegError(f"{who}: one entry of planes_per_frame, {lists} per frame, at least one frame")
        call = self._full_call(who, n, dims, *enc, factors=factors, sizes=sizes, orientations=orientations, resized=stem != "reduced")
        pieces, keep = _binding.SHAPED[f"sjpeg_hip_encode_ragged_{stem}_src"][1], []

        def segments():
            values = {name: getattr(call, name) for name in ("factors", "sizes", "orientations") if name in pieces}
            if "flatten" in pieces:              # (the flattened entries: `flatten`, or NULL, behind params)
                values.update(_flatten_segment(who, flatten, keep))
            return values
        return self._encode_shaped(who, stem, fmt, planes_per_frame, dims, call, segments, packed, **outs)

    def encode_ragged_reduced(self, fmt, planes_per_frame, dims, factors, yuv_mode, quant, method=4, min_quant=None,
                              q_bias=0x78, dmax_luma=12, dmax_chroma=1, search=None, capacities=None, out=None,
                              offsets=None, sizes=None, metadata=None):
        """sjpeg_hip_encode_ragged_reduced_src: encode_ragged_full of the pictures reduced by factors[k] (1..8; None:
        all 1) inside the call -- the reduce kernel into engine memory, then one inner call over the reduced pictures.
        Frame k's bytes are those encode_ragged_full makes of the reduced uint8 picture (Engine.reduce_ragged returns
        it).  dims are the SOURCE sizes; the default capacities are the bounds of the reduced ones.  Returns
        (out, sizes, offsets, modes, q, value) as encode_ragged_full."""
        enc = (yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search, capacities, metadata)
        return self._encode_sized("encode_ragged_reduced", "reduced", "dims and factors", fmt, planes_per_frame, dims, enc, False,
                                  factors=factors, out=out, offsets=offsets, sizes_out=sizes)

    def encode_ragged_reduced_packed(self, fmt, planes_per_frame, dims, factors, yuv_mode, quant, method=4, min_quant=None,
                                     q_bias=0x78, dmax_luma=12, dmax_chroma=1, search=None, capacities=None,
                                     packed_capacity=None, out=None, metadata=None):
        """sjpeg_hip_encode_ragged_reduced_packed_src: encode_ragged_reduced into ONE packed buffer, with the arguments
        and the layout of encode_ragged_full_packed.  Returns (out, sizes, offsets, modes, q, value)."""
        enc = (yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search, capacities, metadata)
        return self._encode_sized("encode_ragged_reduced_packed", "reduced", "dims and factors", fmt, planes_per_frame, dims, enc, True,
                                  factors=factors, out=out, packed_capacity=packed_capacity)

    def resize_ragged(self, fmt, planes_per_frame, dims, sizes, out=None):
        """sjpeg_hip_resize_ragged_src: the pictures of a ragged batch (fmt, planes_per_frame, dims as encode_ragged; any
        RGB-like or gray format) resized to sizes[k] = (w, h), each side 1..the source's, in one launch.  Returns
        (resized_fmt, pictures, buf) as reduce_ragged does, with the same layout of buf; out as there."""
        n = len(dims)
        if len(sizes) != n:
            raise SjpegError("resize_ragged: one size per frame")
        frames, _, _, _ = _ragged_frames(planes_per_frame, dims, None, None, None, None)
        arr = _sizes_array("resize_ragged", sizes)
        return self._make_pictures("resize_ragged", "resize_ragged", "resize_ragged", fmt, planes_per_frame, frames,
                                   {"sizes": arr.ctypes.data}, {}, out)

    def encode_ragged_resized(self, fmt, planes_per_frame, dims, sizes, yuv_mode, quant, method=4, min_quant=None,
                              q_bias=0x78, dmax_luma=12, dmax_chroma=1, search=None, capacities=None, out=None,
                              offsets=None, sizes_out=None, metadata=None):
        """sjpeg_hip_encode_ragged_resized_src: encode_ragged_full of the pictures resized to sizes[k] = (w, h) (None:
        their own sizes) inside the call -- the resize kernel into engine memory, then one inner call over the resized
        pictures.  Frame k's bytes are those encode_ragged_full makes of the resized uint8 picture (Engine.resize_ragged
        returns it).  dims are the SOURCE sizes; the default capacities are the bounds of the resized ones; sizes_out:
        the `sizes` tensor of encode_ragged_full.  Returns (out, sizes, offsets, modes, q, value) as encode_ragged_full."""
        enc = (yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search, capacities, metadata)
        return self._encode_sized("encode_ragged_resized", "resized", "dims and sizes", fmt, planes_per_frame, dims, enc, False,
                                  sizes=sizes, out=out, offsets=offsets, sizes_out=sizes_out)

    def encode_ragged_resized_packed(self, fmt, planes_per_frame, dims, sizes, yuv_mode, quant, method=4, min_quant=None,
                                     q_bias=0x78, dmax_luma=12, dmax_chroma=1, search=None, capacities=None,
                                     packed_capacity=None, out=None, metadata=None):
        """sjpeg_hip_encode_ragged_resized_packed_src: encode_ragged_resized into ONE packed buffer, with the arguments
        and the layout of encode_ragged_full_packed.  Returns (out, sizes, offsets, modes, q, value)."""
        enc = (yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search, capacities, metadata)
        return self._encode_sized("encode_ragged_resized_packed", "resized", "dims and sizes", fmt, planes_per_frame, dims, enc, True,
                                  sizes=sizes, out=out, packed_capacity=packed_capacity)

    def orient_ragged(self, fmt, planes_per_frame, dims, sizes, orientations, out=None):
        """sjpeg_hip_orient_ragged_src: the pictures of a ragged batch resized to sizes[k] = (w, h) (None: their own
        sizes; the STORED orientation) and turned upright by orientations[k] (EXIF 1..8; None: all 1) in one launch.
        Returns (fmt, pictures, buf) as resize_ragged does: picture k is [h, w, 3] or [h, w] for 1..4, [w, h, ...] for
        5..8.  Row and picture padding of buf may hold anything."""
        return self._orient_ragged("orient_ragged", fmt, planes_per_frame, dims, {}, sizes, orientations, out)

    def flatten_ragged(self, fmt, planes_per_frame, dims, flatten, sizes=None, orientations=None, out=None):
        """sjpeg_hip_flatten_ragged_src: orient_ragged of pictures with an alpha channel (fmt SRC_BGRA, SRC_RGBA or
        SRC_RGBA_F32 / _F16 / _BF16), every pixel laid over the Flatten `flatten`'s background as its row is staged --
        flatten, resize and turn in ONE launch; sizes None and orientations None: the flattened pictures themselves.
        Returns (SRC_RGB, pictures, buf) as orient_ragged."""
        flat = _flatten_struct("flatten_ragged", flatten)
        return self._orient_ragged("flatten_ragged", fmt, planes_per_frame, dims, {"flatten": C.addressof(flat)}, sizes, orientations, out)

    def _orient_ragged(self, who, fmt, planes_per_frame, dims, more, sizes, orientations, out, bytes_stem="orient_ragged"):
        """orient_ragged, flatten_ragged (more: its struct sjpeg_hip_flatten) and resize_ragged_yuv: sjpeg_hip_<who>_src"""
        n = len(dims)
        if sizes is not None and len(sizes) != n:
            raise SjpegError(f"{who}: one size per frame")
        frames, _, _, _ = _ragged_frames(planes_per_frame, dims, None, None, None, None)
        arr, oarr = _shape_arrays(who, n, sizes, orientations)
        return self._make_pictures(who, who, bytes_stem, fmt, planes_per_frame, frames,
                                   {"sizes": _address(arr), "orientations": _address(oarr)}, more, out)

    def _oriented_call(self, who, planes_per_frame, dims, sizes, orientations, yuv_mode, quant, method, min_quant, q_bias,
                       dmax_luma, dmax_chroma, search, capacities, metadata):
        """what the encodes of resized and turned pictures share: their check, and the call with the bounds of the UPRIGHT
        sizes"""
        n = len(dims)
        if n == 0 or len(planes_per_frame) != n or (sizes is not None and len(sizes) != n):
            raise SjpegError(f"{who}: one entry of planes_per_frame, dims, sizes and orientations per frame, at least one frame")
        return self._full_call(who, n, dims, yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search,
                               capacities, metadata, sizes=sizes, orientations=orientations, resized=True)

    def encode_ragged_oriented(self, fmt, planes_per_frame, dims, sizes, orientations, yuv_mode, quant, method=4,
                               min_quant=None, q_bias=0x78, dmax_luma=12, dmax_chroma=1, search=None, capacities=None,
                               out=None, offsets=None, sizes_out=None, metadata=None):
        """sjpeg_hip_encode_ragged_oriented_src: encode_ragged_resized plus orientations[k] (EXIF 1..8; None: all 1) --
        the pictures resized and turned upright by the one kernel launch, then one inner call over the upright
        pictures.  Frame k's bytes are those encode_ragged_full makes of the upright uint8 picture (Engine.orient_ragged
        returns it).  sizes are in the STORED orientation (None: the pictures' own); the default capacities are the
        bounds of the upright sizes.  Returns (out, sizes, offsets, modes, q, value) as encode_ragged_full."""
        enc = (yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search, capacities, metadata)
        return self._encode_sized("encode_ragged_oriented", "oriented", "dims, sizes and orientations", fmt, planes_per_frame, dims, enc, False,
                                  sizes=sizes, orientations=orientations, out=out, offsets=offsets, sizes_out=sizes_out)

    def encode_ragged_flattened(self, fmt, planes_per_frame, dims, flatten, sizes, orientations, yuv_mode, quant, method=4,
                                min_quant=None, q_bias=0x78, dmax_luma=12, dmax_chroma=1, search=None, capacities=None,
                                out=None, offsets=None, sizes_out=None, metadata=None):
        """sjpeg_hip_encode_ragged_flattened_src: encode_ragged_oriented of pictures with an alpha channel laid over the
        Flatten `flatten`'s background in the same launch (None: exactly encode_ragged_oriented).  Frame k's bytes are
        those encode_ragged_full makes of the uint8 picture Engine.flatten_ragged returns; YUV_AUTO, a search and the
        metadata act on that picture.  Returns (out, sizes, offsets, modes, q, value)."""
        enc = (yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search, capacities, metadata)
        return self._encode_sized("encode_ragged_flattened", "flattened", "dims, sizes and orientations", fmt, planes_per_frame, dims, enc, False,
                                  sizes=sizes, orientations=orientations, flatten=flatten, out=out, offsets=offsets, sizes_out=sizes_out)

    def encode_ragged_flattened_packed(self, fmt, planes_per_frame, dims, flatten, sizes, orientations, yuv_mode, quant, method=4,
                                       min_quant=None, q_bias=0x78, dmax_luma=12, dmax_chroma=1, search=None,
                                       capacities=None, packed_capacity=None, out=None, metadata=None):
        """sjpeg_hip_encode_ragged_flattened_packed_src: encode_ragged_flattened into ONE packed buffer, with the
        arguments and the returns of encode_ragged_oriented_packed."""
        enc = (yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search, capacities, metadata)
        return self._encode_sized("encode_ragged_flattened_packed", "flattened", "dims, sizes and orientations", fmt, planes_per_frame, dims, enc, True,
                                  sizes=sizes, orientations=orientations, flatten=flatten, out=out, packed_capacity=packed_capacity)

    def encode_ragged_oriented_packed(self, fmt, planes_per_frame, dims, sizes, orientations, yuv_mode, quant, method=4,
                                      min_quant=None, q_bias=0x78, dmax_luma=12, dmax_chroma=1, search=None,
                                      capacities=None, packed_capacity=None, out=None, metadata=None):
        """sjpeg_hip_encode_ragged_oriented_packed_src: encode_ragged_oriented into ONE packed buffer, with the
        arguments and the layout of encode_ragged_full_packed.  Returns (out, sizes, offsets, modes, q, value)."""
        enc = (yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search, capacities, metadata)
        return self._encode_sized("encode_ragged_oriented_packed", "oriented", "dims, sizes and orientations", fmt, planes_per_frame, dims, enc, True,
                                  sizes=sizes, orientations=orientations, out=out, packed_capacity=packed_capacity)

    def resize_ragged_yuv(self, fmt, planes_per_frame, dims, sizes, orientations=None, out=None):
        """sjpeg_hip_resize_ragged_yuv_src: decoded video frames (fmt SRC_NV12, SRC_NV21, SRC_YUV420 or SRC_YUV444;
        planes_per_frame[k] = [y, uv] or [y, u, v], dims[k] = (w, h) as encode_ragged) resized to sizes[k] = (w, h) (None:
        their own; the STORED orientation) and turned upright by orientations[k] (EXIF 1..8; None: all 1), every plane
        as a picture of its own, in one launch.  Returns (out_fmt, pictures, buf): SRC_YUV420 or SRC_YUV444 -- always
        planar --, picture k a tuple (y, u, v) of uint8 views into buf ([h, w] each; rows padded to a multiple of 4
        bytes, planes at multiples of 16), which any ragged entry takes as its planes.  out as resize_ragged."""
        return self._orient_ragged("resize_ragged_yuv", fmt, planes_per_frame, dims, {}, sizes, orientations, out, "resize_ragged_yuv")

    def encode_ragged_yuv_resized(self, fmt, planes_per_frame, dims, sizes, orientations, yuv_mode, quant, method=4,
                                  min_quant=None, q_bias=0x78, dmax_luma=12, dmax_chroma=1, search=None, capacities=None,
                                  out=None, offsets=None, sizes_out=None, metadata=None):
        """sjpeg_hip_encode_ragged_yuv_resized_src: encode_ragged_full of decoded video frames (the four formats of
        resize_ragged_yuv) resized and turned upright inside the call, with the arguments and the returns of
        encode_ragged_oriented.  Frame k's bytes are those encode_ragged_full makes of the three planes
        Engine.resize_ragged_yuv returns, handed over in its out_fmt; yuv_mode is the format's own (YUV_420, or YUV_444
        for SRC_YUV444).  sizes None or the frames' own and orientations None or all 1: exactly encode_ragged_full on
        the caller's frames."""
        enc = (yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search, capacities, metadata)
        return self._encode_sized("encode_ragged_yuv_resized", "yuv_resized", "dims, sizes and orientations", fmt, planes_per_frame, dims, enc, False,
                                  sizes=sizes, orientations=orientations, out=out, offsets=offsets, sizes_out=sizes_out)

    def encode_ragged_yuv_resized_packed(self, fmt, planes_per_frame, dims, sizes, orientations, yuv_mode, quant, method=4,
                                         min_quant=None, q_bias=0x78, dmax_luma=12, dmax_chroma=1, search=None,
                                         capacities=None, packed_capacity=None, out=None, metadata=None):
        """sjpeg_hip_encode_ragged_yuv_resized_packed_src: encode_ragged_yuv_resized into ONE packed buffer, with the
        arguments and the returns of encode_ragged_oriented_packed."""
        enc = (yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search, capacities, metadata)
        return self._encode_sized("encode_ragged_yuv_resized_packed", "yuv_resized", "dims, sizes and orientations", fmt, planes_per_frame, dims, enc, True,
                                  sizes=sizes, orientations=orientations, out=out, packed_capacity=packed_capacity)

    def sheet_ragged(self, fmt, planes_per_frame, dims, sheet, sizes=None, orientations=None, out=None, flatten=None):
        """sjpeg_hip_sheet_ragged_src: the pictures of a ragged batch (any format the resize entries take, the YUV-plane
        ones included) resized to sizes[k] (None: fitted into their cells), turned upright by orientations[k] and stored
        into their cells of contact sheets of the Sheet `sheet`: a background fill and one launch of the resize kernel.
        Returns (out_fmt, sheets, buf): sheet s a uint8 view into buf -- [SH, SW, 3] (SRC_RGB), [SH, SW] (SRC_GRAY) or a
        tuple (y, u, v) of planes (SRC_YUV420 / SRC_YUV444) --, rows padded to a multiple of 4 bytes.  out: a contiguous
        uint8 CUDA tensor of at least sjpeg_hip_sheet_ragged_bytes bytes at a multiple of 16 (None: made here).
        flatten (a Flatten; None: today's call): sjpeg_hip_sheet_ragged_flat_src -- pictures of an alpha format laid over
        the flatten's background, which is a field of its own beside the sheet's."""
        who, keep = "sheet_ragged", []
        n = len(dims)
        if sizes is not None and len(sizes) != n:
            raise SjpegError(f"{who}: one size per frame")
        frames, _, _, _ = _ragged_frames(planes_per_frame, dims, None, None, None, None)
        shape, nsheets, skeep = _sheet_shape(who, n, sheet, sizes, orientations)
        return self._make_pictures(who, "sheet_ragged" if flatten is None else "sheet_ragged_flat", "sheet_ragged", fmt, planes_per_frame, frames,
                                   shape, lambda: {} if flatten is None else _flatten_segment(who, flatten, keep), out, nsheets)

    def _sheet_call(self, who, fmt, planes_per_frame, dims, sheet, sizes, orientations, yuv_mode, quant, method, min_quant,
                    q_bias, dmax_luma, dmax_chroma, search, metadata):
        """what the sheet encodes share: the sheets' number and bound, the call (params and metadata count SHEETS), and
        the segments every one of them has: the struct sjpeg_hip_sheet, the sizes and the orientations"""
        n = len(dims)
        if n == 0 or len(planes_per_frame) != n or (sizes is not None and len(sizes) != n):
            raise SjpegError(f"{who}: one entry of planes_per_frame, dims and sizes per frame, at least one frame")
        st = _sheet_struct(who, sheet)
        sw, sh = sheet_size(sheet, fmt)
        ns = (n + sheet.cols * sheet.rows - 1) // (sheet.cols * sheet.rows)
        call = self._full_call(who, ns, [(sw, sh)] * ns, yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search,
                               lambda msizes: [frame_bound(sw, sh, _bound_mode(yuv_mode), 2048 + max(msizes))] * ns, metadata)
        arr, oarr = _shape_arrays(who, n, sizes, orientations)
        call.keep += (st, arr, oarr)
        return ns, call, {"sheet": C.addressof(st), "sizes": _address(arr), "orientations": _address(oarr)}

    def _encode_sheet(self, who, packed, fmt, planes_per_frame, dims, sheet, sizes, orientations, enc, flatten, **outs):
        """encode_ragged_sheet and its packed form; with a Flatten, the _sheet_flat entries and its struct behind the sheet's"""
        ns, call, segments = self._sheet_call(who, fmt, planes_per_frame, dims, sheet, sizes, orientations, *enc)
        keep = []
        return self._encode_sheets_shaped(
            who, "sheet" if flatten is None else "sheet_flat", fmt, planes_per_frame, dims, ns, call,
            lambda: segments if flatten is None else dict(segments, **_flatten_segment(who, flatten, keep)), packed, **outs)

    def encode_ragged_sheet(self, fmt, planes_per_frame, dims, sheet, sizes, orientations, yuv_mode, quant, method=4,
                            min_quant=None, q_bias=0x78, dmax_luma=12, dmax_chroma=1, search=None, out_stride=None, out=None,
                            metadata=None, flatten=None):
        """sjpeg_hip_encode_ragged_sheet_src: the JPEGs of the contact sheets Engine.sheet_ragged makes of the same
        arguments, each byte for byte what encode_ragged_full makes of that sheet.  quant, search and metadata are one
        for all or one per SHEET; yuv_mode any SjpegYUVMode for RGB-like pictures (YUV_AUTO decides on the sheet), YUV_400
        for gray ones, the format's own for YUV frames.  Sheet s is written at out[s * out_stride:] (default: the bound
        of a sheet).  Returns (out, sizes, offsets, modes, q, value) as encode_ragged_full, one entry per sheet.
        flatten (a Flatten; None: today's call): sjpeg_hip_encode_ragged_sheet_flat_src, as sheet_ragged."""
        enc = (yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search, metadata)
        return self._encode_sheet("encode_ragged_sheet", False, fmt, planes_per_frame, dims, sheet, sizes, orientations, enc, flatten,
                                  out_stride=out_stride, out=out)

    def encode_ragged_sheet_packed(self, fmt, planes_per_frame, dims, sheet, sizes, orientations, yuv_mode, quant, method=4,
                                   min_quant=None, q_bias=0x78, dmax_luma=12, dmax_chroma=1, search=None,
                                   packed_capacity=None, out=None, metadata=None, flatten=None):
        """sjpeg_hip_encode_ragged_sheet_packed_src: encode_ragged_sheet into ONE packed buffer, the sheets back to back,
        with the layout of encode_ragged_full_packed over the sheets.  Returns (out, sizes, offsets, modes, q, value):
        sizes [nsheets] and offsets [nsheets + 1] device tensors.  flatten: as encode_ragged_sheet."""
        enc = (yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search, metadata)
        return self._encode_sheet("encode_ragged_sheet_packed", True, fmt, planes_per_frame, dims, sheet, sizes, orientations, enc, flatten,
                                  packed_capacity=packed_capacity, out=out)

    def search_stats(self):
        """sjpeg_hip_engine_search_stats: six host counters of the engine's most recent encode_ragged_full /
        _full_packed call -- [most passes any frame ran, measurement launches, host waits, frames whose stream replays
        the blocks their own last search pass kept, frames quantized once more after the search, trellis statistics
        launches].  No synchronisation."""
        arr = (C.c_uint64 * 6)()
        self._chk(lib().sjpeg_hip_engine_search_stats(self._h, arr), "sjpeg_hip_engine_search_stats")
        return [int(x) for x in arr]


TARGET_SIZE, TARGET_PSNR = 1, 2      # sjpeg_hip_search.target_mode (EncoderParam::TargetMode)


class _FullCall:
    """what Engine._full_call built: params (a reference to sjpeg_hip_ragged_params), the addresses of the factors, sizes
    and orientations (None: not given), meta = (the metadata array or None, whether there is one per frame), the
    capacities, results = (modes, q, value) for the library to fill, and keep: everything those point into"""

    def __init__(self, params, factors, sizes, orientations, meta, capacities, results, keep):
        self.params, self.factors, self.sizes, self.orientations = params, factors, sizes, orientations
        self.meta, self.capacities, self.results, self.keep = meta, capacities, results, keep

    def answers(self):
        """(modes, q, value) as lists, once the library has filled them"""
        return tuple(list(r) for r in self.results)


def _bound_mode(yuv_mode):
    """the sampling a frame's bound is taken at: the largest, YUV_444, where the encoder chooses (YUV_AUTO, YUV_SHARP)"""
    return YUV_444 if int(yuv_mode) in (YUV_AUTO, YUV_SHARP) else int(yuv_mode)


def _address(arr):
    return None if arr is None else arr.ctypes.data


def _shape_arrays(who, n, sizes, orientations):
    """(sizes, orientations) as the C entries take them, None for None"""
    return (None if sizes is None else _sizes_array(who, sizes),
            None if orientations is None else _orientations_array(who, n, orientations))


def _sheet_shape(who, n, sheet, sizes, orientations):
    """What the contact-sheet makers share: (the segments their _bytes entry takes -- the struct sjpeg_hip_sheet, the
    sizes and the orientations --, the most sheets n frames make, what the segments point into)"""
    st = _sheet_struct(who, sheet)
    arr, oarr = _shape_arrays(who, n, sizes, orientations)
    per = max(int(sheet.cols) * int(sheet.rows), 1)
    return {"sheet": C.addressof(st), "sizes": _address(arr), "orientations": _address(oarr)}, max((n + per - 1) // per, 1), (st, arr, oarr)


def _packed_out(who, n, planes_per_frame, capacities, packed_capacity, out):
    """The output of a packed call: (out, packed_capacity, the int64 tensor [2 n + 1] of sizes and offsets).
    packed_capacity defaults to len(out), or to the capacities' sum, each rounded up to 16, which always fits."""
    import torch
    dev = _ragged_device(planes_per_frame)
    if packed_capacity is None:
        packed_capacity = int(out.numel()) if out is not None else sum((int(c) + 15) & ~15 for c in capacities)
    packed_capacity = int(packed_capacity)
    if out is None:
        out = torch.empty(max(packed_capacity, 16), dtype=torch.uint8, device=dev)
    if out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.numel() < packed_capacity:
        raise SjpegError(f"{who}: out must be a contiguous uint8 CUDA tensor of packed_capacity bytes")
    return out, packed_capacity, torch.zeros(2 * n + 1, dtype=torch.int64, device=dev)


def _made_out(who, planes_per_frame, need, out):
    """the buffer a picture-making call writes: the caller's, or one of `need` bytes on the pictures' device"""
    import torch
    dev = _ragged_device(planes_per_frame)
    if out is None:
        out = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    if out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous():
        raise SjpegError(f"{who}: out must be a contiguous uint8 CUDA tensor")
    return out


def _frame_views(out, made, fmt):
    """The pictures a picture-making call made, as views of `out`: [h, w, 3] (SRC_RGB), a tuple (y, u, v) of planes
    (SRC_YUV420 / SRC_YUV444) or [h, w] (gray)."""
    base = out.storage_offset() - out.data_ptr()     # (as_strided counts from the start of the storage: `out` may be a slice)
    if fmt == SRC_RGB:
        return [out.as_strided((r.height, r.width, 3), (int(r.row_stride[0]), 3, 1), base + int(r.plane[0])) for r in made]
    if fmt in (SRC_YUV420, SRC_YUV444):
        return [tuple(out.as_strided(yuv_plane_size(fmt, r.width, r.height, c)[::-1], (int(r.row_stride[c]), 1),
                                     base + int(r.plane[c])) for c in range(3)) for r in made]
    return [out.as_strided((r.height, r.width), (int(r.row_stride[0]), 1), base + int(r.plane[0])) for r in made]


def _ragged_args(who, n, quant, min_quant, search, yuv_mode, capacities, dims):
    """What the ragged batch calls hand to the library: the starting matrices ([1][2][64], or with a list [n][2][64])
    and whether there is one per frame; min_quant [2][64] or None; the SearchParams array (None without a search) and
    whether there is one per frame; the capacities (default: frame_bound(w, h, yuv_mode, 2048)).  who: the caller, for
    its error texts."""
    per_frame = isinstance(quant, (list, tuple))
    if per_frame and len(quant) != n:
        raise SjpegError(f"{who}: one starting matrix per frame")
    q = np.ascontiguousarray(np.stack([np.asarray(m, np.uint8).reshape(2, 64) for m in quant]) if per_frame
                             else np.asarray(quant, np.uint8).reshape(1, 2, 64))
    mq = None if min_quant is None else np.ascontiguousarray(min_quant, np.uint8).reshape(2, 64)
    sarr, search_per_frame = None, False
    if search is not None:
        search_per_frame = isinstance(search, (list, tuple))
        if search_per_frame and len(search) != n:
            raise SjpegError(f"{who}: one search per frame")
        sp = [_search_params(x) for x in (search if search_per_frame else [search])]
        sarr = (SearchParams * len(sp))(*sp)
    if capacities is None:
        capacities = [frame_bound(w, h, yuv_mode, 2048) for (w, h) in dims]
    return q, per_frame, mq, sarr, search_per_frame, capacities


def _search_params(x):
    """A SearchParams of a SearchParams or a dict of its fields (defaults: passes 10, tolerance 1, qmin 0, qmax 100)."""
    if isinstance(x, SearchParams):
        return x
    d = dict(x)
    return SearchParams(int(d["target_mode"]), float(d["target_value"]), int(d.get("passes", 10)),
                        float(d.get("tolerance", 1.0)), float(d.get("qmin", 0.0)), float(d.get("qmax", 100.0)))


def riskiness_verdict(sums, w, h):
    """sjpeg_hip_riskiness_verdict: (SjpegYUVMode, risk) of one frame's three riskiness sums (SjpegRiskiness'
    arithmetic, host only)."""
    arr = (C.c_uint64 * 3)(*[int(x) for x in sums])
    risk = C.c_float(0)
    mode = lib().sjpeg_hip_riskiness_verdict(arr, int(w), int(h), C.byref(risk))
    return int(mode), float(risk.value)


def _ragged_device(planes_per_frame):
    import torch
    return next((p.device for fr in planes_per_frame for p in fr if not isinstance(p, tuple)),
                torch.device("cuda", torch.cuda.current_device()))


def _ragged_frames(planes_per_frame, dims, capacities, out, offsets, sizes):
    """The sjpeg_hip_ragged_frame array of a ragged call (planes_per_frame, dims as Engine.encode_ragged) and, where
    capacities are given, its output: offsets (default: the capacities back to back, 16-byte aligned), out and sizes
    (made on the pictures' device where None).  Returns (frames, out, sizes, offsets)."""
    import torch
    n = len(dims)
    if n == 0 or len(planes_per_frame) != n:
        raise SjpegError("ragged call: one entry of planes_per_frame and dims per frame, at least one frame")
    frames = (RaggedFrame * n)()
    if capacities is not None:
        if offsets is None:
            offsets, at = [], 0
            for c in capacities:
                offsets.append(at)
                at += (int(c) + 15) & ~15
            total = at
        else:
            total = max(int(o) + int(c) for o, c in zip(offsets, capacities))
        dev = _ragged_device(planes_per_frame)
        if out is None:
            out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        if sizes is None:
            sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    for k in range(n):
        fr = frames[k]
        for i, p in enumerate(planes_per_frame[k]):
            if isinstance(p, tuple):                 # (device address of row 0, row stride): bottom-up rows too
                fr.plane[i], fr.row_stride[i] = int(p[0]), int(p[1])
            else:
                fr.plane[i] = p.data_ptr()
                fr.row_stride[i] = p.stride(0) * p.element_size()
        fr.width, fr.height = int(dims[k][0]), int(dims[k][1])
        if capacities is not None:
            fr.out_offset, fr.out_capacity = int(offsets[k]), int(capacities[k])
    return frames, out, sizes, offsets


def _check_layout(who, layout):
    if layout not in ("hwc", "chw"):
        raise SjpegError(f"{who}: layout {layout!r} is not 'hwc' ([H, W, 3]) or 'chw' ([3, H, W])")
    return layout == "chw"


def _chw_kinds(im, floats):
    """How a layout="chw" picture may be read: a subset of "planar", "rgb" / "rgba" (interleaved, 3 / 4 elements a
    pixel) and "gray" (float pictures only), empty when it is none of them.  A dimension of size 1 is never stepped
    over, so whatever stride torch reports for it is not looked at: a one-pixel-wide picture is planar with any
    stride(2), and interleaved as well when its channels lie next to each other."""
    st, sh = im.stride(), im.shape
    if im.dim() == 3 and sh[0] == 3 and sh[1] >= 1 and sh[2] >= 1:
        kinds = []
        if st[2] == 1 or sh[2] == 1:
            kinds.append("planar")
        if st[0] == 1 and (st[2] == 3 or sh[2] == 1):
            kinds.append("rgb")
        if st[0] == 1 and (st[2] == 4 or sh[2] == 1):
            kinds.append("rgba")
        return kinds
    if floats and im.dim() in (2, 3) and (im.dim() == 2 or sh[0] == 1) and sh[-2] >= 1 and sh[-1] >= 1 and \
            (st[-1] == 1 or sh[-1] == 1):
        return ["gray"]
    return []


def _chw_planes(who, images, fp=None):
    """The planes, dims, device and format of a layout="chw" call: every image a CUDA uint8 tensor [3, H, W] with stride
    1 over x (any row stride: crops of a larger tensor work) -- SRC_RGB_PLANAR, its R, G and B planes im[0], im[1],
    im[2] -- or with stride 1 over the channels and 3 or 4 over x (a slice of a channels_last batch, a permuted
    [H, W, 3] or [H, W, 4] array) -- SRC_RGB / SRC_RGBA, one plane.  fp (the call's FloatPixels): float tensors of one
    dtype instead, SRC_RGB_PLANAR_F* / SRC_RGB_F* / SRC_RGBA_F*, or gray pictures [1, H, W] / [H, W], SRC_GRAY_F*.  A call
    has one format: every image lies as image 0 does."""
    import torch
    dev = None
    esz, kind0, dt = 1, None, None                   # (dt: the float dtype by name; None: bytes)
    for k, im in enumerate(images):
        if not isinstance(im, torch.Tensor) or not im.is_cuda:
            raise SjpegError(f"{who}: image {k} is not a CUDA tensor")
        if fp is None:
            if im.dtype != torch.uint8:
                raise SjpegError(f"{who}: image {k} is {im.dtype}, not torch.uint8")
        else:
            by_dtype = {getattr(torch, name): name for name in _DTYPE_BYTES}
            if im.dtype not in by_dtype:
                raise SjpegError(f"{who}: image {k} is {im.dtype}: FloatPixels take torch.float32, torch.float16 or "
                                 f"torch.bfloat16")
            if k > 0 and im.dtype != images[0].dtype:
                raise SjpegError(f"{who}: image {k} is {im.dtype}, image 0 {images[0].dtype}: one dtype per call")
            dt, esz = by_dtype[im.dtype], im.element_size()
        kinds = _chw_kinds(im, fp is not None)
        if not kinds:
            raise SjpegError(f"{who}: image {k} must be [3, H, W] planar RGB with layout='chw' (stride 1 over x; its "
                             f"shape is {tuple(im.shape)}, its strides {tuple(im.stride())})" +
                             ("" if fp is None else "; or [3, H, W] with stride 1 over the channels and 3 or 4 over x; "
                                                    "or gray [1, H, W] / [H, W]"))
        both = kinds if kind0 is None else [x for x in kind0 if x in kinds]
        if not both:
            raise SjpegError(f"{who}: image {k} lies in memory as {kinds[0]!r} (shape {tuple(im.shape)}, strides "
                             f"{tuple(im.stride())}), the images before it as {kind0[0]!r}: one format per call")
        kind0 = both
        if dev is None:
            dev = im.device
        elif im.device != dev:
            raise SjpegError(f"{who}: image {k} is on {im.device}, image 0 on {dev}")
    # ((address, row stride) pairs; torch reports any stride for a dimension of size 1, so a one-pixel-wide picture
    # passes with any stride(2), and a one-row picture is handed over with its width as the row stride)
    # (strides in bytes: esz is the element size, 1 for uint8)
    kind0 = kind0[0] if kind0 else "planar"          # (planar before interleaved where a call could be read as both)
    fmt = _CHW_FORMAT[(kind0, dt)]
    if kind0 == "planar":
        planes = [[(im.data_ptr() + c * im.stride(0) * esz, (im.stride(1) if im.shape[1] > 1 else im.shape[2]) * esz)
                   for c in range(3)] for im in images]
    elif kind0 == "gray":
        planes = [[(im.data_ptr(), (im.stride(-2) if im.shape[-2] > 1 else im.shape[-1]) * esz)] for im in images]
    else:
        step = _FORMATS[fmt][1]
        planes = [[(im.data_ptr(), (im.stride(1) if im.shape[1] > 1 else im.shape[2] * step) * esz)] for im in images]
    dims = [(int(im.shape[-1]), int(im.shape[-2])) for im in images]
    return planes, dims, dev, fmt


def _pictures(who, images, chw, fp=None, alpha=False, fine=False):
    """The one reader of a call's pictures: (planes, dims, device, format).  layout="hwc": CUDA uint8 tensors [H, W, 3] of
    packed RGB on one device, each handed over as one plane of rows -- SRC_RGB; refused in the three sentences of
    encode_images and encode_images_full (fine) or in the one of the other calls.  chw: what _chw_planes reads, with fp
    the call's FloatPixels.  alpha: what _alpha_pictures reads."""
    import torch
    images = list(images)
    if not images:
        raise SjpegError(f"{who}: no images")
    if alpha:
        return _alpha_pictures(who, images, fp)
    if chw:
        return _chw_planes(who, images, fp)
    dev = None
    for k, im in enumerate(images):
        if not (isinstance(im, torch.Tensor) and im.is_cuda and im.dtype == torch.uint8 and im.dim() == 3 and
                im.shape[2] == 3 and im.stride(2) == 1 and im.stride(1) == 3):
            if not fine:
                raise SjpegError(f"{who}: image {k} must be a CUDA uint8 tensor [H, W, 3] of packed RGB")
            if not isinstance(im, torch.Tensor) or not im.is_cuda:
                raise SjpegError(f"{who}: image {k} is not a CUDA tensor")
            if im.dtype != torch.uint8:
                raise SjpegError(f"{who}: image {k} is {im.dtype}, not torch.uint8")
            raise SjpegError(f"{who}: image {k} must be [H, W, 3] packed RGB (stride 1 over the channels, "
                             f"3 over x)")
        if dev is None:
            dev = im.device
        elif im.device != dev:
            raise SjpegError(f"{who}: image {k} is on {im.device}, image 0 on {dev}")
    planes = [[im.as_strided((im.shape[0], im.shape[1] * 3), (im.stride(0), 1))] for im in images]
    dims = [(int(im.shape[1]), int(im.shape[0])) for im in images]
    return planes, dims, dev, SRC_RGB


class _Shaping:
    """What a call's wrappers ask for before the pictures are coded: flat (the Flattened), orients, factors, sizes (None:
    nothing to do), fp (the FloatPixels whose transform the engine takes); every: launch the resize even where the
    sizes are the pictures' own (the calls that return the pictures do)."""

    def __init__(self, flat, orients, factors, sizes, fp):
        self.flat, self.orients, self.factors, self.sizes, self.fp, self.every = flat, orients, factors, sizes, fp, False


def _unwrap(who, images, chw):
    """(the bare images of a call, the _Shaping its wrappers ask for): the one place where Flattened, Oriented, Reduced,
    Resized and FloatPixels come off, in this order.  A new wrapper comes off here."""
    images, flat = _flattened(who, images, chw)
    images, orients = _oriented(images)
    images, factors = _reduced(images)
    images, sizes = _resized(images)
    images, fp = _float_pixels(who, images, chw)
    return images, _Shaping(flat, orients, factors, sizes, fp if flat is None else flat.fp)


def _engine_for(engine, dev, fp=None):
    """the caller's engine, or one made for the pictures' device; the transform of a FloatPixels is set on it"""
    eng = engine or Engine(dev.index or 0)
    if fp is not None:
        eng.set_pixel_transform(fp.scale, fp.bias)
    return eng


def _shape(eng, dev, fmt, planes, dims, todo):
    """Runs the one launch a _Shaping asks for -- flatten_ragged, reduce_ragged, orient_ragged or resize_ragged -- and
    returns (fmt, planes, dims) of the uint8 pictures it made, for the rest of the call to code; they live until it
    returns.  Nothing to do: the arguments as they came."""
    import torch
    with torch.cuda.device(dev):
        if todo.flat is not None:
            # (Flattened: laid over the background, resized and turned upright by the one launch)
            fmt, made, _ = eng.flatten_ragged(fmt, planes, dims, todo.flat.flatten, todo.flat.sizes, todo.flat.orientations)
        elif todo.factors is not None:
            fmt, made, _ = eng.reduce_ragged(fmt, planes, dims, todo.factors)
        elif todo.orients is not None:
            # (Oriented: resized and turned upright by the one launch)
            fmt, made, _ = eng.orient_ragged(fmt, planes, dims, todo.sizes, todo.orients)
        elif todo.sizes is not None and (todo.every or todo.sizes != dims):
            fmt, made, _ = eng.resize_ragged(fmt, planes, dims, todo.sizes)
        else:
            return fmt, planes, dims
    return fmt, [[p] for p in made], [(int(p.shape[1]), int(p.shape[0])) for p in made]


def _one_target(who, target_size, target_psnr):
    """the target of a call -- its target_size or its target_psnr --, or None"""
    if target_size is not None and target_psnr is not None:
        raise SjpegError(f"{who}: give target_size or target_psnr, not both")
    return target_size if target_size is not None else target_psnr


def _target_search(who, what, n, target_size, target_psnr, passes=10, tolerance=1.0, qmin=0.0, qmax=100.0):
    """The SearchParams of a call's target, one value or one per `what` (image, frame, sheet): a list of n, or None
    without a target."""
    target = target_size if target_size is not None else target_psnr
    if target is None:
        return None
    ts = _per_picture(target, n)
    if len(ts) != n:
        raise SjpegError(f"{who}: one target per {what}")
    mode = TARGET_SIZE if target_size is not None else TARGET_PSNR
    return [SearchParams(mode, float(t), int(passes), float(tolerance), float(qmin), float(qmax)) for t in ts]


def _gray_mode(who, fmt, yuv_mode):
    """gray float pictures are coded in YUV_400 and nothing else"""
    if fmt in _GRAY_FLOAT and int(yuv_mode) != YUV_400:
        raise SjpegError(f"{who}: gray FloatPixels ([1, H, W] or [H, W]) are coded with yuv_mode=YUV_400 only, not "
                         f"{int(yuv_mode)} (YUV_AUTO and YUV_SHARP take RGB pictures)")


def encode_images(images, quality=75.0, yuv_mode=YUV_420, engine=None, method=0, min_quant=None, q_bias=0x78,
                  dmax_luma=12, dmax_chroma=1, target_size=None, target_psnr=None, passes=10, tolerance=1.0, qmin=0.0,
                  qmax=100.0, use_trellis=False, packed=False, metadata=None, layout="hwc"):
    """JPEGs (list of bytes) of device-resident pictures of any sizes in ONE ragged call: images is a sequence of CUDA
    uint8 tensors [H_k, W_k, 3] on one device (packed RGB: stride 1 over the channels, 3 over x; any row stride);
    quality is one float or one per image.  method 0 (the default): frame k's bytes are what encode_device makes of it
    alone.  Methods 1..6 (4: the reference's defaults) with min_quant, q_bias and the qdelta limits: what
    encode_device_method makes of it alone.

    target_size (bytes) or target_psnr (dB), one value or one per image, at most one of the two: the reference's
    multi-pass search (sjpeg::Encode with EncoderParam.target_mode / target_value / passes / tolerance / qmin / qmax)
    per picture, the quality its starting point -- Engine.encode_ragged_search.  passes defaults to 10, as the
    reference's command-line tool uses when a target is given; EncoderParam's own default of 1 means no search.  Not
    with YUV_AUTO / YUV_SHARP or the trellis methods 7 and 8.  With neither target, nothing changes.

    use_trellis=True: EncoderParam::use_trellis as the reference maps it (src/api.cc:155-157) -- method 4 becomes 7,
    method 6 becomes 8, and the pictures go through Engine.encode_ragged_trellis: frame k's bytes are what
    SjpegEncode(picture, quality, 7 or 8, yuv_mode) makes of it alone.  With any other method the reference ignores
    the flag, and so does this call.  Not together with a target.  (method=7 / 8 without the keyword is refused as
    before; with it they are taken as they are.)

    packed=True: the same list of bytes through Engine.encode_ragged_packed -- the JPEGs back to back in one pool and
    ONE device-to-host copy of it instead of one per picture.  The first pool is small (per picture 2048 bytes of
    header allowance plus half a byte per sample, at least 64 KiB for the call); the pictures a full pool dropped are
    coded again in a second packed call whose pool always fits (packed_stats() counts those).  The default keeps the
    unpacked path.

    layout="chw": every image is a CUDA uint8 tensor [3, H_k, W_k] instead -- channel-first, as torch stores pictures --
    with stride 1 over x and any row stride (a crop of a larger tensor works); the pictures go in as SRC_RGB_PLANAR,
    without a repack, and the bytes are those of the same pixels handed over as [H, W, 3].  A call has one layout; the
    keyword is explicit because [3, W, 3] is both.  A [3, H_k, W_k] picture that lies channels-last in memory -- stride
    1 over the channels, 3 or 4 over x: x[k] of a torch.channels_last batch, hwc.permute(2, 0, 1) -- goes in as SRC_RGB /
    SRC_RGBA, again without a copy.  With layout="chw", images may be a FloatPixels: float32, float16 or bfloat16
    pictures, planar, channels-last or gray, converted to bytes inside the encoder (see FloatPixels).

    metadata: None, one PictureMetadata for every picture or a sequence of one per picture (None entries: none): each
    JPEG carries its EXIF, ICC profile, XMP and APP markers as the reference writes them (EncoderParam's fields), a
    target_size counts them, and the output buffers make room for them.  (It stands in front of layout, which stays
    the last parameter: pass layout by keyword.)"""
    import torch
    who = "encode_images"
    chw = _check_layout(who, layout)
    images, todo = _unwrap(who, images, chw)
    target = _one_target(who, target_size, target_psnr)
    if use_trellis and target is not None:
        raise SjpegError("encode_images: a target size or PSNR is not searched with the trellis (use_trellis): that "
                         "search prices every pass with the pass's own codes")
    if target is not None:
        if int(method) in (7, 8):
            raise SjpegError("encode_images: a target size or PSNR is searched with methods 0..6, not the trellis "
                             "methods 7 and 8")
        if int(yuv_mode) in (YUV_AUTO, YUV_SHARP):
            raise SjpegError("encode_images: a target size or PSNR takes YUV_420, YUV_444 or YUV_400, not YUV_AUTO "
                             "or YUV_SHARP")
    method = int(method)
    if method in (7, 8) and not use_trellis:
        raise SjpegError("encode_images: trellis methods 7 and 8 go through the host API (SjpegEncode / sjpeg::Encode)")
    if method < 0 or method > 8:
        raise SjpegError(f"encode_images: method {method} is not one of 0..6")
    if use_trellis:
        method = {4: 7, 6: 8}.get(method, method)
    yuv_mode = int(yuv_mode)
    if yuv_mode < 0 or yuv_mode > 4:
        raise SjpegError(f"encode_images: yuv_mode {yuv_mode} is not one of 0..4 (SjpegYUVMode)")
    images = list(images)
    if not images:
        raise SjpegError("encode_images: no images")
    if yuv_mode in (YUV_AUTO, YUV_SHARP) and not chw and todo.flat is None:
        for k, im in enumerate(images):
            if len(getattr(im, "shape", ())) != 3 or im.shape[2] != 3:
                raise SjpegError(f"encode_images: image {k}: YUV_AUTO and YUV_SHARP take RGB pictures [H, W, 3]")
    n = len(images)
    qs = _per_picture(quality, n)
    if len(qs) != n:
        raise SjpegError("encode_images: one quality per image")
    planes, dims, dev, fmt = _pictures(who, images, chw, todo.fp, alpha=todo.flat is not None, fine=True)
    _gray_mode(who, fmt, yuv_mode)
    eng = _engine_for(engine, dev, todo.fp)
    fmt, planes, dims = _shape(eng, dev, fmt, planes, dims, todo)
    search = _target_search(who, "image", n, target_size, target_psnr, passes, tolerance, qmin, qmax)
    _, _, _, metas = _metadata_args("encode_images", n, metadata)
    if metadata is not None and not packed and not (method == 0 and target is None and yuv_mode not in (YUV_AUTO, YUV_SHARP)):
        # (every flow below but the method 0 call with ready headers: the one call that takes them all, with metadata)
        with torch.cuda.device(dev):
            out, sizes, offs, _, _, _ = eng.encode_ragged_full(fmt, planes, dims, yuv_mode, _quality_quant(qs), method,
                                                               min_quant, q_bias, dmax_luma, dmax_chroma, search,
                                                               metadata=metadata)
            eng.wait()                           # (pipelined mode: the output is complete after this)
            return _fetch_ragged(out, sizes, offs)
    if packed:
        # (the unpacked method 0 path with a fixed sampling and no target codes with the tables of the quality alone --
        # make_tables: no min_quant, the default bias --, so the packed one does too)
        plain0 = method == 0 and search is None and yuv_mode not in (YUV_AUTO, YUV_SHARP)
        with torch.cuda.device(dev):
            return _encode_images_packed(eng, planes, dims, yuv_mode, _quality_quant(qs), method,
                                         None if plain0 else min_quant, 0x78 if plain0 else q_bias,
                                         dmax_luma, dmax_chroma, search, fmt=fmt, metadata=metadata)
    if target is not None:
        with torch.cuda.device(dev):
            out, sizes, offs, _, _ = eng.encode_ragged_search(fmt, planes, dims, yuv_mode, _quality_quant(qs),
                                                              search, method, min_quant, q_bias, dmax_luma,
                                                              dmax_chroma)
            eng.wait()                           # (pipelined mode: the output is complete after this)
            return _fetch_ragged(out, sizes, offs)
    if method >= 7:
        with torch.cuda.device(dev):
            out, sizes, offs, _ = eng.encode_ragged_trellis(fmt, planes, dims, yuv_mode, _quality_quant(qs), method,
                                                            min_quant, q_bias, dmax_luma, dmax_chroma)
            eng.wait()                           # (pipelined mode: the output is complete after this)
            return _fetch_ragged(out, sizes, offs)
    if yuv_mode in (YUV_AUTO, YUV_SHARP):
        with torch.cuda.device(dev):
            out, sizes, offs, _ = eng.encode_ragged_auto(fmt, planes, dims, yuv_mode, _quality_quant(qs), method,
                                                         min_quant, q_bias, dmax_luma, dmax_chroma)
            eng.wait()                           # (pipelined mode: the output is complete after this)
            return _fetch_ragged(out, sizes, offs)
    if method != 0:
        with torch.cuda.device(dev):
            out, sizes, offs = eng.encode_ragged_batch(fmt, planes, dims, yuv_mode, _quality_quant(qs), method,
                                                       min_quant, q_bias, dmax_luma, dmax_chroma)
            eng.wait()                           # (pipelined mode: the output is complete after this)
            return _fetch_ragged(out, sizes, offs)
    made = {}
    tables, headers = [], []
    for k, im in enumerate(images):
        q = float(qs[k])
        if q not in made:
            made[q] = make_tables(quality=q)
        t, qm = made[q]
        tables.append(t)
        if metas[k] is None:
            headers.append(make_header(dims[k][0], dims[k][1], yuv_mode, qm))
        else:
            m = metas[k]
            headers.append(make_header_meta(dims[k][0], dims[k][1], yuv_mode, qm, None, m.app_markers, m.exif, m.iccp, m.xmp,
                                            m.xmp_split_point))
    per_frame = len(made) > 1
    with torch.cuda.device(dev):
        out, sizes, offs = eng.encode_ragged(fmt, planes, dims, yuv_mode, tables if per_frame else tables[0],
                                             headers)
        eng.wait()                               # (pipelined mode: the output is complete after this)
        return _fetch_ragged(out, sizes, offs)


def encode_images_full(images, quality=75.0, yuv_mode=YUV_AUTO, method=4, use_trellis=False, target_size=None,
                       target_psnr=None, passes=10, tolerance=1.0, qmin=0.0, qmax=100.0, min_quant=None, q_bias=0x78,
                       dmax_luma=12, dmax_chroma=1, engine=None, packed=False):
    """JPEGs (list of bytes) of device-resident RGB pictures [H_k, W_k, 3] of any sizes, each what the reference's
    sjpeg::Encode() makes of it alone with these EncoderParam fields -- ANY combination of them, in one ragged call
    (Engine.encode_ragged_full).  The defaults are those of EncoderParam / SjpegCompress: quality 75, SJPEG_YUV_AUTO,
    method 4.  use_trellis maps method 4 to 7 and 6 to 8 (src/api.cc:155-157).  target_size (bytes) or target_psnr (dB),
    one value or one per image, at most one of the two: the multi-pass search per picture with passes / tolerance /
    qmin / qmax -- with YUV_AUTO, YUV_SHARP and the trellis too, which encode_images refuses.  packed=True: through
    Engine.encode_ragged_full_packed and the two-pool scheme of encode_images (packed_stats() counts it).
    Channel-first pictures [3, H_k, W_k]: encode_images_full_chw, the same call with layout="chw" of encode_images (this
    function's parameter list is pinned as it is)."""
    return _encode_images_full("hwc", images, quality, yuv_mode, method, use_trellis, target_size, target_psnr, passes,
                               tolerance, qmin, qmax, min_quant, q_bias, dmax_luma, dmax_chroma, engine, packed)


def encode_images_full_chw(images, quality=75.0, yuv_mode=YUV_AUTO, method=4, use_trellis=False, target_size=None,
                           target_psnr=None, passes=10, tolerance=1.0, qmin=0.0, qmax=100.0, min_quant=None, q_bias=0x78,
                           dmax_luma=12, dmax_chroma=1, engine=None, packed=False):
    """encode_images_full of channel-first pictures: every image a CUDA uint8 tensor [3, H_k, W_k] with stride 1 over x
    and any row stride, as encode_images(layout="chw") takes them -- SRC_RGB_PLANAR, no repack; the bytes are those of
    the same pixels handed to encode_images_full as [H, W, 3]."""
    return _encode_images_full("chw", images, quality, yuv_mode, method, use_trellis, target_size, target_psnr, passes,
                               tolerance, qmin, qmax, min_quant, q_bias, dmax_luma, dmax_chroma, engine, packed)


def encode_images_full_meta(images, metadata, layout="hwc", **params):
    """encode_images_full (layout="hwc") or encode_images_full_chw ("chw") with metadata: None, one PictureMetadata for
    every picture or a sequence of one per picture (None entries: none), as encode_images takes it.  params: the
    keywords of encode_images_full.  (Those two functions' parameter lists are pinned as they are; this is their
    metadata form.)"""
    import inspect
    sig = list(inspect.signature(encode_images_full).parameters.values())[1:]      # (its names and defaults, in its order)
    for k in params:
        if k not in [p.name for p in sig]:
            raise TypeError(f"encode_images_full_meta: unexpected keyword {k!r}")
    return _encode_images_full(layout, images, *[params.get(p.name, p.default) for p in sig], metadata=metadata)


def _encode_images_full(layout, images, quality, yuv_mode, method, use_trellis, target_size, target_psnr, passes,
                        tolerance, qmin, qmax, min_quant, q_bias, dmax_luma, dmax_chroma, engine, packed, metadata=None):
    import torch
    who = "encode_images_full"
    chw = _check_layout(who, layout)
    images, todo = _unwrap(who, images, chw)
    _one_target(who, target_size, target_psnr)
    method = int(method)
    if method < 0 or method > 8:
        raise SjpegError(f"encode_images_full: method {method} is not one of 0..8")
    if use_trellis:
        method = {4: 7, 6: 8}.get(method, method)
    yuv_mode = int(yuv_mode)
    if yuv_mode < 0 or yuv_mode > 4:
        raise SjpegError(f"encode_images_full: yuv_mode {yuv_mode} is not one of 0..4 (SjpegYUVMode)")
    images = list(images)
    if not images:
        raise SjpegError("encode_images_full: no images")
    n = len(images)
    qs = _per_picture(quality, n)
    if len(qs) != n:
        raise SjpegError("encode_images_full: one quality per image")
    planes, dims, dev, fmt = _pictures(who, images, chw, todo.fp, alpha=todo.flat is not None, fine=True)
    _gray_mode(who, fmt, yuv_mode)
    eng = _engine_for(engine, dev, todo.fp)
    fmt, planes, dims = _shape(eng, dev, fmt, planes, dims, todo)
    search = _target_search(who, "image", n, target_size, target_psnr, passes, tolerance, qmin, qmax)
    with torch.cuda.device(dev):
        if packed:
            return _encode_images_packed(eng, planes, dims, yuv_mode, _quality_quant(qs), method, min_quant, q_bias,
                                         dmax_luma, dmax_chroma, search, "full", fmt=fmt,
                                         metadata=metadata)
        out, sizes, offs, _, _, _ = eng.encode_ragged_full(fmt, planes, dims, yuv_mode, _quality_quant(qs), method,
                                                           min_quant, q_bias, dmax_luma, dmax_chroma, search,
                                                           metadata=metadata)
        eng.wait()                               # (pipelined mode: the output is complete after this)
        return _fetch_ragged(out, sizes, offs)


def _quality_quant(qs):
    """The starting matrices of the qualities qs: one [2][64] matrix when they are all equal, else a list."""
    made = {}
    for q in qs:
        if float(q) not in made:
            m = np.zeros((2, 64), np.uint8)
            lib().sjpeg_hip_quality_matrices(float(q), m.ctypes.data)
            made[float(q)] = m
    return [made[float(q)] for q in qs] if len(made) > 1 else made[float(qs[0])]


def compress_images(images, quality=75.0, engine=None, use_trellis=False, packed=False, metadata=None, layout="hwc"):
    """The batch SjpegCompress(): JPEGs (list of bytes) of device-resident RGB pictures [H_k, W_k, 3] of any sizes, each
    what SjpegCompress (method 4, SJPEG_YUV_AUTO) makes of it alone, in one ragged call.  use_trellis=True: with
    EncoderParam::use_trellis, i.e. what SjpegEncode(picture, quality, 7, SJPEG_YUV_AUTO) makes of it.  packed=True:
    through the packed call and one device-to-host copy, as encode_images.  layout="chw": the pictures are
    [3, H_k, W_k] instead, as encode_images takes them.  metadata: what every picture carries, as encode_images."""
    return encode_images(images, quality, YUV_AUTO, engine=engine, method=4, use_trellis=use_trellis, packed=packed,
                         metadata=metadata, layout=layout)


def riskiness_images(images, engine=None, layout="hwc"):
    """[(SjpegYUVMode, risk)] of device-resident RGB pictures [H_k, W_k, 3] of any sizes, each what SjpegRiskiness says
    of it alone, from one ragged riskiness call.  layout="chw": the pictures are [3, H_k, W_k] instead, as encode_images
    takes them."""
    import torch
    who = "riskiness_images"
    chw = _check_layout(who, layout)
    if isinstance(images, Reduced):
        raise SjpegError("riskiness_images: Reduced pictures are not taken: reduce first -- "
                         "riskiness_images(reduce_images(images, factor)) -- the verdict is that of the reduced picture")
    if isinstance(images, Resized):
        raise SjpegError("riskiness_images: Resized pictures are not taken: resize first -- "
                         "riskiness_images(resize_images(images, sizes)) -- the verdict is that of the resized picture")
    if isinstance(images, Oriented):
        raise SjpegError("riskiness_images: Oriented pictures are not taken: turn them first -- "
                         "riskiness_images(orient_images(images, orientations)) -- the verdict is that of the upright picture")
    if isinstance(images, Flattened):
        raise SjpegError("riskiness_images: Flattened pictures are not taken: flatten first -- "
                         "riskiness_images(flatten_images(images, ...)) -- the verdict is that of the flattened picture")
    images, fp = _float_pixels(who, images, chw)
    planes, dims, dev, fmt = _pictures(who, images, chw, fp)
    _gray_mode(who, fmt, YUV_AUTO)
    eng = _engine_for(engine, dev, fp)
    with torch.cuda.device(dev):
        sums = eng.riskiness_ragged(fmt, planes, dims).cpu().numpy()
    return [riskiness_verdict(sums[k], w, h) for k, (w, h) in enumerate(dims)]


def reduce_images(images, factor, engine=None, layout="hwc"):
    """The reduced uint8 pictures Reduced(images, factor) codes, as views of ONE device buffer, from one launch of the
    reduce kernel: images as encode_images takes them (layout="hwc": CUDA uint8 tensors [H_k, W_k, 3]; "chw": channel-first
    uint8 tensors or a FloatPixels), factor one int in 1..8 or one per picture.  Returns uint8 CUDA tensors
    [h'_k, w'_k, 3] (layout="chw": [3, h'_k, w'_k], channels-last in memory, which the layout="chw" calls take as they
    are; gray FloatPixels: [h'_k, w'_k]).  Rows are padded to a multiple of 4 bytes: the views are not contiguous.  The
    pixel transform of a FloatPixels is set on the engine (it stays set)."""
    chw = _check_layout("reduce_images", layout)
    red = Reduced(images, factor)
    return _made_images("reduce_images", red, engine, chw, factors=red.factors)


def resize_images(images, sizes, engine=None, layout="hwc"):
    """The resized uint8 pictures Resized(images, sizes) codes, as views of ONE device buffer, from one launch of the
    resize kernel: images as encode_images takes them (layout="hwc": CUDA uint8 tensors [H_k, W_k, 3]; "chw":
    channel-first uint8 tensors or a FloatPixels), sizes one (w, h) or one per picture.  Returns what reduce_images
    returns: uint8 CUDA tensors [h_k, w_k, 3] (layout="chw": [3, h_k, w_k], channels-last in memory; gray FloatPixels:
    [h_k, w_k]), rows padded to a multiple of 4 bytes.  The pixel transform of a FloatPixels is set on the engine (it
    stays set)."""
    chw = _check_layout("resize_images", layout)
    return _made_images("resize_images", Resized(images, sizes), engine, chw, every=True)


def orient_images(images, orientations, sizes=None, engine=None, layout="hwc"):
    """The upright uint8 pictures Oriented(images, orientations, sizes) codes, as views of ONE device buffer, from one
    launch of the resize kernel: images, sizes (None: the pictures' own), engine and layout as resize_images takes them,
    orientations one EXIF Orientation 1..8 or one per picture.  Returns what resize_images returns, picture k being
    [h_k, w_k, 3] for the orientations 1..4 and [w_k, h_k, 3] for 5..8 (layout="chw": channel-first views)."""
    chw = _check_layout("orient_images", layout)
    ori = Oriented(images, orientations, sizes)
    return _made_images("orient_images", ori, engine, chw, orients=ori.orientations)


def flatten_images(images, background=(255, 255, 255), premultiplied=False, alpha_scale=255.0, alpha_bias=0.0,
                   orientations=None, sizes=None, engine=None, layout="hwc"):
    """The flattened uint8 pictures Flattened(images, background, ...) codes, as views of ONE device buffer, from one
    launch of the resize kernel: images CUDA uint8 tensors [H_k, W_k, 4] or a FloatPixels of float tensors [H_k, W_k, 4]
    (R, G, B, alpha), the other arguments as Flattened takes them.  Returns uint8 CUDA tensors [h_k, w_k, 3] (upright:
    [w_k, h_k, 3] for the orientations 5..8), rows padded to a multiple of 4 bytes."""
    chw = _check_layout("flatten_images", layout)
    flat = images if isinstance(images, Flattened) else Flattened(images, background, premultiplied, alpha_scale, alpha_bias,
                                                                   orientations, sizes)
    return _made_images("flatten_images", flat, engine, chw)


def _made_images(who, wrapped, engine, chw, **always):
    """reduce_images, resize_images, orient_images and flatten_images: the pictures the wrapper codes, from its one launch.
    always: what the call hands to that launch even where it changes nothing (factors and orientations that are all 1,
    sizes that are the pictures' own)."""
    import torch
    images, todo = _unwrap(who, wrapped, chw)
    planes, dims, dev, fmt = _pictures(who, images, chw, todo.fp, alpha=todo.flat is not None)
    eng = _engine_for(engine, dev, todo.fp)
    vars(todo).update(always)
    fmt, planes, _ = _shape(eng, dev, fmt, planes, dims, todo)
    if engine is None:
        with torch.cuda.device(dev):
            torch.cuda.current_stream().synchronize()        # (the engine made here goes away with the call)
    pics = [p[0] for p in planes]
    return [p.permute(2, 0, 1) for p in pics] if chw and fmt == SRC_RGB else pics


def _sheet_flatten(who, flatten, sheet):
    """the Flatten of a sheet call: None (today's call); True -- over the sheet's own background; three bytes -- over
    that background; a Flatten or a Flattened -- its description (a Flattened's pictures are not looked at)"""
    if flatten is None or flatten is False:
        return None
    if flatten is True:
        if not isinstance(sheet, Sheet):
            raise SjpegError(f"{who}: sheet is not a Sheet")
        return Flatten(sheet.background)
    if isinstance(flatten, Flattened):
        return flatten.flatten
    if isinstance(flatten, Flatten):
        return flatten
    if isinstance(flatten, (tuple, list, np.ndarray)):
        return Flatten(*flatten) if len(flatten) != 3 or isinstance(flatten[0], (tuple, list, np.ndarray)) else Flatten(tuple(flatten))
    raise SjpegError(f"{who}: flatten is None, True (over the sheet's background), a background (R, G, B), a tuple "
                     f"(background, premultiplied, alpha_scale, alpha_bias) or a Flatten")


def _sheet_pictures(who, images, layout, flatten=None):
    """(planes, dims, device, format, FloatPixels or None) of the pictures a sheet call takes: those of resize_images;
    with a flatten, those of flatten_images"""
    chw = _check_layout(who, layout)
    if isinstance(images, (Reduced, Resized, Oriented, Flattened)):
        raise SjpegError(f"{who}: Reduced, Resized, Oriented and Flattened pictures are not taken: give sizes, orientations and "
                         f"flatten to the call")
    if flatten is not None and chw:
        raise SjpegError(f"{who}: layout='chw' has no alpha format: flatten takes [H, W, 4] pictures, layout='hwc'")
    if flatten is not None:
        fp = images if isinstance(images, FloatPixels) else None
        images = images.images if fp is not None else images
    else:
        images, fp = _float_pixels(who, images, chw)
    return _pictures(who, images, chw, fp, alpha=flatten is not None) + (fp,)


def _orientation_list(who, n, orientations):
    """the orientations of a call -- None, one EXIF value or one per picture -- as a list of n ints, or None"""
    return None if orientations is None else [int(o) for o in _orientations_array(who, n, _per_picture(orientations, n))]


def make_sheets(images, sheet, sizes=None, orientations=None, engine=None, layout="hwc", flatten=None):
    """The uint8 contact sheets of a batch, as views of ONE device buffer: images as resize_images takes them
    (layout="hwc": CUDA uint8 tensors [H_k, W_k, 3]; "chw": channel-first uint8 tensors or a FloatPixels -- a network's
    [N, 3, H, W] float output), each resized to sizes[k] = (w, h) in the stored orientation (None: fitted into its cell,
    never enlarged), turned upright by orientations (one EXIF value 1..8 or one per picture) and stored centred into its
    cell of the Sheet -- a background fill and one launch, no thumbnail made a second time.  Returns uint8 CUDA tensors
    [SH, SW, 3] (gray FloatPixels: [SH, SW]), rows padded to a multiple of 4 bytes; sheet_places gives the rectangles.
    flatten (default None: today's call): the pictures are [H_k, W_k, 4] RGBA (uint8 tensors, or a FloatPixels of float
    ones) and are laid over a background first, as Flattened defines it -- True: over the sheet's own background;
    (R, G, B): over that one; a Flatten: with every field of it."""
    import torch
    who = "make_sheets"
    flatten = _sheet_flatten(who, flatten, sheet)
    planes, dims, dev, fmt, fp = _sheet_pictures(who, images, layout, flatten)
    eng = _engine_for(engine, dev, fp)
    with torch.cuda.device(dev):
        _, sheets, _ = eng.sheet_ragged(fmt, planes, dims, sheet, sizes, _orientation_list(who, len(dims), orientations), flatten=flatten)
        if engine is None:
            torch.cuda.current_stream().synchronize()        # (the engine made here goes away with the call)
    return sheets


def _encode_sheets(who, eng, dev, fmt, planes, dims, sheet, sizes, orientations, yuv_mode, quality, method, use_trellis,
                   target_size, target_psnr, packed, metadata, flatten=None):
    """the rest of encode_sheets / encode_yuv_sheets: (list of JPEG bytes, places)"""
    import torch
    places = sheet_places(sheet, dims, fmt, sizes, orientations)
    ns = places[-1][0] + 1
    method = int(method)
    if use_trellis:
        method = {4: 7, 6: 8}.get(method, method)
    qs = _per_picture(quality, ns)
    if len(qs) != ns:
        raise SjpegError(f"{who}: one quality per sheet")
    _one_target(who, target_size, target_psnr)
    search = _target_search(who, "sheet", ns, target_size, target_psnr)
    with torch.cuda.device(dev):
        if packed:
            out, sz, offs, _, _, _ = eng.encode_ragged_sheet_packed(fmt, planes, dims, sheet, sizes, orientations, yuv_mode,
                                                                    _quality_quant(qs), method, search=search, metadata=metadata,
                                                                    flatten=flatten)
            eng.wait()
            return _fetch_packed(out, sz, offs, ns, "sheet"), places
        out, sz, offs, _, _, _ = eng.encode_ragged_sheet(fmt, planes, dims, sheet, sizes, orientations, yuv_mode,
                                                         _quality_quant(qs), method, search=search, metadata=metadata,
                                                         flatten=flatten)
        eng.wait()                               # (pipelined mode: the output is complete after this)
        return _fetch_ragged(out, sz, offs), places


def encode_sheets(images, sheet, sizes=None, orientations=None, quality=75.0, yuv_mode=YUV_AUTO, method=4, use_trellis=False,
                  target_size=None, target_psnr=None, packed=False, metadata=None, layout="hwc", engine=None, flatten=None):
    """The contact-sheet call: (JPEGs, places) -- the JPEGs (list of bytes, one per sheet) of the sheets make_sheets makes
    of the same pictures, each byte for byte what encode_images_full makes of that sheet, and places[k] = (sheet, x, y, w,
    h), the rectangle of picture k (a storyboard's #xywh=).  quality, target_size / target_psnr and metadata: one for all
    sheets or one per SHEET; yuv_mode as encode_images_full (YUV_AUTO decides on the sheet; gray FloatPixels: YUV_400);
    use_trellis maps method 4 to 7 and 6 to 8; packed=True: through the packed entry and one device-to-host copy.
    flatten: as make_sheets takes it -- RGBA pictures laid over a background first."""
    who = "encode_sheets"
    flatten = _sheet_flatten(who, flatten, sheet)
    planes, dims, dev, fmt, fp = _sheet_pictures(who, images, layout, flatten)
    _gray_mode(who, fmt, int(yuv_mode))
    eng = _engine_for(engine, dev, fp)
    return _encode_sheets(who, eng, dev, fmt, planes, dims, sheet, sizes, _orientation_list(who, len(dims), orientations),
                          int(yuv_mode), quality, method, use_trellis, target_size, target_psnr, packed, metadata, flatten)


def _yuv_frames(who, frames, fmt):
    """(planes, dims, device) of the frames a YUV call takes: frames[k] = (y, uv) for SRC_NV12 / SRC_NV21 or (y, u, v)
    for SRC_YUV420 / SRC_YUV444, every plane a uint8 CUDA tensor [rows, bytes] with stride 1 along a row"""
    import torch
    frames = [tuple(fr) for fr in frames]
    if not frames:
        raise SjpegError(f"{who}: no frames")
    nplanes = 2 if fmt in (SRC_NV12, SRC_NV21) else 3 if fmt in (SRC_YUV420, SRC_YUV444) else 0
    if nplanes == 0:
        raise SjpegError(f"{who}: fmt {fmt} is not SRC_NV12, SRC_NV21, SRC_YUV420 or SRC_YUV444")
    for k, fr in enumerate(frames):
        if len(fr) != nplanes:
            raise SjpegError(f"{who}: frame {k} has {len(fr)} planes, the format takes {nplanes}")
        for p in fr:
            if not isinstance(p, torch.Tensor) or not p.is_cuda or p.dtype != torch.uint8 or p.dim() != 2 or p.stride(1) != 1:
                raise SjpegError(f"{who}: frame {k}: a plane is a uint8 CUDA tensor [rows, bytes] with stride 1 along a row")
    return [list(fr) for fr in frames], [(int(fr[0].shape[1]), int(fr[0].shape[0])) for fr in frames], frames[0][0].device


def _fetch_packed(out, sizes, offsets, n, what):
    """The JPEGs of a packed call as byte strings: one copy of the sizes and offsets, ONE of the frames."""
    import torch
    meta = torch.cat([sizes, offsets]).cpu().numpy()
    sz, offs = meta[:n], meta[n:2 * n]
    if (sz <= 0).any():
        raise SjpegError("%s %d did not fit its output capacity (the device reported size 0)" % (what, int(np.argmax(sz <= 0))))
    top = int(max(offs[k] + sz[k] for k in range(n)))
    host = out[:top].cpu().numpy()
    return [host[int(offs[k]):int(offs[k] + sz[k])].tobytes() for k in range(n)]


def encode_yuv_sheets(frames, fmt=SRC_NV12, sheet=None, sizes=None, orientations=None, quality=75.0, method=4,
                      target_size=None, target_psnr=None, packed=False, metadata=None, engine=None):
    """encode_sheets for decoded video, shaped like encode_yuv_frames: frames[k] = (y, uv) for SRC_NV12 / SRC_NV21 or
    (y, u, v) for SRC_YUV420 / SRC_YUV444, each resized plane by plane (sizes None: fitted into its cell), turned and
    stored into its cell -- chroma at half the luma's place for the 4:2:0 formats, whose Sheet takes even cells, gutter
    and margin; background is (Y, U, V).  No colour conversion: the sheets are coded 4:2:0 (SRC_YUV444: 4:4:4) --
    sjpeg_amd.video.encode_video_sheets converts BT.709 and limited-range frames to JFIF's colour inside the call.
    Returns (JPEGs, places) as encode_sheets -- the storyboard behind a scrub bar in one call."""
    who = "encode_yuv_sheets"
    planes, dims, dev = _yuv_frames(who, frames, fmt)
    eng = _engine_for(engine, dev)
    return _encode_sheets(who, eng, dev, fmt, planes, dims, sheet, sizes, _orientation_list(who, len(dims), orientations),
                          YUV_444 if fmt == SRC_YUV444 else YUV_420, quality, method, False, target_size, target_psnr, packed,
                          metadata)


_packed_stats = {"calls": 0, "retries": 0}


def encode_yuv_frames(frames, fmt=SRC_NV12, sizes=None, box=None, orientations=None, quality=75.0, method=4,
                      target_size=None, target_psnr=None, packed=False, metadata=None, engine=None):
    """The thumbnail call for decoded video: JPEGs (list of bytes) of device-resident frames in one of the YUV-plane
    formats -- frames[k] = (y, uv) for SRC_NV12 / SRC_NV21 ([H, W] and [(H + 1) // 2, 2 * ((W + 1) // 2)] uint8 CUDA
    tensors) or (y, u, v) for SRC_YUV420 / SRC_YUV444 --, each resized to sizes[k] = (w, h) or fitted into box = (bw, bh)
    (fit_size; the box is the UPRIGHT one) and turned upright by orientations (one EXIF value 1..8 or one per frame),
    in one ragged call with no colour conversion: the frames are coded 4:2:0 (SRC_YUV444: 4:4:4) as they are sampled
    (right for full-range BT.601 frames; sjpeg_amd.video.encode_video_frames converts BT.709 and limited-range ones).
    quality: one value or one per frame; target_size / target_psnr: a per-frame search as encode_images_full;
    packed=True: through the packed entry and one device-to-host copy; metadata: as encode_images."""
    import torch
    who = "encode_yuv_frames"
    planes, dims, dev = _yuv_frames(who, frames, fmt)
    n = len(dims)
    if sizes is not None and box is not None:
        raise SjpegError(f"{who}: give sizes or box, not both")
    orientations = _orientation_list(who, n, orientations)
    if box is not None:
        try:
            bw, bh = box
        except (TypeError, ValueError):
            raise SjpegError(f"{who}: box {box!r} is not a pair (width, height)")
        sizes = [fit_size(w, h, (bh, bw) if orientations is not None and orientations[k] >= 5 else (bw, bh))
                 for k, (w, h) in enumerate(dims)]
    _one_target(who, target_size, target_psnr)
    search = _target_search(who, "frame", n, target_size, target_psnr)
    qs = _per_picture(quality, n)
    if len(qs) != n:
        raise SjpegError(f"{who}: one quality per frame")
    yuv_mode = YUV_444 if fmt == SRC_YUV444 else YUV_420
    eng = _engine_for(engine, dev)
    with torch.cuda.device(dev):
        if packed:
            out, sz, offs, _, _, _ = eng.encode_ragged_yuv_resized_packed(fmt, planes, dims, sizes, orientations, yuv_mode,
                                                                          _quality_quant(qs), method, search=search,
                                                                          metadata=metadata)
            eng.wait()
            return _fetch_packed(out, sz, offs, n, "frame")
        out, sz, offs, _, _, _ = eng.encode_ragged_yuv_resized(fmt, planes, dims, sizes, orientations, yuv_mode,
                                                               _quality_quant(qs), method, search=search, metadata=metadata)
        eng.wait()                               # (pipelined mode: the output is complete after this)
        return _fetch_ragged(out, sz, offs)


def packed_stats():
    """Counters of encode_images(packed=True): calls, and how many of them needed the second packed call."""
    return dict(_packed_stats)


def _first_pool(dims, yuv_mode):
    """The first pool of encode_images(packed=True): per picture 2048 bytes of header allowance plus half a byte per
    sample (the host API's first capacity without its 64 KiB per picture), each rounded up to 16; at least 64 KiB."""
    total = 0
    for (w, h) in dims:
        px = w * h
        samples = 3 * px if yuv_mode in (YUV_444, YUV_AUTO) else px if yuv_mode == YUV_400 else px + px // 2
        total += (2048 + samples // 2 + 15) & ~15
    return max(total, 65536)


def _encode_images_packed(eng, planes, dims, yuv_mode, quant, method, min_quant, q_bias, dmax_luma, dmax_chroma, search,
                          stem="", fmt=SRC_RGB, metadata=None):
    """encode_images through the packed call: a small first pool, one copy of sizes and offsets, one of the pool; the
    pictures a full pool dropped go through a second packed call whose pool is the sum of their bounds."""
    import torch
    n = len(dims)
    _packed_stats["calls"] += 1
    bound_mode = YUV_444 if yuv_mode in (YUV_AUTO, YUV_SHARP) else yuv_mode
    _, _, msizes, metas = _metadata_args("encode_images", n, metadata)
    bounds = [frame_bound(w, h, bound_mode, 2048 + msizes[k]) for k, (w, h) in enumerate(dims)]

    def run(which, pool):
        m = len(which)
        out, meta, _, _, _ = eng._encode_ragged_packed(
            fmt, [planes[k] for k in which], [dims[k] for k in which], yuv_mode,
            [quant[k] for k in which] if isinstance(quant, list) else quant, method, min_quant, q_bias, dmax_luma,
            dmax_chroma, None if search is None else [search[k] for k in which], [bounds[k] for k in which], pool, None,
            stem, None if metadata is None else [metas[k] for k in which], one_tensor=True)
        eng.wait()                               # (pipelined mode: the output is complete after this)
        meta = meta.cpu().numpy()                # sizes and offsets together
        sz, off, end = meta[:m], meta[m:2 * m], int(meta[2 * m])
        over = end < 0                           # (bit 63 of the int64)
        top = max((int(off[i] + sz[i]) for i in range(m) if sz[i] > 0), default=0)
        stage = torch.empty(max(top, 1), dtype=torch.uint8, pin_memory=True)
        stage[:top].copy_(out[:top], non_blocking=True)      # the ONE copy of the pictures
        torch.cuda.synchronize()
        host = stage.numpy()
        return [host[int(off[i]):int(off[i] + sz[i])].tobytes() if sz[i] > 0 else None for i in range(m)], over

    got, over = run(list(range(n)), _first_pool(dims, yuv_mode) + sum((s + 15) & ~15 for s in msizes))
    again = [k for k in range(n) if got[k] is None]
    if again and not over:
        raise SjpegError("frame %d did not fit its output capacity (the device reported size 0)" % again[0])
    if again:
        _packed_stats["retries"] += 1
        more, _ = run(again, sum((bounds[k] + 15) & ~15 for k in again))
        for k, b in zip(again, more):
            if b is None:
                raise SjpegError("frame %d did not fit its output capacity (the device reported size 0)" % k)
            got[k] = b
    return got


def _fetch_ragged(out, sizes, offsets):
    """The JPEGs of a ragged call as byte strings: one pinned staging buffer, one synchronisation."""
    import torch
    sz = sizes.cpu().numpy()
    if (sz <= 0).any():
        raise SjpegError("frame %d did not fit its output capacity (the device reported size 0)" % int(np.argmax(sz <= 0)))
    at = np.concatenate([[0], np.cumsum(sz)]).astype(np.int64)
    stage = torch.empty(int(at[-1]), dtype=torch.uint8, pin_memory=True)
    for k in range(len(sz)):
        stage[int(at[k]):int(at[k + 1])].copy_(out[int(offsets[k]):int(offsets[k]) + int(sz[k])], non_blocking=True)
    torch.cuda.synchronize()
    host = stage.numpy()
    return [host[int(at[k]):int(at[k + 1])].tobytes() for k in range(len(sz))]


def encode_device_method(frames, quality=75.0, yuv_mode=YUV_420, method=4, engine=None, quant=None,
                         min_quant=None, q_bias=0x78, dmax_luma=12, dmax_chroma=1):
    """Per-frame adaptive quantization / optimised Huffman tables (reference methods 0..6) for a
    batch of device-resident frames [F, H, W, 3]: one call of sjpeg_hip_encode_batch_src (every
    device pass is one launch over the batch).  Returns a list of JPEG byte strings."""
    eng = engine or Engine(frames.device.index or 0)
    method = max(0, min(int(method), 8))
    if method >= 7:
        raise SjpegError("trellis methods: use the host API (SjpegEncode / sjpeg::Encode)")
    f, h, w, _ = frames.shape
    assert frames.stride(3) == 1 and frames.stride(2) == 3
    rows = frames.as_strided((f, h, w * 3), (frames.stride(0), frames.stride(1), 1))
    src, _ = make_source(SRC_RGB, [rows])
    if quant is None:
        q = np.zeros((2, 64), np.uint8)
        lib().sjpeg_hip_quality_matrices(float(quality), q.ctypes.data)
    else:
        q = np.asarray(quant, np.uint8).reshape(2, 64)
    out, sizes = eng.encode_batch(src, f, w, h, yuv_mode, q, method, min_quant, q_bias, dmax_luma, dmax_chroma,
                                  device=frames.device)
    eng.wait()                                   # (pipelined mode: the output is complete after this)
    return _fetch_frames(out, sizes)


def _fetch_frames(out, sizes):
    """The batch's JPEGs as byte strings: the used part of every slot, one pinned staging buffer,
    one synchronisation."""
    import torch
    sz = sizes.cpu().numpy()
    if (sz <= 0).any():
        raise SjpegError("frame %d did not fit its output slot (the device reported size 0): raise out_stride"
                         % int(np.argmax(sz <= 0)))
    offs = np.concatenate([[0], np.cumsum(sz)]).astype(np.int64)
    stage = torch.empty(int(offs[-1]), dtype=torch.uint8, pin_memory=True)
    for k in range(len(sz)):
        stage[int(offs[k]):int(offs[k + 1])].copy_(out[k, :int(sz[k])], non_blocking=True)
    torch.cuda.synchronize()
    host = stage.numpy()
    return [host[int(offs[k]):int(offs[k + 1])].tobytes() for k in range(len(sz))]


def encode_source_method(fmt, planes, w, h, quality=75.0, yuv_mode=YUV_420, method=0, engine=None,
                         quant=None, min_quant=None, q_bias=0x78, dmax_luma=12, dmax_chroma=1):
    """One frame in any source layout (planes: CUDA uint8 tensors [1, rows, row_bytes]) with the
    reference's method 0..6 semantics, through the C-ABI.  Returns the JPEG bytes."""
    import torch
    eng = engine or Engine(planes[0].device.index or 0)
    yuv_mode = _IMPLIED_MODE.get(fmt, yuv_mode)
    method = max(0, min(int(method), 8))
    adaptive, optimize = method >= 3, method not in (0, 3)
    src, n = make_source(fmt, planes)
    assert n == 1
    tables, q = make_tables(quality=quality, quant=quant, min_quant=min_quant, q_bias=q_bias)
    if adaptive:
        hist = eng.scan_histogram_source(src, 1, w, h, yuv_mode).cpu().numpy().view(np.uint32)[0]
        tables, q = adapt_quant(hist, yuv_mode, q, min_quant, q_bias, dmax_luma, dmax_chroma)
    specs = None
    if optimize:
        freq = eng.scan_symbol_stats_source(src, 1, w, h, tables, yuv_mode).cpu().numpy().view(np.uint32)[0]
        specs = optimize_huffman(freq, yuv_mode, tables)
    header = make_header_ex(w, h, yuv_mode, q, specs)
    out, sizes = eng.encode_source(src, 1, w, h, tables, header, yuv_mode)
    return _fetch_frames(out, sizes)[0]


def encode_device(frames, quality=75.0, yuv_mode=YUV_420, engine=None, quant=None):
    """Convenience: list of JPEG byte strings for device-resident frames [F, H, W, 3]."""
    import torch
    eng = engine or Engine(frames.device.index or 0)
    tables, q = make_tables(quality=quality, quant=quant)
    f, h, w, _ = frames.shape
    header = make_header(w, h, yuv_mode, q)
    out, sizes = eng.encode_frames(frames, tables, header, yuv_mode)
    eng.wait()                                   # (pipelined mode: the output is complete after this)
    return _fetch_frames(out, sizes)
