"""Pictures resampled with Pillow's filters inside the ragged call (sjpeg_hip.h, "resampling with Pillow's filters").
Every other shape entry makes its picture with the exact area average: it only shrinks, it is soft, and it is this
library's own answer.  The calls here make the bytes PIL.Image.resize(size, LANCZOS | BICUBIC | BILINEAR | HAMMING |
BOX) of Pillow 12.2.0 makes of a picture of bytes -- along x, then along y, with a uint8 intermediate, integers only
given the tables -- in ONE launch over the batch, to sizes smaller or larger than the source on either axis.  The
tables are built on the host (resample_table shows one) and uploaded once per (filter, in, out) of a call.  Order of
steps: pixel transform, flatten, resample, turn, unsharp.  sizes are in the STORED orientation: the upright picture is
turn(resample(stored)) -- NOT exif_transpose followed by resize, which rounds its intermediate along the other axis.
There is no linear light and there are no contact sheets here; the YUV-plane formats are refused.

Thumbnails are mostly not made by a bare resize.  source_box= and reducing_gap= make the bytes of Image.resize(size,
filter, box=, reducing_gap=): a fractional source box inside the tables, and Pillow's integer reduce -- its own
rounding, not this library's half-up average -- in front of the resample where the source is at least 2 * gap times the
target, summed as the rows are staged.  thumbnail_images / encode_thumbnails follow Image.thumbnail and fit_images /
encode_fitted_images ImageOps.fit; thumbnail_size and fit_crop are their size and crop rules.  With an orientation,
boxes and sizes are in the STORED orientation and the result is turn(...) of what Pillow makes of the stored picture.
A picture more than 100 times as tall as wide brought to fewer rows is resampled along y first by Pillow: the calls with
a source_box or a reducing_gap refuse it; the plain calls do not, and for such a picture they do not make Pillow's bytes.

The chain of a Python thumbnailer ends in im.filter(...).  post= (a PillowFilter, or one per picture) runs Pillow
12.2.0's BoxBlur, GaussianBlur or UnsharpMask over the made upright picture as the call's last step --
filter(turn(resample(flatten(stored)))) -- in two launches over the batch (sjpeg_hip.h, "Pillow's GaussianBlur, BoxBlur
and UnsharpMask"); it goes through the box entries and excludes unsharp=, the 3 x 3 mask of this library's own.

Two links often stand between filter and save: ImageOps.pad / expand and im.paste(logo, (x, y), logo).  compose= (a
Compose, or one per picture) runs both as the call's very last step, in ONE launch over the batch's canvases --
compose(filter(turn(resample(flatten(stored))))) -- in the UPRIGHT picture's coordinates and to Pillow's bytes
(sjpeg_hip.h, "composed behind that").  pad_images / encode_padded_images are ImageOps.pad of the upright picture."""
import ctypes as C
import enum

import numpy as np

import sjpeg_amd as sj
import sjpeg_amd.light as li
import sjpeg_amd.unsharp as un
from sjpeg_amd import YUV_420, SjpegError

KSIZE_MAX = 385          # an axis whose window is longer is refused (Lanczos shrinking by more than 64, box by more than 384)


class Filter(enum.IntEnum):
    """SJPEG_HIP_RESAMPLE_*: Pillow's Image.BOX, BILINEAR, HAMMING, BICUBIC and LANCZOS"""
    BOX = 0
    BILINEAR = 1
    HAMMING = 2
    BICUBIC = 3
    LANCZOS = 4


class _BoxStruct(C.Structure):
    """struct sjpeg_hip_resample_box"""
    _fields_ = [("box", C.c_double * 4), ("reducing_gap", C.c_double)]


class _DecisionStruct(C.Structure):
    """struct sjpeg_hip_resample_box_decision"""
    _fields_ = [("factor", C.c_int32 * 2), ("safe_box", C.c_int32 * 4), ("reduced_size", C.c_int32 * 2), ("multiplier", C.c_uint32 * 4),
                ("inner_box", C.c_double * 4)]


class _ResampleStruct(C.Structure):
    """struct sjpeg_hip_resample"""
    _fields_ = [("filter", C.c_uint8), ("reserved", C.c_uint8 * 3)]


_lib = sj.lib                            # (the one table of sjpeg_amd._binding binds every entry when the library loads)


def _last_error():
    return (_lib().sjpeg_hip_last_error() or b"").decode()


def _filter(who, f):
    if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or int(f) not in tuple(int(v) for v in Filter):
        raise SjpegError(f"{who}: filter {f!r} is not a Filter (BOX 0, BILINEAR 1, HAMMING 2, BICUBIC 3, LANCZOS 4)")
    return int(f)


def _filter_args(who, n, filter):
    """(the struct array, its address, whether there is one per frame) of one Filter or a sequence of one per frame"""
    if isinstance(filter, (int, np.integer)) and not isinstance(filter, bool):
        arr = (_ResampleStruct * 1)(_ResampleStruct(_filter(who, filter)))
        return arr, C.addressof(arr), 0
    try:
        fs = list(filter)
    except TypeError:
        raise SjpegError(f"{who}: filter {filter!r} is not a Filter or a sequence of one per frame")
    if len(fs) != n:
        raise SjpegError(f"{who}: filter is one Filter or a sequence of one per frame ({n})")
    arr = (_ResampleStruct * n)(*[_ResampleStruct(_filter(who, f)) for f in fs])
    return arr, C.addressof(arr), 1


def resample_ksize(filter, n_in, n_out):
    """sjpeg_hip_resample_ksize: the coefficients a row of the table of an axis has room for.  Host only."""
    k = _lib().sjpeg_hip_resample_ksize(_filter("resample_ksize", filter), int(n_in), int(n_out))
    if k == 0:
        raise SjpegError(f"sjpeg_hip_resample_ksize failed: {_last_error()}")
    return k


def resample_table(filter, n_in, n_out):
    """sjpeg_hip_resample_table: (bounds int32 [n_out, 2] -- xmin and n of every output sample --, K int32 [n_out, ksize]
    -- its coefficients in 2^-22, the rest of a row 0) of an axis from n_in to n_out samples.  Host only."""
    ks = resample_ksize(filter, n_in, n_out)
    bounds, K = np.zeros((int(n_out), 2), np.int32), np.zeros((int(n_out), ks), np.int32)
    if _lib().sjpeg_hip_resample_table(int(filter), int(n_in), int(n_out), bounds.ctypes.data, K.ctypes.data, K.size) != 0:
        raise SjpegError(f"sjpeg_hip_resample_table failed: {_last_error()}")
    return bounds, K


def resample_box_table(filter, n_in, n_out, b0, b1):
    """sjpeg_hip_resample_box_table: resample_table of an axis of n_in samples brought to n_out from its part [b0, b1),
    the two ends rounded to float32 as Pillow's C layer receives them.  Host only."""
    L = _lib()
    b0, b1 = float(np.float32(b0)), float(np.float32(b1))
    ks = L.sjpeg_hip_resample_box_ksize(_filter("resample_box_table", filter), int(n_in), int(n_out), b0, b1)
    if ks == 0:
        raise SjpegError(f"sjpeg_hip_resample_box_ksize failed: {_last_error()}")
    bounds, K = np.zeros((int(n_out), 2), np.int32), np.zeros((int(n_out), ks), np.int32)
    if L.sjpeg_hip_resample_box_table(int(filter), int(n_in), int(n_out), b0, b1, bounds.ctypes.data, K.ctypes.data, K.size) != 0:
        raise SjpegError(f"sjpeg_hip_resample_box_table failed: {_last_error()}")
    return bounds, K


def thumbnail_size(width, height, box):
    """sjpeg_hip_thumbnail_size: the size Image.thumbnail(box) gives a width x height picture.  Host only."""
    try:
        bw, bh = box
    except (TypeError, ValueError):
        raise SjpegError(f"thumbnail_size: box {box!r} is not a pair (width, height)")
    out = (C.c_int32 * 2)()
    if _lib().sjpeg_hip_thumbnail_size(int(width), int(height), float(bw), float(bh), out) != 0:
        raise SjpegError(f"sjpeg_hip_thumbnail_size failed: {_last_error()}")
    return int(out[0]), int(out[1])


def fit_crop(width, height, size, bleed=0.0, centering=(0.5, 0.5)):
    """sjpeg_hip_fit_crop: the crop box (left, top, right, bottom), in doubles, that ImageOps.fit(im, size, bleed=,
    centering=) resizes a width x height picture from.  Host only."""
    out = (C.c_double * 4)()
    if _lib().sjpeg_hip_fit_crop(int(width), int(height), int(size[0]), int(size[1]), float(bleed), float(centering[0]), float(centering[1]),
                                 out) != 0:
        raise SjpegError(f"sjpeg_hip_fit_crop failed: {_last_error()}")
    return tuple(float(v) for v in out)


def box_decision(filter, width, height, size, source_box=None, reducing_gap=None):
    """sjpeg_hip_resample_box_decide: what the plan decides for one frame, as a dict: factor (fx, fy), safe_box,
    reduced_size, multiplier (interior, right edge, bottom edge, corner) and inner_box.  Host only."""
    b = _BoxStruct((C.c_double * 4)(*(source_box if source_box is not None else (0, 0, 0, 0))), float(reducing_gap or 0.0))
    d = _DecisionStruct()
    if _lib().sjpeg_hip_resample_box_decide(_filter("box_decision", filter), int(width), int(height), int(size[0]), int(size[1]), C.addressof(b),
                                            C.addressof(d)) != 0:
        raise SjpegError(f"sjpeg_hip_resample_box_decide failed: {_last_error()}")
    return {"factor": tuple(d.factor), "safe_box": tuple(d.safe_box), "reduced_size": tuple(d.reduced_size), "multiplier": tuple(d.multiplier),
            "inner_box": tuple(d.inner_box)}


def _box_args(who, n, source_box, reducing_gap):
    """(the struct array, its address, whether there is one per frame) of source_box -- None, one (l, t, r, b) or one
    per frame -- and reducing_gap -- None, one number or one per frame --; (None, None, 0) where neither is given: the
    call is the plain one"""
    if source_box is None and reducing_gap is None:
        return None, None, 0
    def one_box(b):
        if b is None:
            return (0.0, 0.0, 0.0, 0.0)
        try:
            l, t, r, bt = (float(v) for v in b)
        except (TypeError, ValueError):
            raise SjpegError(f"{who}: source_box {b!r} is not (left, top, right, bottom)")
        return (l, t, r, bt)
    def one_gap(g):
        if g is None:
            return 0.0
        if isinstance(g, bool) or not isinstance(g, (int, float, np.integer, np.floating)) or not float(g) >= 1.0:
            raise SjpegError(f"{who}: reducing_gap {g!r} is not None or a number of 1.0 or more")
        return float(g)
    number = (int, float, np.integer, np.floating)
    boxes_many = source_box is not None and not (len(source_box) == 4 and all(isinstance(v, number) for v in source_box))
    gaps_many = isinstance(reducing_gap, (tuple, list, np.ndarray))
    if boxes_many and len(source_box) != n:
        raise SjpegError(f"{who}: source_box is one box or a sequence of one per frame ({n})")
    if gaps_many and len(reducing_gap) != n:
        raise SjpegError(f"{who}: reducing_gap is one number or a sequence of one per frame ({n})")
    count = n if boxes_many or gaps_many else 1
    arr = (_BoxStruct * count)()
    for k in range(count):
        arr[k].box[:] = one_box(source_box[k] if boxes_many else source_box)
        arr[k].reducing_gap = one_gap(reducing_gap[k] if gaps_many else reducing_gap)
    return arr, C.addressof(arr), 1 if count == n and (boxes_many or gaps_many) else 0


# ---- Pillow's filters behind the resample: post=

class _FilterStruct(C.Structure):
    """struct sjpeg_hip_pillow_filter"""
    _fields_ = [("kind", C.c_uint8), ("threshold", C.c_uint8), ("percent", C.c_uint16), ("radius_x", C.c_float), ("radius_y", C.c_float),
                ("reserved", C.c_uint8 * 4)]


class PillowFilter:
    """What post= takes: PIL.ImageFilter's BoxBlur, GaussianBlur or UnsharpMask of Pillow 12.2.0, run over the made
    upright picture as the last step of the call -- filter(turn(resample(flatten(stored)))) -- in two launches over the
    batch.  radius is a number or (x, y), the upright picture's axes; an axis whose integer box radius exceeds 63 (a box
    radius of 64, a sigma above about 64) is refused, which Pillow does not."""
    NONE, BOX, GAUSSIAN, UNSHARP = 0, 1, 2, 3

    def __init__(self, kind, radius=(0.0, 0.0), percent=0, threshold=0):
        who = "PillowFilter"
        if isinstance(radius, (int, float, np.integer, np.floating)) and not isinstance(radius, bool):
            radius = (radius, radius)
        try:
            rx, ry = (float(v) for v in radius)
        except (TypeError, ValueError):
            raise SjpegError(f"{who}: radius {radius!r} is not a number or a pair (x, y)")
        if kind not in (0, 1, 2, 3):
            raise SjpegError(f"{who}: kind {kind!r} is not one of 0..3 (none, box, gaussian, unsharp mask)")
        for name, v, hi in (("percent", percent, 65535), ("threshold", threshold, 255)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= hi:
                raise SjpegError(f"{who}: {name} {v!r} is not an integer of 0..{hi}")
        self.kind, self.radius, self.percent, self.threshold = int(kind), (rx, ry), int(percent), int(threshold)

    @classmethod
    def none(cls):
        """the picture as it is made (a frame of a mixed batch that is not filtered)"""
        return cls(cls.NONE)

    @classmethod
    def box_blur(cls, radius):
        """ImageFilter.BoxBlur(radius)"""
        return cls(cls.BOX, radius)

    @classmethod
    def gaussian_blur(cls, radius=2):
        """ImageFilter.GaussianBlur(radius)"""
        return cls(cls.GAUSSIAN, radius)

    @classmethod
    def unsharp_mask(cls, radius=2, percent=150, threshold=3):
        """ImageFilter.UnsharpMask(radius, percent, threshold)"""
        if not isinstance(radius, (int, float, np.integer, np.floating)) or isinstance(radius, bool):
            raise SjpegError(f"PillowFilter: an unsharp mask has one radius, not {radius!r}")
        return cls(cls.UNSHARP, radius, percent, threshold)

    def __repr__(self):
        return f"PillowFilter(kind={self.kind}, radius={self.radius}, percent={self.percent}, threshold={self.threshold})"

    def _struct(self):
        return _FilterStruct(self.kind, self.threshold, self.percent, self.radius[0], self.radius[1])


def _post_args(who, n, post, unsharp=None):
    """(the struct array, its address, whether there is one per frame) of post -- None, one PillowFilter or one per
    frame (None in a sequence: that frame is not filtered); (None, None, 0) for None"""
    if post is None:
        return None, None, 0
    if unsharp is not None:
        raise SjpegError(f"{who}: post= and unsharp= are both given: a call has one last step, Pillow's filter (post=) or the 3 x 3 mask (unsharp=)")
    if isinstance(post, PillowFilter):
        arr = (_FilterStruct * 1)(post._struct())
        return arr, C.addressof(arr), 0
    try:
        ps = list(post)
    except TypeError:
        raise SjpegError(f"{who}: post {post!r} is not a PillowFilter or a sequence of one per frame")
    if len(ps) != n or not all(p is None or isinstance(p, PillowFilter) for p in ps):
        raise SjpegError(f"{who}: post is one PillowFilter or a sequence of one (or None) per frame ({n})")
    arr = (_FilterStruct * n)(*[(p if p is not None else PillowFilter.none())._struct() for p in ps])
    return arr, C.addressof(arr), 1


def pillow_filter_weights(kind, radius):
    """sjpeg_hip_pillow_filter_weights: (r, ww, fw, passes) of one axis of a kind (PillowFilter.BOX, GAUSSIAN or
    UNSHARP) with `radius`, a box radius or a sigma; passes 0: the axis is skipped.  Host only."""
    out = [C.c_uint32() for _ in range(4)]
    if _lib().sjpeg_hip_pillow_filter_weights(int(kind), float(np.float32(radius)), *[C.addressof(v) for v in out]) != 0:
        raise SjpegError(f"sjpeg_hip_pillow_filter_weights failed: {_last_error()}")
    return tuple(int(v.value) for v in out)


def _whole_box():
    """the box entries' own words for a call without source_box and reducing_gap: the picture of the plain entries"""
    arr = (_BoxStruct * 1)()
    return arr, C.addressof(arr), 0


# ---- a canvas and overlays behind everything else: compose=

class _OverlayStruct(C.Structure):
    """struct sjpeg_hip_overlay"""
    _fields_ = [("rgba", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int64)]


class _PlaceStruct(C.Structure):
    """struct sjpeg_hip_overlay_place"""
    _fields_ = [("overlay", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("anchor", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class _ComposeStruct(C.Structure):
    """struct sjpeg_hip_compose"""
    _fields_ = [("canvas_width", C.c_int32), ("canvas_height", C.c_int32), ("mode", C.c_uint8), ("colour", C.c_uint8 * 3), ("px", C.c_int32),
                ("py", C.c_int32), ("reserved", C.c_uint8 * 4), ("cx", C.c_double), ("cy", C.c_double), ("first_place", C.c_int32),
                ("nplaces", C.c_int32)]


ANCHORS = {"top-left": 0, "top-right": 1, "bottom-left": 2, "bottom-right": 3, "centre": 4, "center": 4}
PLACES_MAX = 8           # overlay places one picture may have


class Overlay:
    """A watermark, logo or badge: a uint8 CUDA tensor [h, w, 4] of straight-alpha R, G, B, A bytes, of any row stride
    that is a multiple of 4 bytes -- a crop of a larger tensor is one.  It is given to the call once, referenced by
    every picture that places it, and never copied."""

    def __init__(self, tensor):
        import torch
        who = "Overlay"
        if not isinstance(tensor, torch.Tensor) or tensor.dtype != torch.uint8 or not tensor.is_cuda or tensor.dim() != 3 or tensor.shape[2] != 4:
            raise SjpegError(f"{who}: not a uint8 CUDA tensor [h, w, 4]")
        h, w = int(tensor.shape[0]), int(tensor.shape[1])
        if not (1 <= w <= 65535 and 1 <= h <= 65535):
            raise SjpegError(f"{who}: width {w} or height {h} is not one of 1..65535")
        if tensor.stride(2) != 1 or tensor.stride(1) != 4 or (h > 1 and (tensor.stride(0) < 4 * w or tensor.stride(0) % 4 != 0)) or tensor.data_ptr() % 4 != 0:
            raise SjpegError(f"{who}: pixels must be 4 bytes apart, rows a multiple of 4 bytes and at least 4 * width apart, the first pixel at a multiple of 4")
        self.tensor, self.width, self.height = tensor, w, h
        self.stride = int(tensor.stride(0)) if h > 1 else 4 * w

    def _struct(self):
        return _OverlayStruct(self.tensor.data_ptr(), self.width, self.height, self.stride)


def _colour(who, colour):
    if isinstance(colour, (int, np.integer)) and not isinstance(colour, bool):
        colour = (colour,) * 3
    try:
        c = tuple(int(v) for v in colour)
    except (TypeError, ValueError):
        c = ()
    if len(c) != 3 or not all(0 <= v <= 255 for v in c):
        raise SjpegError(f"{who}: colour {colour!r} is not one byte or (r, g, b) bytes")
    return c


def _pair(who, name, v, kind=int):
    try:
        a, b = v
        return kind(a), kind(b)
    except (TypeError, ValueError):
        raise SjpegError(f"{who}: {name} {v!r} is not a pair")


class Compose:
    """What compose= takes: the call's last step over the made UPRIGHT picture.  canvas=(cw, ch) filled with colour (a
    gray picture uses colour[0]) with the picture at at=(px, py) or, by ImageOps.pad's rule, at
    round((cw - w) * cx), round((ch - h) * cy) for centering=(cx, cy) (neither given: centred); canvas None: the picture's
    own size.  Then overlays, in list order: (overlay, (x, y), anchor) pastes the Overlay -- as
    im.paste(logo, (ox, oy), logo) does -- with (x, y) the margin inward from the anchor "top-left", "top-right",
    "bottom-left", "bottom-right" or "centre" of the CANVAS; clipped to it, over padding and picture alike.  One Compose
    can serve pictures of every size."""

    def __init__(self, canvas=None, at=None, centering=None, colour=(0, 0, 0), overlays=(), _border=None):
        who = "Compose"
        if at is not None and centering is not None:
            raise SjpegError(f"{who}: at= and centering= are both given")
        self.canvas = None if canvas is None else _pair(who, "canvas", canvas)
        self.at = None if at is None else _pair(who, "at", at)
        self.centering = None if centering is None else _pair(who, "centering", centering, float)
        self.colour, self.border = _colour(who, colour), _border
        self.overlays = []
        for item in overlays:
            try:
                ov, xy, anchor = item if len(item) == 3 else (item[0], item[1], "top-left")
            except (TypeError, IndexError, ValueError):
                raise SjpegError(f"{who}: an overlay place is (overlay, (x, y), anchor), not {item!r}")
            if not isinstance(ov, Overlay):
                raise SjpegError(f"{who}: {ov!r} is not an Overlay")
            code = ANCHORS.get(anchor, anchor) if isinstance(anchor, str) else anchor
            if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or not 0 <= int(code) <= 4:
                raise SjpegError(f"{who}: anchor {anchor!r} is not one of {sorted(set(ANCHORS))}")
            self.overlays.append((ov, _pair(who, "an overlay's (x, y)", xy), int(code)))
        if len(self.overlays) > PLACES_MAX:
            raise SjpegError(f"{who}: {len(self.overlays)} overlay places are more than {PLACES_MAX}")

    @classmethod
    def pad(cls, size, colour=(0, 0, 0), centering=(0.5, 0.5), overlays=()):
        """the canvas of ImageOps.pad(im, size, color=colour, centering=centering), for a picture that fits into size"""
        return cls(canvas=size, centering=centering, colour=colour, overlays=overlays)

    @classmethod
    def expand(cls, border=0, fill=0, overlays=()):
        """ImageOps.expand(im, border, fill): border one number, (left-right, top-bottom) or (left, top, right, bottom)"""
        b = (border,) * 4 if isinstance(border, (int, np.integer)) else tuple(border)
        if len(b) == 2:
            b = b + b
        if len(b) != 4 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v >= 0 for v in b):
            raise SjpegError(f"Compose.expand: border {border!r} is not one, two or four numbers of 0 and more")
        return cls(colour=fill, overlays=overlays, _border=tuple(int(v) for v in b))

    def _struct(self, size, first_place):
        """for an upright picture of `size` (a border needs it; None where the picture is not known: the ragged level)"""
        c = _ComposeStruct()
        canvas, at = self.canvas, self.at
        if self.border is not None:
            if size is None:
                raise SjpegError("Compose.expand: the picture's size is not known here; give canvas= and at=")
            l, t, r, b = self.border
            canvas, at = (size[0] + l + r, size[1] + t + b), (l, t)
        if canvas is not None:
            c.canvas_width, c.canvas_height = canvas
        c.colour[:] = self.colour
        if self.centering is not None:
            c.mode, c.cx, c.cy = 1, self.centering[0], self.centering[1]
        elif at is not None:
            c.px, c.py = at
        elif canvas is not None:
            c.mode, c.cx, c.cy = 1, 0.5, 0.5
        c.first_place, c.nplaces = first_place, len(self.overlays)
        return c


def _upright_sizes(dims, sizes, orientations):
    """the made upright pictures' sizes of a call: sizes[k] (None: the picture's own) turned by orientations[k]"""
    out = []
    for k, d in enumerate(dims):
        w, h = (int(v) for v in (sizes[k] if sizes is not None else d))
        out.append((h, w) if orientations is not None and int(orientations[k]) >= 5 else (w, h))
    return out


class _ComposeArgs:
    """what a C call takes for compose=: the six arguments, what they point into, and the canvases' sizes"""

    def __init__(self, who, n, compose, made_sizes):
        self.given = compose is not None
        self.args = (None, 0, None, 0, None, 0)
        self.canvases = list(made_sizes) if made_sizes is not None else None
        if compose is None:
            return
        one = isinstance(compose, Compose)
        if one:
            cs = [compose]
        else:
            try:
                cs = list(compose)
            except TypeError:
                raise SjpegError(f"{who}: compose {compose!r} is not a Compose or a sequence of one per frame")
            if len(cs) != n or not all(c is None or isinstance(c, Compose) for c in cs):
                raise SjpegError(f"{who}: compose is one Compose or a sequence of one (or None) per frame ({n})")
        if one and compose.border is not None:                    # (a border makes a canvas of every picture's own)
            one, cs = False, [compose] * n
        overlays, index, places, structs = [], {}, [], []
        for k, c in enumerate(cs):
            c = c if c is not None else Compose()
            structs.append(c._struct(None if made_sizes is None or one else made_sizes[k], len(places)))
            for ov, (x, y), anchor in c.overlays:
                if id(ov) not in index:
                    index[id(ov)] = len(overlays)
                    overlays.append(ov)
                places.append(_PlaceStruct(index[id(ov)], x, y, anchor))
        self.carr = (_ComposeStruct * len(structs))(*structs)
        self.oarr = (_OverlayStruct * max(len(overlays), 1))(*[o._struct() for o in overlays])
        self.parr = (_PlaceStruct * max(len(places), 1))(*places)
        self.keep = overlays
        self.args = (C.addressof(self.carr), 0 if one else 1, C.addressof(self.oarr) if overlays else None, len(overlays),
                     C.addressof(self.parr) if places else None, len(places))
        if self.canvases is not None:
            for k in range(n):
                c = structs[0 if one else k]
                if c.canvas_width or c.canvas_height:
                    self.canvases[k] = (int(c.canvas_width), int(c.canvas_height))


def _compose_args(who, n, compose, dims, sizes, orientations, unsharp=None):
    """_ComposeArgs of compose -- None, one Compose or one per frame -- over the made upright pictures of the call"""
    if compose is not None and unsharp is not None:
        raise SjpegError(f"{who}: compose= and unsharp= are both given: the compose stage stands behind Pillow's filter (post=), not the 3 x 3 mask")
    return _ComposeArgs(who, n, compose, _upright_sizes(dims, sizes, orientations) if compose is not None else None)


def contain_size(width, height, box):
    """sjpeg_hip_contain_size: the size ImageOps.contain(im, box) resizes a width x height picture to.  Host only."""
    bw, bh = _pair("contain_size", "box", box)
    out = (C.c_int32 * 2)()
    if _lib().sjpeg_hip_contain_size(int(width), int(height), bw, bh, out) != 0:
        raise SjpegError(f"sjpeg_hip_contain_size failed: {_last_error()}")
    return int(out[0]), int(out[1])


def pad_place(width, height, canvas, centering=(0.5, 0.5)):
    """sjpeg_hip_pad_place: where ImageOps.pad puts a width x height picture on `canvas` for `centering`.  Host only."""
    cw, ch = _pair("pad_place", "canvas", canvas)
    cx, cy = _pair("pad_place", "centering", centering, float)
    out = (C.c_int32 * 2)()
    if _lib().sjpeg_hip_pad_place(int(width), int(height), cw, ch, cx, cy, out) != 0:
        raise SjpegError(f"sjpeg_hip_pad_place failed: {_last_error()}")
    return int(out[0]), int(out[1])


def compose_sample(dst, src, alpha, gray=False):
    """sjpeg_hip_compose_sample: one sample of the paste -- dst under src with alpha; gray: src is (r, g, b), its luma
    is blended.  Host only."""
    r, g, b = (src if gray else (src, 0, 0))
    return int(_lib().sjpeg_hip_compose_sample(int(dst), int(r), int(g), int(b), int(alpha), 1 if gray else 0))


# ---- the ragged level: fmt, planes_per_frame and dims as Engine.encode_ragged takes them

def resample_ragged(engine, fmt, planes_per_frame, dims, sizes=None, filter=Filter.LANCZOS, orientations=None, flatten=None, unsharp=None,
                    out=None, source_box=None, reducing_gap=None, post=None, compose=None):
    """sjpeg_hip_resample_ragged_src: the pictures of a ragged batch resampled to sizes[k] = (w, h) (None: their own; the
    STORED orientation; larger or smaller than the source) with `filter` (one Filter or one per frame), turned upright
    and optionally sharpened.  source_box / reducing_gap (one or one per frame): sjpeg_hip_resample_box_ragged_src, the
    pictures of Image.resize(size, filter, box=, reducing_gap=).  post (one PillowFilter or one per frame):
    sjpeg_hip_filter_ragged_src, Pillow's BoxBlur, GaussianBlur or UnsharpMask over the upright pictures; it goes
    through the box entries, and not with unsharp.  compose (one Compose or one per frame): sjpeg_hip_compose_ragged_src,
    the canvases with their overlays; not with unsharp either.  Returns (fmt, pictures, buf) as Engine.orient_ragged does."""
    who = "resample_ragged"
    n = len(dims)
    if sizes is not None and len(sizes) != n:
        raise SjpegError(f"{who}: one size per frame")
    rkeep, raddr, rper = _filter_args(who, n, filter)
    bkeep, baddr, bper = _box_args(who, n, source_box, reducing_gap)
    pkeep, paddr, pper = _post_args(who, n, post, unsharp)
    ukeep, uaddr, uper = un._unsharp_args(who, n, unsharp)
    comp = _compose_args(who, n, compose, dims, sizes, orientations, unsharp)
    if (pkeep is not None or comp.given) and bkeep is None:
        bkeep, baddr, bper = _whole_box()
    frames, _, _, _ = sj._ragged_frames(planes_per_frame, dims, None, None, None, None)
    arr, oarr = sj._shape_arrays(who, n, sizes, orientations)
    keep, faddr = li._flat_struct(who, flatten)
    family, shape, more = _entry(faddr, (raddr, rper), (baddr, bper) if bkeep is not None else None, (uaddr, uper),
                                 (paddr, pper) if pkeep is not None or comp.given else None, comp)
    shape.update(sizes=sj._address(arr), orientations=sj._address(oarr))
    return engine._make_pictures(who, family[0], family[1], fmt, planes_per_frame, frames, shape, more, out)


def _entry(faddr, resample, box, unsharp, post, comp):
    """Which family a call goes through -- the plain resample; with a box (an (address, per-frame flag) pair) the box
    entries; with post the filter entries, which have it where the others have the unsharp; with a compose the compose
    entries --: (the stems of its picture-making entry, of the _bytes entry that goes with it and of its encodes, the
    segments the _bytes entry takes besides sizes and orientations, the other segments)"""
    shape, more = {}, {"flatten": faddr, "resample": resample}
    if box is None:
        return ("resample_ragged", "resample_ragged", "resampled"), shape, dict(more, unsharp=unsharp)
    shape["box"] = box
    if post is None:
        return ("resample_box_ragged", "resample_box_ragged", "resampled_box"), shape, dict(more, unsharp=unsharp)
    more["filter"] = post
    if not comp.given:
        return ("filter_ragged", "resample_box_ragged", "filtered"), shape, more
    shape["compose"] = comp.args[:2]
    return ("compose_ragged", "compose_ragged", "composed"), shape, dict(more, overlays=comp.args[2:4], places=comp.args[4:])


def encode_ragged_resampled(engine, fmt, planes_per_frame, dims, sizes, orientations, yuv_mode, quant, method=4, filter=Filter.LANCZOS,
                            flatten=None, unsharp=None, search=None, metadata=None, packed=False, min_quant=None, q_bias=0x78, dmax_luma=12,
                            dmax_chroma=1, source_box=None, reducing_gap=None, post=None, compose=None):
    """sjpeg_hip_encode_ragged_resampled_src / _resampled_packed_src (source_box, reducing_gap: the _resampled_box_
    entries; post: the _filtered_ ones; compose: the _composed_ ones, the default capacities the canvases' bounds).  Frame k's bytes are those Engine.encode_ragged_full makes of the uint8 picture
    resample_ragged returns.  Returns (out, sizes, offsets, modes, q, value)."""
    who = "encode_ragged_resampled"
    n = len(dims)
    rkeep, raddr, rper = _filter_args(who, n, filter)
    pkeep, paddr, pper = _post_args(who, n, post, unsharp)
    ukeep, uaddr, uper = un._unsharp_args(who, n, unsharp)
    comp = _compose_args(who, n, compose, dims, sizes, orientations, unsharp)
    capacities = None
    if comp.given:
        bound_mode = sj._bound_mode(yuv_mode)
        capacities = lambda msizes: [sj.frame_bound(w, h, bound_mode, 2048 + m) for (w, h), m in zip(comp.canvases, msizes)]
    call = engine._oriented_call(who, planes_per_frame, dims, sizes, orientations, yuv_mode, quant, method, min_quant, q_bias, dmax_luma,
                                 dmax_chroma, search, capacities, metadata)
    keep, faddr = li._flat_struct(who, flatten)
    bkeep, baddr, bper = _box_args(who, n, source_box, reducing_gap)
    if (pkeep is not None or comp.given) and bkeep is None:
        bkeep, baddr, bper = _whole_box()
    family, shape, more = _entry(faddr, (raddr, rper), (baddr, bper) if bkeep is not None else None, (uaddr, uper),
                                 (paddr, pper) if pkeep is not None or comp.given else None, comp)
    return engine._encode_shaped(who, family[2], fmt, planes_per_frame, dims, call,
                                 dict(shape, **more, sizes=call.sizes, orientations=call.orientations), packed)


# ---- the picture level: images as resize_images / flatten_images take them

def resample_images(images, sizes, filter=Filter.LANCZOS, orientations=None, flatten=None, engine=None, layout="hwc", source_box=None,
                    reducing_gap=None, post=None, compose=None, _shape=None):
    """The uint8 pictures PIL.Image.resize(sizes[k], filter) makes of `images`, as views of ONE device buffer from one
    launch: images, orientations, flatten and layout as resize_images / orient_images / flatten_images take them; sizes
    one (w, h) or one per picture, in the STORED orientation, each side 1..65535 -- larger than the source too; filter
    one Filter or one per picture.  source_box=(l, t, r, b) in doubles, in the stored picture's samples, and
    reducing_gap= (None, or 1.0 and more), each one value or one per picture: the pictures of Image.resize(sizes[k],
    filter, box=, reducing_gap=).  post= (one PillowFilter or one per picture, None among them: not filtered): the made
    upright pictures through im.filter(BoxBlur | GaussianBlur | UnsharpMask), Pillow's bytes again.  compose= (one
    Compose or one per picture, None among them): the canvases with their overlays behind that.  Returns uint8 CUDA
    tensors [h_k, w_k, 3] (layout="chw": [3, h_k, w_k]; gray FloatPixels: [h_k, w_k]), rows padded to a multiple of 4 bytes."""
    import torch
    who = "resample_images"
    planes, dims, dev, fmt, fp = li._read(who, images, layout, flatten)
    orientations = sj._orientation_list(who, len(dims), orientations)
    if _shape is not None:                       # (thumbnail_images, fit_images: sizes and boxes follow from the pictures' own)
        sizes, source_box = _shape(dims)
    sizes = li._sizes(who, dims, sizes, None, orientations)
    _filter_args(who, len(dims), filter)
    _box_args(who, len(dims), source_box, reducing_gap)
    _post_args(who, len(dims), post)
    _compose_args(who, len(dims), compose, dims, sizes, orientations)
    eng = sj._engine_for(engine, dev, fp)
    with torch.cuda.device(dev):
        rfmt, made, _ = resample_ragged(eng, fmt, planes, dims, sizes, filter, orientations, flatten, source_box=source_box,
                                        reducing_gap=reducing_gap, post=post, compose=compose)
        if engine is None:
            torch.cuda.current_stream().synchronize()        # (the engine made here goes away with the call)
    return [p.permute(2, 0, 1) for p in made] if layout == "chw" and rfmt == sj.SRC_RGB else made


def encode_resampled_images(images, sizes=None, box=None, filter=Filter.LANCZOS, unsharp=None, metadata=None, packed=False, orientations=None,
                            flatten=None, quality=75.0, yuv_mode=YUV_420, method=4, use_trellis=False, target_size=None, target_psnr=None,
                            layout="hwc", engine=None, source_box=None, reducing_gap=None, post=None, compose=None, _shape=None):
    """The thumbnail call with Pillow's filters: JPEGs (list of bytes), picture k's byte for byte what encode_images_full
    makes of the picture resample_images returns for the same arguments (sharpened by `unsharp`, an unsharp.Unsharp or
    one per picture, where given).  box=(bw, bh) fits the upright picture into the box and never enlarges; sizes= is
    explicit and may enlarge.  source_box=, reducing_gap=, post= and compose= as resample_images takes them; post= or
    compose= together with unsharp= is an error.  The other arguments as unsharp.encode_unsharp_images takes them."""
    import torch
    who = "encode_resampled_images"
    planes, dims, dev, fmt, fp = li._read(who, images, layout, flatten)
    n = len(dims)
    sj._gray_mode(who, fmt, int(yuv_mode))
    orientations = sj._orientation_list(who, n, orientations)
    if _shape is not None:
        sizes, source_box = _shape(dims)
    sizes = li._sizes(who, dims, sizes, box, orientations)
    _filter_args(who, n, filter)
    _box_args(who, n, source_box, reducing_gap)
    _post_args(who, n, post, unsharp)
    _compose_args(who, n, compose, dims, sizes, orientations, unsharp)
    un._unsharp_args(who, n, unsharp)
    method = li._method(who, method, use_trellis)
    sj._one_target(who, target_size, target_psnr)
    search = sj._target_search(who, "image", n, target_size, target_psnr)
    qs = sj._per_picture(quality, n)
    if len(qs) != n:
        raise SjpegError(f"{who}: one quality per image")
    eng = sj._engine_for(engine, dev, fp)
    with torch.cuda.device(dev):
        res = encode_ragged_resampled(eng, fmt, planes, dims, sizes, orientations, int(yuv_mode), sj._quality_quant(qs), method, filter, flatten,
                                      unsharp, search, metadata, packed, source_box=source_box, reducing_gap=reducing_gap, post=post,
                                      compose=compose)
        eng.wait()                               # (pipelined mode: the output is complete after this)
        return sj._fetch_packed(res[0], res[1], res[2], n, "image") if packed else sj._fetch_ragged(res[0], res[1], res[2])


# ---- Image.thumbnail and ImageOps.fit: sizes and source boxes that follow from the pictures' own sizes

def _thumbnail_shape(box):
    """(sizes, source boxes) of Image.thumbnail(box): the whole picture said outright, so that the call goes through the
    box entries and their refusals also where nothing is reduced"""
    return lambda dims: ([thumbnail_size(w, h, box) for w, h in dims], [(0.0, 0.0, float(w), float(h)) for w, h in dims])


def _fit_shape(size, bleed, centering):
    """(sizes, source boxes) of ImageOps.fit(size, bleed=, centering=).  (left + width may leave the picture by one
    rounding of a double; Pillow's float32 box does not see that, so the crop is held inside the picture.)"""
    size = (int(size[0]), int(size[1]))
    return lambda dims: ([size] * len(dims), [tuple(min(v, float(lim)) for v, lim in zip(fit_crop(w, h, size, bleed, centering), (w, h, w, h)))
                                              for w, h in dims])


def thumbnail_images(images, box, filter=Filter.BICUBIC, reducing_gap=2.0, **kw):
    """The pictures im.thumbnail(box, filter, reducing_gap=) leaves of `images`: thumbnail_size's sizes -- the aspect
    kept, never larger than the picture --, Pillow's reduce where a side is at least 2 * reducing_gap times its target,
    then the resample.  box is in the STORED orientation.  The other arguments as resample_images takes them."""
    return resample_images(images, None, filter, reducing_gap=reducing_gap, _shape=_thumbnail_shape(box), **kw)


def encode_thumbnails(images, box, filter=Filter.BICUBIC, reducing_gap=2.0, **kw):
    """JPEGs of the pictures thumbnail_images makes, byte for byte what encode_images_full makes of them.  The other
    arguments as encode_resampled_images takes them (but sizes and box)."""
    return encode_resampled_images(images, filter=filter, reducing_gap=reducing_gap, _shape=_thumbnail_shape(box), **kw)


def fit_images(images, size, filter=Filter.BICUBIC, bleed=0.0, centering=(0.5, 0.5), **kw):
    """The pictures ImageOps.fit(im, size, filter, bleed, centering) makes of `images`: cropped to the ratio of size
    around the centering -- a fractional crop, fit_crop's -- and resized to it.  size and the crop are in the STORED
    orientation.  The other arguments as resample_images takes them."""
    return resample_images(images, None, filter, _shape=_fit_shape(size, bleed, centering), **kw)


def encode_fitted_images(images, size, filter=Filter.BICUBIC, bleed=0.0, centering=(0.5, 0.5), **kw):
    """JPEGs of the pictures fit_images makes, byte for byte what encode_images_full makes of them.  The other arguments
    as encode_resampled_images takes them (but sizes and box)."""
    return encode_resampled_images(images, filter=filter, _shape=_fit_shape(size, bleed, centering), **kw)


# ---- ImageOps.pad: contain's size, then a canvas

def _upright(d, o):
    return (d[1], d[0]) if o is not None and int(o) >= 5 else (d[0], d[1])


def _pad_shape(size, orientations):
    """(sizes, source boxes) of ImageOps.contain(size) of the UPRIGHT pictures, handed on in the stored orientation: no
    reducing gap and the whole picture, as contain calls resize"""
    def shape(dims):
        ol = sj._orientation_list("pad_images", len(dims), orientations)
        sizes = []
        for k, d in enumerate(dims):
            o = None if ol is None else ol[k]
            sizes.append(_upright(contain_size(*_upright(d, o), size), o))
        return sizes, None
    return shape


def pad_images(images, size, filter=Filter.BICUBIC, colour=(0, 0, 0), centering=(0.5, 0.5), orientations=None, overlays=(), **kw):
    """The pictures ImageOps.pad(im, size, filter, color=colour, centering=centering) makes of the UPRIGHT `images`:
    contain_size's sizes -- the aspect kept, enlarging too --, then the canvas of `size` with the picture at pad_place's
    place; overlays=[(overlay, (x, y), anchor), ...] are pasted onto it.  The other arguments as resample_images takes them."""
    return resample_images(images, None, filter, orientations=orientations, compose=Compose.pad(size, colour, centering, overlays),
                           _shape=_pad_shape(size, orientations), **kw)


def encode_padded_images(images, size, filter=Filter.BICUBIC, colour=(0, 0, 0), centering=(0.5, 0.5), orientations=None, overlays=(), **kw):
    """JPEGs of the pictures pad_images makes, byte for byte what encode_images_full makes of them.  The other arguments
    as encode_resampled_images takes them (but sizes and box)."""
    return encode_resampled_images(images, filter=filter, orientations=orientations, compose=Compose.pad(size, colour, centering, overlays),
                                   _shape=_pad_shape(size, orientations), **kw)
