"""Pictures resampled with Pillow's filters inside the ragged call (sjpeg_hip.h, "resampling with Pillow's filters").
Every other shape entry makes its picture with the exact area average: it only shrinks, it is soft, and it is this
library's own answer.  The calls here make the bytes PIL.Image.resize(size, LANCZOS | BICUBIC | BILINEAR | HAMMING |
BOX) of Pillow 12.2.0 makes of a picture of bytes -- along x, then along y, with a uint8 intermediate, integers only
given the tables -- in ONE launch over the batch, to sizes smaller or larger than the source on either axis.  The
tables are built on the host (resample_table shows one) and uploaded once per (filter, in, out) of a call.  Order of
steps: pixel transform, flatten, resample, turn, unsharp.  sizes are in the STORED orientation: the upright picture is
turn(resample(stored)) -- NOT exif_transpose followed by resize, which rounds its intermediate along the other axis.
There is no linear light and there are no contact sheets here; the YUV-plane formats are refused."""
import ctypes as C
import enum

import numpy as np

import sjpeg_amd as sj
import sjpeg_amd.light as li
import sjpeg_amd.unsharp as un
from sjpeg_amd import YUV_420, RaggedFrame, SjpegError

_bound = False

KSIZE_MAX = 385          # an axis whose window is longer is refused (Lanczos shrinking by more than 64, box by more than 384)


class Filter(enum.IntEnum):
    """SJPEG_HIP_RESAMPLE_*: Pillow's Image.BOX, BILINEAR, HAMMING, BICUBIC and LANCZOS"""
    BOX = 0
    BILINEAR = 1
    HAMMING = 2
    BICUBIC = 3
    LANCZOS = 4


class _ResampleStruct(C.Structure):
    """struct sjpeg_hip_resample"""
    _fields_ = [("filter", C.c_uint8), ("reserved", C.c_uint8 * 3)]


def _lib():
    """the library with the argument types of the entries this module binds: the unsharp ones without `light`, plus
    (resample, resample_per_frame) in front of the unsharp"""
    global _bound
    L = un._lib()
    if _bound:
        return L
    L.sjpeg_hip_resample_ksize.restype = C.c_int
    L.sjpeg_hip_resample_ksize.argtypes = [C.c_int, C.c_int, C.c_int]
    L.sjpeg_hip_resample_table.restype = C.c_int
    L.sjpeg_hip_resample_table.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    L.sjpeg_hip_resample_ragged_bytes.restype = C.c_size_t
    L.sjpeg_hip_resample_ragged_bytes.argtypes = list(L.sjpeg_hip_orient_ragged_bytes.argtypes)
    two = [C.c_void_p, C.c_int]
    # (..., flatten, light, sizes, orientations, unsharp, unsharp_per_frame, ...): light goes, resample comes
    for older, mine, at in (("unsharp_ragged", "resample_ragged", 5), ("encode_ragged_unsharp", "encode_ragged_resampled", 6),
                            ("encode_ragged_unsharp_packed", "encode_ragged_resampled_packed", 6)):
        plain = list(getattr(L, f"sjpeg_hip_{older}_src").argtypes)
        fn = getattr(L, f"sjpeg_hip_{mine}_src")
        fn.restype, fn.argtypes = C.c_int, plain[:at] + plain[at + 1:at + 3] + two + plain[at + 3:]
    _bound = True
    return L


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


# ---- the ragged level: fmt, planes_per_frame and dims as Engine.encode_ragged takes them

def resample_ragged(engine, fmt, planes_per_frame, dims, sizes=None, filter=Filter.LANCZOS, orientations=None, flatten=None, unsharp=None,
                    out=None):
    """sjpeg_hip_resample_ragged_src: the pictures of a ragged batch resampled to sizes[k] = (w, h) (None: their own; the
    STORED orientation; larger or smaller than the source) with `filter` (one Filter or one per frame), turned upright
    and optionally sharpened.  Returns (fmt, pictures, buf) as Engine.orient_ragged does."""
    who = "resample_ragged"
    n = len(dims)
    if sizes is not None and len(sizes) != n:
        raise SjpegError(f"{who}: one size per frame")
    L = _lib()
    rkeep, raddr, rper = _filter_args(who, n, filter)
    ukeep, uaddr, uper = un._unsharp_args(who, n, unsharp)
    frames, _, _, _ = sj._ragged_frames(planes_per_frame, dims, None, None, None, None)
    arr, oarr = sj._shape_arrays(who, n, sizes, orientations)
    keep, faddr = li._flat_struct(who, flatten)
    # (a batch the library refuses has need == 0: the call below says why)
    need = L.sjpeg_hip_resample_ragged_bytes(fmt, n, frames, sj._address(arr), sj._address(oarr))
    out = sj._made_out(who, planes_per_frame, need, out)
    made, rfmt = (RaggedFrame * n)(), C.c_int(-1)
    engine._chk(L.sjpeg_hip_resample_ragged_src(engine._h, fmt, n, frames, faddr, sj._address(arr), sj._address(oarr), raddr, rper, uaddr, uper,
                                                out.data_ptr(), int(out.numel()) if need else 0, made, C.byref(rfmt), engine._stream()),
                "sjpeg_hip_resample_ragged_src")
    return int(rfmt.value), sj._frame_views(out, made, rfmt.value), out


def encode_ragged_resampled(engine, fmt, planes_per_frame, dims, sizes, orientations, yuv_mode, quant, method=4, filter=Filter.LANCZOS,
                            flatten=None, unsharp=None, search=None, metadata=None, packed=False, min_quant=None, q_bias=0x78, dmax_luma=12,
                            dmax_chroma=1):
    """sjpeg_hip_encode_ragged_resampled_src / _resampled_packed_src.  Frame k's bytes are those Engine.encode_ragged_full
    makes of the uint8 picture resample_ragged returns.  Returns (out, sizes, offsets, modes, q, value)."""
    who = "encode_ragged_resampled"
    _lib()
    n = len(dims)
    rkeep, raddr, rper = _filter_args(who, n, filter)
    ukeep, uaddr, uper = un._unsharp_args(who, n, unsharp)
    call = engine._oriented_call(who, planes_per_frame, dims, sizes, orientations, yuv_mode, quant, method, min_quant, q_bias, dmax_luma,
                                 dmax_chroma, search, None, metadata)
    keep, faddr = li._flat_struct(who, flatten)
    special = (faddr, call.sizes, call.orientations, raddr, rper, uaddr, uper)
    if packed:
        out, packed_capacity, meta = sj._packed_out(who, n, planes_per_frame, call.capacities, None, None)
        return sj._split_meta(n, *engine._packed("sjpeg_hip_encode_ragged_resampled_packed_src", fmt, planes_per_frame, dims, call, special, out,
                                                 packed_capacity, meta))
    frames, out, sizes_out, offsets = sj._ragged_frames(planes_per_frame, dims, call.capacities, None, None, None)
    return engine._unpacked("sjpeg_hip_encode_ragged_resampled_src", fmt, frames, call, special, out, sizes_out, offsets)


# ---- the picture level: images as resize_images / flatten_images take them

def resample_images(images, sizes, filter=Filter.LANCZOS, orientations=None, flatten=None, engine=None, layout="hwc"):
    """The uint8 pictures PIL.Image.resize(sizes[k], filter) makes of `images`, as views of ONE device buffer from one
    launch: images, orientations, flatten and layout as resize_images / orient_images / flatten_images take them; sizes
    one (w, h) or one per picture, in the STORED orientation, each side 1..65535 -- larger than the source too; filter
    one Filter or one per picture.  Returns uint8 CUDA tensors [h_k, w_k, 3] (layout="chw": [3, h_k, w_k]; gray
    FloatPixels: [h_k, w_k]), rows padded to a multiple of 4 bytes."""
    import torch
    who = "resample_images"
    planes, dims, dev, fmt, fp = li._read(who, images, layout, flatten)
    orientations = sj._orientation_list(who, len(dims), orientations)
    sizes = li._sizes(who, dims, sizes, None, orientations)
    _filter_args(who, len(dims), filter)
    eng = sj._engine_for(engine, dev, fp)
    with torch.cuda.device(dev):
        rfmt, made, _ = resample_ragged(eng, fmt, planes, dims, sizes, filter, orientations, flatten)
        if engine is None:
            torch.cuda.current_stream().synchronize()        # (the engine made here goes away with the call)
    return [p.permute(2, 0, 1) for p in made] if layout == "chw" and rfmt == sj.SRC_RGB else made


def encode_resampled_images(images, sizes=None, box=None, filter=Filter.LANCZOS, unsharp=None, metadata=None, packed=False, orientations=None,
                            flatten=None, quality=75.0, yuv_mode=YUV_420, method=4, use_trellis=False, target_size=None, target_psnr=None,
                            layout="hwc", engine=None):
    """The thumbnail call with Pillow's filters: JPEGs (list of bytes), picture k's byte for byte what encode_images_full
    makes of the picture resample_images returns for the same arguments (sharpened by `unsharp`, an unsharp.Unsharp or
    one per picture, where given).  box=(bw, bh) fits the upright picture into the box and never enlarges; sizes= is
    explicit and may enlarge.  The other arguments as unsharp.encode_unsharp_images takes them."""
    import torch
    who = "encode_resampled_images"
    planes, dims, dev, fmt, fp = li._read(who, images, layout, flatten)
    n = len(dims)
    sj._gray_mode(who, fmt, int(yuv_mode))
    orientations = sj._orientation_list(who, n, orientations)
    sizes = li._sizes(who, dims, sizes, box, orientations)
    _filter_args(who, n, filter)
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
                                      unsharp, search, metadata, packed)
        eng.wait()                               # (pipelined mode: the output is complete after this)
        return sj._fetch_packed(res[0], res[1], res[2], n, "image") if packed else sj._fetch_ragged(res[0], res[1], res[2])
