"""Thumbnails sharpened inside the ragged call (sjpeg_hip.h, "unsharp mask").  An area average is a box filter, so a
thumbnail comes out soft; every thumbnailer sharpens behind its resize.  The calls here run the 3 x 3 unsharp mask --
weights [1 2 1] x [1 2 1], edge replicated, amount in 32nds, threshold in byte levels, one right answer in integers -- as
ONE more launch behind the launch that makes the pictures, on the made bytes: for RGB-like and gray pictures behind
pixel transform, flatten, light, average, inverse and turn; for video behind resize, turn and colour conversion, on Y
only.  unsharp_sample is the formula on one neighbourhood.  ("sharp" elsewhere in the package is the reference's sharp
YUV conversion.)  Contact sheets are not sharpened."""
import ctypes as C

import numpy as np

import sjpeg_amd as sj
import sjpeg_amd.light as li
import sjpeg_amd.video as vi
from sjpeg_amd import YUV_420, YUV_444, SjpegError

class _UnsharpStruct(C.Structure):
    """struct sjpeg_hip_unsharp"""
    _fields_ = [("amount", C.c_uint8), ("threshold", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class Unsharp:
    """amount 0..255 in 32nds (32: out = 2 p - blur; 0: nothing is sharpened), threshold 0..255 in byte levels: a sample
    closer than that to its blur is left alone (0: every sample is sharpened)."""

    def __init__(self, amount=32, threshold=0):
        for name, v in (("amount", amount), ("threshold", threshold)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 255:
                raise SjpegError(f"Unsharp: {name} {v!r} is not one of 0..255")
        self.amount, self.threshold = int(amount), int(threshold)

    def __eq__(self, other):
        return isinstance(other, Unsharp) and (self.amount, self.threshold) == (other.amount, other.threshold)

    def __hash__(self):
        return hash((self.amount, self.threshold))

    def __repr__(self):
        return "Unsharp(%d, %d)" % (self.amount, self.threshold)

    def _struct(self):
        return _UnsharpStruct(self.amount, self.threshold)


_lib = sj.lib                            # (the one table of sjpeg_amd._binding binds every entry when the library loads)


def _unsharp_args(who, n, unsharp):
    """(the struct array, its address, whether there is one per frame) of one Unsharp or a sequence of one per frame;
    None: the entries' NULL -- nothing is sharpened"""
    if unsharp is None:
        return None, None, 0
    if isinstance(unsharp, Unsharp):
        arr = (_UnsharpStruct * 1)(unsharp._struct())
        return arr, C.addressof(arr), 0
    try:
        us = list(unsharp)
    except TypeError:
        raise SjpegError(f"{who}: unsharp {unsharp!r} is not an Unsharp or a sequence of one per frame")
    if len(us) != n or not all(isinstance(u, Unsharp) for u in us):
        raise SjpegError(f"{who}: unsharp is one Unsharp or a sequence of one per frame ({n})")
    arr = (_UnsharpStruct * n)(*[u._struct() for u in us])
    return arr, C.addressof(arr), 1


def unsharp_sample(n, amount=32, threshold=0):
    """sjpeg_hip_unsharp_sample: the formula on single neighbourhoods, host only.  n: uint8 [..., 3, 3] (or [..., 9]),
    row above / at / below, n[..., 1, 1] the sample; returns uint8 [...]."""
    who = "unsharp_sample"
    u = Unsharp(amount, threshold)
    src = np.ascontiguousarray(n, dtype=np.uint8)
    if src.ndim >= 2 and src.shape[-2:] == (3, 3):
        src = src.reshape(src.shape[:-2] + (9,))
    if src.ndim < 1 or src.shape[-1] != 9:
        raise SjpegError(f"{who}: n is uint8 [..., 3, 3] or [..., 9]")
    flat = src.reshape(-1, 9)
    out = np.empty(flat.shape[0], np.uint8)
    L, byte = _lib(), C.c_uint32(0)
    for k in range(flat.shape[0]):
        if L.sjpeg_hip_unsharp_sample(u.amount, u.threshold, flat[k].ctypes.data, C.byref(byte)) != 0:
            raise SjpegError(f"sjpeg_hip_unsharp_sample failed: {sj.last_error()}")
        out[k] = byte.value
    return out.reshape(src.shape[:-1])


# ---- the ragged level: fmt, planes_per_frame and dims as Engine.encode_ragged takes them

def unsharp_ragged(engine, fmt, planes_per_frame, dims, sizes=None, orientations=None, flatten=None, light=li.CODED, unsharp=Unsharp(),
                   out=None):
    """sjpeg_hip_unsharp_ragged_src: light.linear_ragged (light CODED: Engine.orient_ragged / flatten_ragged) with the made
    pictures sharpened by one more launch; unsharp one Unsharp or one per frame.  Returns (fmt, pictures, buf) as they
    do.  Every frame goes through the resize kernel, at its own size too."""
    who = "unsharp_ragged"
    n = len(dims)
    if sizes is not None and len(sizes) != n:
        raise SjpegError(f"{who}: one size per frame")
    light = li._light(who, light)
    ukeep, uaddr, per_frame = _unsharp_args(who, n, unsharp)
    frames, _, _, _ = sj._ragged_frames(planes_per_frame, dims, None, None, None, None)
    arr, oarr = sj._shape_arrays(who, n, sizes, orientations)
    keep, faddr = li._flat_struct(who, flatten)
    return engine._make_pictures(who, who, "orient_ragged", fmt, planes_per_frame, frames, {"sizes": sj._address(arr), "orientations": sj._address(oarr)},
                                 {"flatten": faddr, "light": light, "unsharp": (uaddr, per_frame)}, out)


def encode_ragged_unsharp(engine, fmt, planes_per_frame, dims, sizes, orientations, yuv_mode, quant, method=4, flatten=None, light=li.CODED,
                          unsharp=Unsharp(), search=None, metadata=None, packed=False, min_quant=None, q_bias=0x78, dmax_luma=12,
                          dmax_chroma=1):
    """sjpeg_hip_encode_ragged_unsharp_src / _unsharp_packed_src: light.encode_ragged_linear with the made pictures
    sharpened.  Frame k's bytes are those Engine.encode_ragged_full makes of the uint8 picture unsharp_ragged returns.
    Returns (out, sizes, offsets, modes, q, value)."""
    who = "encode_ragged_unsharp"
    light = li._light(who, light)
    n = len(dims)
    ukeep, uaddr, per_frame = _unsharp_args(who, n, unsharp)
    call = engine._oriented_call(who, planes_per_frame, dims, sizes, orientations, yuv_mode, quant, method, min_quant, q_bias, dmax_luma,
                                 dmax_chroma, search, None, metadata)
    keep, faddr = li._flat_struct(who, flatten)
    return engine._encode_shaped(who, "unsharp", fmt, planes_per_frame, dims, call,
                                 {"flatten": faddr, "light": light, "sizes": call.sizes, "orientations": call.orientations,
                                  "unsharp": (uaddr, per_frame)}, packed)


# ---- the picture level: images as resize_images / flatten_images take them

def _light_of(who, light):
    return li.CODED if light is None or light is False else li.LINEAR_SRGB if light is True else li._light(who, light)


def unsharp_images(images, sizes=None, box=None, orientations=None, unsharp=Unsharp(), light=None, flatten=None, layout="hwc", engine=None):
    """The uint8 pictures resize_images / orient_images / flatten_images make (light=light.LINEAR_SRGB or True: those of
    light.linear_resize_images), sharpened, as views of ONE device buffer: images, sizes / box, orientations, flatten and
    layout as they take them (neither sizes nor box: the pictures' own sizes -- "sharpen only"); unsharp one Unsharp or
    one per picture.  Returns uint8 CUDA tensors [h_k, w_k, 3] (layout="chw": [3, h_k, w_k]; gray FloatPixels:
    [h_k, w_k]), rows padded to a multiple of 4 bytes."""
    import torch
    who = "unsharp_images"
    light = _light_of(who, light)
    planes, dims, dev, fmt, fp = li._read(who, images, layout, flatten)
    orientations = sj._orientation_list(who, len(dims), orientations)
    sizes = li._sizes(who, dims, sizes, box, orientations)
    _unsharp_args(who, len(dims), unsharp)
    eng = sj._engine_for(engine, dev, fp)
    with torch.cuda.device(dev):
        rfmt, made, _ = unsharp_ragged(eng, fmt, planes, dims, sizes, orientations, flatten, light, unsharp)
        if engine is None:
            torch.cuda.current_stream().synchronize()        # (the engine made here goes away with the call)
    return [p.permute(2, 0, 1) for p in made] if layout == "chw" and rfmt == sj.SRC_RGB else made


def encode_unsharp_images(images, sizes=None, box=None, orientations=None, unsharp=Unsharp(), light=None, flatten=None, quality=75.0,
                          yuv_mode=YUV_420, method=4, use_trellis=False, target_size=None, target_psnr=None, packed=False, metadata=None,
                          layout="hwc", engine=None):
    """The thumbnail call with sharpening: JPEGs (list of bytes), picture k's byte for byte what encode_images_full makes
    of the picture unsharp_images returns for the same arguments.  The other arguments as light.encode_linear_images
    takes them."""
    import torch
    who = "encode_unsharp_images"
    light = _light_of(who, light)
    planes, dims, dev, fmt, fp = li._read(who, images, layout, flatten)
    n = len(dims)
    sj._gray_mode(who, fmt, int(yuv_mode))
    orientations = sj._orientation_list(who, n, orientations)
    sizes = li._sizes(who, dims, sizes, box, orientations)
    _unsharp_args(who, n, unsharp)
    method = li._method(who, method, use_trellis)
    sj._one_target(who, target_size, target_psnr)
    search = sj._target_search(who, "image", n, target_size, target_psnr)
    qs = sj._per_picture(quality, n)
    if len(qs) != n:
        raise SjpegError(f"{who}: one quality per image")
    eng = sj._engine_for(engine, dev, fp)
    with torch.cuda.device(dev):
        res = encode_ragged_unsharp(eng, fmt, planes, dims, sizes, orientations, int(yuv_mode), sj._quality_quant(qs), method, flatten, light,
                                    unsharp, search, metadata, packed)
        eng.wait()                               # (pipelined mode: the output is complete after this)
        return sj._fetch_packed(res[0], res[1], res[2], n, "image") if packed else sj._fetch_ragged(res[0], res[1], res[2])


# ---- decoded video: frames, fmt, colour and depth as sjpeg_amd.video takes them; Y alone is sharpened

def unsharp_video_frames(frames, fmt=sj.SRC_NV12, colour=vi.VideoColour(), sizes=None, box=None, orientations=None, unsharp=Unsharp(),
                         depth=None, engine=None, out=None):
    """sjpeg_hip_unsharp_ragged_yuv_src: the planes video.convert_yuv_frames (depth, a VideoDepth: convert_deep_frames)
    makes, Y sharpened by one more launch, U and V as they were.  Returns (out_fmt, pictures, buf) as they do."""
    import torch
    who = "unsharp_video_frames"
    planes, dims, dev, dkeep, deep = vi._read_frames(who, frames, fmt, depth)
    n = len(dims)
    orientations = sj._orientation_list(who, n, orientations)
    sizes = vi._size_list(who, n, dims, sizes, box, orientations)
    if sizes is not None and len(sizes) != n:
        raise SjpegError(f"{who}: one size per frame")
    keep, caddr, cper = vi._colour_args(who, n, colour)
    ukeep, uaddr, uper = _unsharp_args(who, n, unsharp)
    eng = sj._engine_for(engine, dev)
    with torch.cuda.device(dev):
        cframes, _, _, _ = sj._ragged_frames(planes, dims, None, None, None, None)
        arr, oarr = sj._shape_arrays(who, n, sizes, orientations)
        return eng._make_pictures(who, "unsharp_ragged_yuv", "resize_ragged_yuv", fmt, planes, cframes,
                                  {"sizes": sj._address(arr), "orientations": sj._address(oarr)},
                                  {"colour": (caddr, cper), "depth": deep.get("depth"), "unsharp": (uaddr, uper)}, out)


def encode_unsharp_video_frames(frames, fmt=sj.SRC_NV12, colour=vi.VideoColour(), sizes=None, box=None, orientations=None, unsharp=Unsharp(),
                                depth=None, quality=75.0, method=4, target_size=None, target_psnr=None, packed=False, metadata=None,
                                engine=None):
    """The thumbnail call for decoded video with sharpening: video.encode_video_frames (depth, a VideoDepth:
    encode_deep_video_frames) plus unsharp, one Unsharp or one per frame.  Frame k's JPEG is byte for byte what
    encode_yuv_frames makes of the planes unsharp_video_frames returns.  Returns the JPEGs (list of bytes)."""
    import torch
    who = "encode_unsharp_video_frames"
    planes, dims, dev, dkeep, deep = vi._read_frames(who, frames, fmt, depth)
    n = len(dims)
    orientations = sj._orientation_list(who, n, orientations)
    sizes = vi._size_list(who, n, dims, sizes, box, orientations)
    keep, caddr, cper = vi._colour_args(who, n, colour)
    ukeep, uaddr, uper = _unsharp_args(who, n, unsharp)
    sj._one_target(who, target_size, target_psnr)
    search = sj._target_search(who, "frame", n, target_size, target_psnr)
    qs = sj._per_picture(quality, n)
    if len(qs) != n:
        raise SjpegError(f"{who}: one quality per frame")
    yuv_mode = YUV_444 if fmt == sj.SRC_YUV444 else YUV_420
    eng = sj._engine_for(engine, dev)
    with torch.cuda.device(dev):
        call = eng._oriented_call(who, planes, dims, sizes, orientations, yuv_mode, sj._quality_quant(qs), method, None, 0x78, 12, 1,
                                  search, None, metadata)
        res = eng._encode_shaped(who, "yuv_unsharp", fmt, planes, dims, call,
                                 {"sizes": call.sizes, "orientations": call.orientations, "colour": (caddr, cper), "depth": deep.get("depth"),
                                  "unsharp": (uaddr, uper)}, packed)
        eng.wait()                               # (pipelined mode: the output is complete after this)
        return sj._fetch_packed(res[0], res[1], res[2], n, "frame") if packed else sj._fetch_ragged(res[0], res[1], res[2])
