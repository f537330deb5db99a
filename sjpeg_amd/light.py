"""Resize in linear light inside the ragged call (sjpeg_hip.h, "resize in linear light").  A downscaler that averages
gamma-encoded bytes darkens fine detail: a 0/255 checkerboard halved comes out as 128 where the light it emitted is byte
188.  resize_images, Resized, Oriented, Flattened and the sheets average the stored bytes; the calls here average the
LIGHT the bytes stand for -- every byte through the sRGB table L[] (light_table()), the exact area average of the
16-bit values, and the exact inverse back to the byte whose light is nearest -- still in the resize kernel's ONE launch
and still with one right answer in integers.  The order is: pixel transform (FloatPixels), flatten on bytes as ever,
L[], average, inverse, turn, place; a sheet's background is bytes as given.  A picture at its own size comes back
unchanged.  The YUV-plane formats are refused: their samples are not RGB light."""
import ctypes as C

import numpy as np

import sjpeg_amd as sj
from sjpeg_amd import YUV_420, YUV_AUTO, SjpegError, lib

CODED, LINEAR_SRGB = 0, 1                # SJPEG_HIP_LIGHT_*

_lib = lib                               # (the one table of sjpeg_amd._binding binds every entry when the library loads)


def _light(who, light):
    if isinstance(light, bool) or not isinstance(light, int) or light not in (CODED, LINEAR_SRGB):
        raise SjpegError(f"{who}: light {light!r} is not CODED (0) or LINEAR_SRGB (1)")
    return light


def light_table(light=LINEAR_SRGB):
    """sjpeg_hip_light_table: the 256 uint16 values L[b] = floor(65535 f(b / 255) + 1/2), f the sRGB decoding function of
    IEC 61966-2-1 (CODED: the bytes themselves).  Host only."""
    out = np.zeros(256, np.uint16)
    if _lib().sjpeg_hip_light_table(_light("light_table", light), out.ctypes.data) != 0:
        raise SjpegError(f"sjpeg_hip_light_table failed: {sj.last_error()}")
    return out


def light_round(S, W, H, light=LINEAR_SRGB):
    """sjpeg_hip_light_round: the byte a cell of sum S of a W x H picture becomes -- the number of k in 1..255 with
    2 S >= (L[k-1] + L[k]) W H: the byte whose light is nearest the exact average, a tie to the larger.  Host only."""
    out = C.c_uint32(0)
    if _lib().sjpeg_hip_light_round(_light("light_round", light), int(S), int(W), int(H), C.byref(out)) != 0:
        raise SjpegError(f"sjpeg_hip_light_round failed: {sj.last_error()}")
    return int(out.value)


def _flat_struct(who, flatten):
    """(the struct sjpeg_hip_flatten or None, its address or None) of a call's flatten=: None or a sjpeg_amd.Flatten"""
    if flatten is None:
        return None, None
    st = sj._flatten_struct(who, flatten)
    return st, C.addressof(st)


# ---- the ragged level: fmt, planes_per_frame and dims as Engine.encode_ragged takes them -- any format the resize reads

def linear_ragged(engine, fmt, planes_per_frame, dims, sizes=None, orientations=None, flatten=None, light=LINEAR_SRGB, out=None):
    """sjpeg_hip_linear_ragged_src: Engine.orient_ragged (flatten, a sjpeg_amd.Flatten: Engine.flatten_ragged) in linear
    light.  Returns (fmt, pictures, buf) as they do.  Every frame goes through the kernel, at its own size too."""
    who = "linear_ragged"
    n = len(dims)
    if sizes is not None and len(sizes) != n:
        raise SjpegError(f"{who}: one size per frame")
    light = _light(who, light)
    frames, _, _, _ = sj._ragged_frames(planes_per_frame, dims, None, None, None, None)
    arr, oarr = sj._shape_arrays(who, n, sizes, orientations)
    keep, faddr = _flat_struct(who, flatten)
    # (a flattened picture has the bytes of the same call on SRC_RGB frames)
    return engine._make_pictures(who, who, "orient_ragged", fmt, planes_per_frame, frames, {"sizes": sj._address(arr), "orientations": sj._address(oarr)},
                                 {"flatten": faddr, "light": light}, out)


def encode_ragged_linear(engine, fmt, planes_per_frame, dims, sizes, orientations, yuv_mode, quant, method=4, flatten=None,
                         light=LINEAR_SRGB, search=None, metadata=None, packed=False, min_quant=None, q_bias=0x78, dmax_luma=12,
                         dmax_chroma=1):
    """sjpeg_hip_encode_ragged_linear_src / _linear_packed_src: Engine.encode_ragged_flattened (packed: its packed twin)
    in linear light.  Frame k's bytes are those Engine.encode_ragged_full makes of the uint8 picture linear_ragged
    returns.  Returns (out, sizes, offsets, modes, q, value)."""
    who = "encode_ragged_linear"
    light = _light(who, light)
    call = engine._oriented_call(who, planes_per_frame, dims, sizes, orientations, yuv_mode, quant, method, min_quant, q_bias, dmax_luma,
                                 dmax_chroma, search, None, metadata)
    keep, faddr = _flat_struct(who, flatten)
    return engine._encode_shaped(who, "linear", fmt, planes_per_frame, dims, call,
                                 {"flatten": faddr, "light": light, "sizes": call.sizes, "orientations": call.orientations}, packed)


def sheet_ragged_linear(engine, fmt, planes_per_frame, dims, sheet, sizes=None, orientations=None, flatten=None, light=LINEAR_SRGB,
                        out=None):
    """sjpeg_hip_sheet_ragged_linear_src: Engine.sheet_ragged with the thumbnails averaged in linear light; the sheet's
    background is bytes as given.  Returns (out_fmt, sheets, buf)."""
    who = "sheet_ragged_linear"
    n = len(dims)
    if sizes is not None and len(sizes) != n:
        raise SjpegError(f"{who}: one size per frame")
    light = _light(who, light)
    frames, _, _, _ = sj._ragged_frames(planes_per_frame, dims, None, None, None, None)
    shape, nsheets, skeep = sj._sheet_shape(who, n, sheet, sizes, orientations)
    keep, faddr = _flat_struct(who, flatten)
    return engine._make_pictures(who, who, "sheet_ragged", fmt, planes_per_frame, frames, shape, {"flatten": faddr, "light": light}, out, nsheets)


def encode_ragged_sheet_linear(engine, fmt, planes_per_frame, dims, sheet, sizes, orientations, yuv_mode, quant, method=4, flatten=None,
                               light=LINEAR_SRGB, search=None, metadata=None, packed=False):
    """sjpeg_hip_encode_ragged_sheet_linear_src / _sheet_linear_packed_src: Engine.encode_ragged_sheet (packed: its packed
    twin) of the sheets sheet_ragged_linear makes.  Returns (out, sizes, offsets, modes, q, value), one entry per sheet."""
    who = "encode_ragged_sheet_linear"
    light = _light(who, light)
    ns, call, segments = engine._sheet_call(who, fmt, planes_per_frame, dims, sheet, sizes, orientations, yuv_mode, quant, int(method), None,
                                            0x78, 12, 1, search, metadata)
    keep, faddr = _flat_struct(who, flatten)
    return engine._encode_sheets_shaped(who, "sheet_linear", fmt, planes_per_frame, dims, ns, call, dict(segments, flatten=faddr, light=light), packed)


# ---- the picture level: images as resize_images / flatten_images / make_sheets take them

def _read(who, images, layout, flatten):
    """(planes, dims, device, format, FloatPixels or None) of a call's pictures: those of make_sheets -- layout="hwc": CUDA
    uint8 tensors [H, W, 3]; "chw": channel-first uint8 tensors or a FloatPixels; with a flatten [H, W, 4] RGBA, uint8 or a
    FloatPixels"""
    if flatten is not None and not isinstance(flatten, sj.Flatten):
        raise SjpegError(f"{who}: flatten is not a Flatten")
    return sj._sheet_pictures(who, images, layout, flatten)


def _sizes(who, dims, sizes, box, orientations):
    """sizes (one (w, h) or one per picture), or the pictures fitted into box (the UPRIGHT one), or None: their own"""
    n = len(dims)
    if sizes is not None and box is not None:
        raise SjpegError(f"{who}: give sizes or box, not both")
    if box is not None:
        try:
            bw, bh = box
        except (TypeError, ValueError):
            raise SjpegError(f"{who}: box {box!r} is not a pair (width, height)")
        return [sj.fit_size(w, h, (bh, bw) if orientations is not None and orientations[k] >= 5 else (bw, bh)) for k, (w, h) in enumerate(dims)]
    if sizes is None:
        return None
    sizes = list(sizes)
    if len(sizes) == 2 and not isinstance(sizes[0], (tuple, list, np.ndarray)):
        sizes = [tuple(sizes)] * n
    if len(sizes) != n:
        raise SjpegError(f"{who}: one size per picture")
    return [(int(w), int(h)) for w, h in sizes]


def _method(who, method, use_trellis):
    method = int(method)
    if method < 0 or method > 8:
        raise SjpegError(f"{who}: method {method} is not one of 0..8")
    return {4: 7, 6: 8}.get(method, method) if use_trellis else method


def linear_resize_images(images, sizes=None, box=None, orientations=None, flatten=None, layout="hwc", engine=None):
    """The uint8 pictures resize_images / orient_images / flatten_images make, averaged in LINEAR light, as views of ONE
    device buffer from one launch: images as they take them (flatten, a sjpeg_amd.Flatten: [H, W, 4] RGBA pictures laid
    over its background first, on bytes), sizes one (w, h) or one per picture in the STORED orientation or box (bw, bh)
    to fit the upright picture into (neither: the pictures' own sizes, which come back unchanged), orientations one EXIF
    value 1..8 or one per picture.  Returns uint8 CUDA tensors [h_k, w_k, 3] (layout="chw": [3, h_k, w_k]; gray
    FloatPixels: [h_k, w_k]), rows padded to a multiple of 4 bytes."""
    import torch
    who = "linear_resize_images"
    planes, dims, dev, fmt, fp = _read(who, images, layout, flatten)
    orientations = sj._orientation_list(who, len(dims), orientations)
    sizes = _sizes(who, dims, sizes, box, orientations)
    eng = sj._engine_for(engine, dev, fp)
    with torch.cuda.device(dev):
        rfmt, made, _ = linear_ragged(eng, fmt, planes, dims, sizes, orientations, flatten)
        if engine is None:
            torch.cuda.current_stream().synchronize()        # (the engine made here goes away with the call)
    return [p.permute(2, 0, 1) for p in made] if layout == "chw" and rfmt == sj.SRC_RGB else made


def encode_linear_images(images, sizes=None, box=None, orientations=None, flatten=None, quality=75.0, yuv_mode=YUV_420, method=4,
                         use_trellis=False, target_size=None, target_psnr=None, packed=False, metadata=None, layout="hwc", engine=None):
    """The thumbnail call in linear light: JPEGs (list of bytes), picture k's byte for byte what encode_images_full makes
    of the picture linear_resize_images returns for the same arguments.  quality, target_size / target_psnr and metadata:
    one for all or one per picture; yuv_mode any SjpegYUVMode (YUV_AUTO decides on the made picture; gray FloatPixels:
    YUV_400); use_trellis maps method 4 to 7 and 6 to 8; packed=True: through the packed entry and one device-to-host
    copy."""
    import torch
    who = "encode_linear_images"
    planes, dims, dev, fmt, fp = _read(who, images, layout, flatten)
    n = len(dims)
    sj._gray_mode(who, fmt, int(yuv_mode))
    orientations = sj._orientation_list(who, n, orientations)
    sizes = _sizes(who, dims, sizes, box, orientations)
    method = _method(who, method, use_trellis)
    sj._one_target(who, target_size, target_psnr)
    search = sj._target_search(who, "image", n, target_size, target_psnr)
    qs = sj._per_picture(quality, n)
    if len(qs) != n:
        raise SjpegError(f"{who}: one quality per image")
    eng = sj._engine_for(engine, dev, fp)
    with torch.cuda.device(dev):
        res = encode_ragged_linear(eng, fmt, planes, dims, sizes, orientations, int(yuv_mode), sj._quality_quant(qs), method, flatten,
                                   LINEAR_SRGB, search, metadata, packed)
        eng.wait()                               # (pipelined mode: the output is complete after this)
        return sj._fetch_packed(res[0], res[1], res[2], n, "image") if packed else sj._fetch_ragged(res[0], res[1], res[2])


def make_linear_sheets(images, sheet, sizes=None, orientations=None, flatten=None, layout="hwc", engine=None):
    """make_sheets with the thumbnails averaged in linear light (flatten: None or a sjpeg_amd.Flatten); the sheet's
    background and gutters are bytes as given.  Returns the sheets as make_sheets does."""
    import torch
    who = "make_linear_sheets"
    planes, dims, dev, fmt, fp = _read(who, images, layout, flatten)
    eng = sj._engine_for(engine, dev, fp)
    with torch.cuda.device(dev):
        _, sheets, _ = sheet_ragged_linear(eng, fmt, planes, dims, sheet, sizes, sj._orientation_list(who, len(dims), orientations), flatten)
        if engine is None:
            torch.cuda.current_stream().synchronize()        # (the engine made here goes away with the call)
    return sheets


def encode_linear_sheets(images, sheet, sizes=None, orientations=None, flatten=None, quality=75.0, yuv_mode=YUV_AUTO, method=4,
                         use_trellis=False, target_size=None, target_psnr=None, packed=False, metadata=None, layout="hwc", engine=None):
    """encode_sheets in linear light: (JPEGs, places) -- the JPEGs of the sheets make_linear_sheets makes of the same
    pictures, each byte for byte what encode_images_full makes of that sheet, and places[k] = (sheet, x, y, w, h)."""
    import torch
    who = "encode_linear_sheets"
    planes, dims, dev, fmt, fp = _read(who, images, layout, flatten)
    sj._gray_mode(who, fmt, int(yuv_mode))
    orientations = sj._orientation_list(who, len(dims), orientations)
    places = sj.sheet_places(sheet, dims, fmt, sizes, orientations)
    ns = places[-1][0] + 1
    method = _method(who, method, use_trellis)
    qs = sj._per_picture(quality, ns)
    if len(qs) != ns:
        raise SjpegError(f"{who}: one quality per sheet")
    sj._one_target(who, target_size, target_psnr)
    search = sj._target_search(who, "sheet", ns, target_size, target_psnr)
    eng = sj._engine_for(engine, dev, fp)
    with torch.cuda.device(dev):
        res = encode_ragged_sheet_linear(eng, fmt, planes, dims, sheet, sizes, orientations, int(yuv_mode), sj._quality_quant(qs), method,
                                         flatten, LINEAR_SRGB, search, metadata, packed)
        eng.wait()                               # (pipelined mode: the output is complete after this)
        jpegs = sj._fetch_packed(res[0], res[1], res[2], ns, "sheet") if packed else sj._fetch_ragged(res[0], res[1], res[2])
    return jpegs, places
