"""Records what the Python binding answers to calls that break one of its argument rules -- the exception's class and
full text, or "ok" -- and the signature of every public name, in tests/golden/python_messages.json.  No GPU is needed:
the pictures are CPU tensors of a subclass that says is_cuda (as tests/test_float_layouts_host.py makes them), and every
case ends before an Engine is made.  To hold that, sjpeg_amd.Engine is replaced by a guard while the cases of the public
calls run: a case that gets as far as making an engine is recorded as "ReachedEngine", which pins that no check before
that point refused it.  The Engine methods' own length checks are reached with Engine.__new__ and a null handle and
stop before the first library call that would read it -- and before the first look at the current device, which a machine
without a GPU answers differently.

tests/test_python_messages_host.py replays the same table (cases() and signatures() below) on the current binding and
wants the same answers, byte for byte.

The file is made with the binding of the commit BEFORE a change to it, never with the change itself: copy this script
into a checkout of the parent commit and run it there,

    python tests/golden/make_python_messages.py
"""
import ctypes as C
import hashlib
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import sjpeg_amd as sj  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "python_messages.json")


class _Cuda(torch.Tensor):
    is_cuda = True


class _Cuda1(_Cuda):
    """... and one that says it lives on a second device"""
    @property
    def device(self):
        return torch.device("cuda", 1)


def fake(t):
    return t.as_subclass(_Cuda)


def fake1(t):
    return t.as_subclass(_Cuda1)


class ReachedEngine(Exception):
    pass


class _GuardEngine:
    def __init__(self, *a, **k):
        raise ReachedEngine("the call went on to make an Engine")


U8 = torch.uint8


def hwc(h=4, w=5, c=3, dtype=U8):
    return fake(torch.zeros((h, w, c), dtype=dtype))


def chw(h=4, w=5, c=3, dtype=U8):
    return fake(torch.zeros((c, h, w), dtype=dtype))


def good(layout, dtype=U8):
    return hwc(dtype=dtype) if layout == "hwc" else chw(dtype=dtype)


SHEET = sj.Sheet(2, 2, (8, 8))
META = sj.PictureMetadata(exif=b"Exif\0\0II*\0")

# public call -> (the layouts it takes, f(images, layout, **keywords))
CALLS = {
    "encode_images": (("hwc", "chw"), lambda im, layout, **k: sj.encode_images(im, layout=layout, **k)),
    "encode_images_full": (("hwc",), lambda im, layout, **k: sj.encode_images_full(im, **k)),
    "encode_images_full_chw": (("chw",), lambda im, layout, **k: sj.encode_images_full_chw(im, **k)),
    "encode_images_full_meta": (("hwc", "chw"), lambda im, layout, metadata=None, **k:
                                sj.encode_images_full_meta(im, metadata, layout=layout, **k)),
    "compress_images": (("hwc", "chw"), lambda im, layout, **k: sj.compress_images(im, layout=layout, **k)),
    "riskiness_images": (("hwc", "chw"), lambda im, layout, **k: sj.riskiness_images(im, layout=layout, **k)),
    "reduce_images": (("hwc", "chw"), lambda im, layout, factor=2, **k: sj.reduce_images(im, factor, layout=layout, **k)),
    "resize_images": (("hwc", "chw"), lambda im, layout, sizes=(2, 2), **k: sj.resize_images(im, sizes, layout=layout, **k)),
    "orient_images": (("hwc", "chw"), lambda im, layout, orientations=6, **k:
                      sj.orient_images(im, orientations, layout=layout, **k)),
    "flatten_images": (("hwc", "chw"), lambda im, layout, **k: sj.flatten_images(im, layout=layout, **k)),
    "make_sheets": (("hwc", "chw"), lambda im, layout, sheet=SHEET, **k: sj.make_sheets(im, sheet, layout=layout, **k)),
    "encode_sheets": (("hwc", "chw"), lambda im, layout, sheet=SHEET, **k: sj.encode_sheets(im, sheet, layout=layout, **k)),
}
ENCODES = ("encode_images", "encode_images_full", "encode_images_full_chw", "encode_images_full_meta", "compress_images")
WRAPPERS = {
    "Reduced": lambda im: sj.Reduced(im, 2),
    "Resized": lambda im: sj.Resized(im, (2, 2)),
    "Oriented": lambda im: sj.Oriented(im, 6),
    "Flattened": lambda im: sj.Flattened(im),
}


def picture_faults(layout):
    """(name, images): every way the pictures of a call with this layout break a rule"""
    g = lambda: good(layout)
    cpu = torch.zeros((4, 5, 3) if layout == "hwc" else (3, 4, 5), dtype=U8)
    yield "empty", []
    yield "numpy", [np.zeros(tuple(cpu.shape), np.uint8)]
    yield "cpu_tensor", [cpu]
    yield "second_cpu_tensor", [g(), cpu]
    yield "int16", [good(layout, torch.int16)]
    yield "float32_bare", [good(layout, torch.float32)]
    yield "second_int16", [g(), good(layout, torch.int16)]
    yield "rank2", [fake(torch.zeros((4, 5), dtype=U8))]
    yield "rank4", [fake(torch.zeros((1, 4, 5, 3), dtype=U8))]
    yield "two_channels", [hwc(c=2) if layout == "hwc" else chw(c=2)]
    yield "four_channels", [hwc(c=4) if layout == "hwc" else chw(c=4)]
    yield "other_layout", [good("chw" if layout == "hwc" else "hwc")]
    if layout == "hwc":
        yield "strides_x", [fake(torch.zeros((4, 5, 6), dtype=U8)[:, :, ::2])]
        yield "strides_pixel", [fake(torch.zeros((4, 10, 3), dtype=U8)[:, ::2])]
        yield "second_strides", [g(), fake(torch.zeros((5, 4, 3), dtype=U8).transpose(0, 1))]
    else:
        yield "strides_x", [fake(torch.zeros((3, 4, 10), dtype=U8)[:, :, ::2])]
        yield "second_other_kind", [g(), fake(torch.zeros((4, 5, 3), dtype=U8).permute(2, 0, 1))]
        yield "zero_width", [fake(torch.zeros((3, 4, 0), dtype=U8))]
    yield "second_device", [g(), fake1(torch.zeros(tuple(cpu.shape), dtype=U8))]
    yield "not_a_list", 5


def float_faults():
    """(name, FloatPixels) for layout="chw" """
    f32 = lambda: chw(dtype=torch.float32)
    yield "float64", sj.FloatPixels([chw(dtype=torch.float64)])
    yield "uint8", sj.FloatPixels([chw()])
    yield "two_dtypes", sj.FloatPixels([f32(), chw(dtype=torch.float16)])
    yield "two_kinds", sj.FloatPixels([f32(), fake(torch.zeros((4, 5, 3), dtype=torch.float32).permute(2, 0, 1))])
    yield "gray_then_rgb", sj.FloatPixels([fake(torch.zeros((4, 5), dtype=torch.float32)), f32()])
    yield "bad_shape", sj.FloatPixels([fake(torch.zeros((2, 4, 5), dtype=torch.float32))])
    yield "cpu_tensor", sj.FloatPixels([torch.zeros((3, 4, 5), dtype=torch.float32)])
    yield "empty", sj.FloatPixels([])
    yield "second_device", sj.FloatPixels([f32(), fake1(torch.zeros((3, 4, 5), dtype=torch.float32))])


def alpha_faults():
    """(name, pictures) of a Flattened / a flatten= call"""
    a = lambda dtype=U8: hwc(c=4, dtype=dtype)
    yield "empty", []
    yield "rgb", [hwc()]
    yield "numpy", [np.zeros((4, 5, 4), np.uint8)]
    yield "cpu_tensor", [torch.zeros((4, 5, 4), dtype=U8)]
    yield "float_bare", [a(torch.float32)]
    yield "float_u8", sj.FloatPixels([a()])
    yield "float_two_dtypes", sj.FloatPixels([a(torch.float32), a(torch.float16)])
    yield "strides", [fake(torch.zeros((4, 10, 4), dtype=U8)[:, ::2])]
    yield "rank2", [fake(torch.zeros((4, 5), dtype=U8))]
    yield "second_device", [a(), fake1(torch.zeros((4, 5, 4), dtype=U8))]


def _public_cases():
    for name, (layouts, f) in CALLS.items():
        yield f"{name}|bad_layout", lambda f=f: f([hwc()], "nhwc")
        yield f"{name}|layout_none", lambda f=f: f([hwc()], None)
        for layout in layouts:
            for fault, images in picture_faults(layout):
                yield f"{name}|{layout}|{fault}", lambda f=f, layout=layout, images=images: f(images, layout)
            yield f"{name}|{layout}|good", lambda f=f, layout=layout: f([good(layout)], layout)
            # FloatPixels: refused with "hwc"; with "chw" its own faults, and gray with a mode that is not YUV_400
            fp = sj.FloatPixels([chw(dtype=torch.float32)])
            yield f"{name}|{layout}|float_pixels", lambda f=f, layout=layout, fp=fp: f(fp, layout)
            if layout == "chw":
                for fault, fpx in float_faults():
                    yield f"{name}|chw|float|{fault}", lambda f=f, fpx=fpx: f(fpx, "chw")
                gray = sj.FloatPixels([fake(torch.zeros((4, 5), dtype=torch.float32))])
                yield f"{name}|chw|gray|default_mode", lambda f=f, gray=gray: f(gray, "chw")
                if name in ENCODES[:4] or name == "encode_sheets":
                    for mode in (sj.YUV_AUTO, sj.YUV_420, sj.YUV_SHARP, sj.YUV_444, sj.YUV_400):
                        yield f"{name}|chw|gray|mode{mode}", lambda f=f, gray=gray, mode=mode: f(gray, "chw", yuv_mode=mode)
            # every wrapper handed to the call: around a good picture, and around one that is no CUDA tensor (the calls
            # that take the wrapper go on to read its pictures)
            for wname, wrap in WRAPPERS.items():
                inner = (lambda: [hwc(c=4)]) if wname == "Flattened" else (lambda layout=layout: [good(layout)])
                bad = [torch.zeros((4, 5, 4 if wname == "Flattened" else 3), dtype=U8)]
                yield f"{name}|{layout}|{wname}|good", lambda f=f, layout=layout, wrap=wrap, inner=inner: f(wrap(inner()), layout)
                yield f"{name}|{layout}|{wname}|cpu_tensor", lambda f=f, layout=layout, wrap=wrap, bad=bad: f(wrap(bad), layout)
                yield f"{name}|{layout}|{wname}|empty", lambda f=f, layout=layout, wrap=wrap: f(wrap([]), layout)
                if wname != "Flattened":
                    yield f"{name}|{layout}|{wname}|float_pixels", \
                        lambda f=f, layout=layout, wrap=wrap: f(wrap(sj.FloatPixels([chw(dtype=torch.float32)])), layout)
            for fault, pics in alpha_faults():
                yield f"{name}|{layout}|Flattened|alpha|{fault}", lambda f=f, layout=layout, pics=pics: f(sj.Flattened(pics), layout)
    # the encodes' own keywords
    for name in ENCODES:
        layouts, f = CALLS[name]
        layout = layouts[0]
        g = lambda layout=layout: [good(layout)]
        two = lambda layout=layout: [good(layout), good(layout)]
        yield f"{name}|quality_length", lambda f=f, layout=layout, two=two: f(two(), layout, quality=[50.0])
        yield f"{name}|quality_array_length", lambda f=f, layout=layout, two=two: f(two(), layout, quality=np.array([50.0, 60.0, 70.0]))
        if name == "compress_images":
            yield f"{name}|trellis", lambda f=f, layout=layout, g=g: f(g(), layout, use_trellis=True)
            yield f"{name}|metadata_length", lambda f=f, layout=layout, g=g: f(g(), layout, metadata=[META, META])
            continue
        yield f"{name}|both_targets", lambda f=f, layout=layout, g=g: f(g(), layout, target_size=1000, target_psnr=40.0)
        yield f"{name}|target_length", lambda f=f, layout=layout, two=two: f(two(), layout, target_size=[1000])
        yield f"{name}|psnr_length", lambda f=f, layout=layout, two=two: f(two(), layout, target_psnr=[40.0, 41.0, 42.0])
        for method in (-1, 0, 6, 7, 8, 9):
            yield f"{name}|method{method}", lambda f=f, layout=layout, g=g, method=method: f(g(), layout, method=method)
            yield f"{name}|method{method}|trellis", \
                lambda f=f, layout=layout, g=g, method=method: f(g(), layout, method=method, use_trellis=True)
            yield f"{name}|method{method}|target", \
                lambda f=f, layout=layout, g=g, method=method: f(g(), layout, method=method, target_size=1000, yuv_mode=sj.YUV_420)
        for mode in (-1, 0, 2, 5):
            yield f"{name}|yuv_mode{mode}", lambda f=f, layout=layout, g=g, mode=mode: f(g(), layout, yuv_mode=mode)
            yield f"{name}|yuv_mode{mode}|target", lambda f=f, layout=layout, g=g, mode=mode: f(g(), layout, yuv_mode=mode, target_psnr=40.0)
        yield f"{name}|trellis_target", lambda f=f, layout=layout, g=g: f(g(), layout, method=4, use_trellis=True, target_size=1000,
                                                                         yuv_mode=sj.YUV_420)
        if name != "encode_images_full_chw" and layout == "hwc":
            for mode in (sj.YUV_AUTO, sj.YUV_SHARP):
                yield f"{name}|mode{mode}|not_rgb", lambda f=f, mode=mode: f([hwc(c=4)], "hwc", yuv_mode=mode, method=4)
                yield f"{name}|mode{mode}|numpy", lambda f=f, mode=mode: f([np.zeros((4, 5), np.uint8)], "hwc", yuv_mode=mode, method=4)
        if name in ("encode_images", "encode_images_full_meta"):
            yield f"{name}|metadata_length", lambda f=f, layout=layout, g=g: f(g(), layout, metadata=[META, META])
            yield f"{name}|metadata_str", lambda f=f, layout=layout, g=g: f(g(), layout, metadata="chw")
            yield f"{name}|metadata_entry", lambda f=f, layout=layout, g=g: f(g(), layout, metadata=[5])
    yield "encode_images_full_meta|unknown_keyword", lambda: sj.encode_images_full_meta([hwc()], None, colour=1)
    yield "encode_images_full_meta|engine_keyword", lambda: sj.encode_images_full_meta([hwc()], None, engine=None, packed=True)
    # the picture makers' own arguments
    for layout in ("hwc", "chw"):
        two = lambda layout=layout: [good(layout), good(layout)]
        yield f"reduce_images|{layout}|factor_length", lambda two=two, layout=layout: sj.reduce_images(two(), [2], layout=layout)
        yield f"reduce_images|{layout}|factor_9", lambda two=two, layout=layout: sj.reduce_images(two(), 9, layout=layout)
        yield f"reduce_images|{layout}|factor_float", lambda two=two, layout=layout: sj.reduce_images(two(), [1, 2.0], layout=layout)
        yield f"resize_images|{layout}|sizes_length", lambda two=two, layout=layout: sj.resize_images(two(), [(2, 2)], layout=layout)
        yield f"resize_images|{layout}|sizes_none", lambda two=two, layout=layout: sj.resize_images(two(), None, layout=layout)
        yield f"resize_images|{layout}|size_zero", lambda two=two, layout=layout: sj.resize_images(two(), [(2, 2), (0, 2)], layout=layout)
        yield f"orient_images|{layout}|orientation_length", lambda two=two, layout=layout: sj.orient_images(two(), [1], layout=layout)
        yield f"orient_images|{layout}|orientation_9", lambda two=two, layout=layout: sj.orient_images(two(), 9, layout=layout)
        yield f"orient_images|{layout}|sizes_length", lambda two=two, layout=layout: sj.orient_images(two(), 6, [(2, 2)], layout=layout)
    a = lambda: [hwc(c=4), hwc(c=4)]
    yield "flatten_images|background", lambda: sj.flatten_images(a(), background=(1, 2))
    yield "flatten_images|background_range", lambda: sj.flatten_images(a(), background=(1, 2, 256))
    yield "flatten_images|premultiplied", lambda: sj.flatten_images(a(), premultiplied=2)
    yield "flatten_images|alpha_scale", lambda: sj.flatten_images(a(), alpha_scale="x")
    yield "flatten_images|alpha_bias_nan", lambda: sj.flatten_images(a(), alpha_bias=float("nan"))
    yield "flatten_images|orientation_length", lambda: sj.flatten_images(a(), orientations=[1])
    yield "flatten_images|sizes_length", lambda: sj.flatten_images(a(), sizes=[(2, 2)])
    yield "flatten_images|a_flattened", lambda: sj.flatten_images(sj.Flattened(a()), background=(1, 2))
    yield "flatten_images|a_flattened_chw", lambda: sj.flatten_images(sj.Flattened(a()), layout="chw")
    # sheets
    for name in ("make_sheets", "encode_sheets"):
        f = CALLS[name][1]
        g = lambda: [hwc(), hwc()]
        yield f"{name}|sheet_none", lambda f=f, g=g: f(g(), "hwc", sheet=None)
        yield f"{name}|sheet_tuple", lambda f=f, g=g: f(g(), "hwc", sheet=(2, 2, (8, 8)))
        yield f"{name}|flatten_str", lambda f=f, g=g: f(g(), "hwc", flatten="white")
        yield f"{name}|flatten_true_no_sheet", lambda f=f, g=g: f(g(), "hwc", sheet=None, flatten=True)
        yield f"{name}|flatten_true_rgb", lambda f=f, g=g: f(g(), "hwc", flatten=True)
        yield f"{name}|flatten_false", lambda f=f, g=g: f(g(), "hwc", flatten=False)
        yield f"{name}|flatten_chw", lambda f=f: f([chw()], "chw", flatten=True)
        yield f"{name}|flatten_bad_tuple", lambda f=f, g=g: f(g(), "hwc", flatten=(1, 2))
        yield f"{name}|flatten_bad_background", lambda f=f, g=g: f(g(), "hwc", flatten=(1, 2, 300))
        yield f"{name}|flatten_long_tuple", lambda f=f, g=g: f(g(), "hwc", flatten=((1, 2, 3), 5))
        yield f"{name}|flatten_a_flattened", lambda f=f: f([hwc(c=4)], "hwc", flatten=sj.Flattened([hwc(c=4)]))
        yield f"{name}|flatten_a_flatten", lambda f=f: f([hwc(c=4)], "hwc", flatten=sj.Flatten())
        for fault, pics in alpha_faults():
            yield f"{name}|flatten|{fault}", lambda f=f, pics=pics: f(pics, "hwc", flatten=True)
        yield f"{name}|flatten|float_chw", lambda f=f: f(sj.FloatPixels([hwc(c=4, dtype=torch.float32)]), "chw", flatten=True)
        yield f"{name}|orientation_length", lambda f=f, g=g: f(g(), "hwc", orientations=[1])
        yield f"{name}|orientation_str", lambda f=f, g=g: f(g(), "hwc", orientations=["a", "b"])
        yield f"{name}|sizes_length", lambda f=f, g=g: f(g(), "hwc", sizes=[(2, 2)])
    yield "encode_sheets|yuv_mode_str", lambda: sj.encode_sheets([hwc()], SHEET, yuv_mode="x")
    yield "encode_sheets|both_targets", lambda: sj.encode_sheets([hwc()], SHEET, target_size=1, target_psnr=2)
    yield "encode_sheets|quality_length", lambda: sj.encode_sheets([hwc()], SHEET, quality=[1, 2])
    # decoded video
    y, uv, u = (lambda: fake(torch.zeros((10, 18), dtype=U8))), (lambda: fake(torch.zeros((5, 18), dtype=U8))), \
        (lambda: fake(torch.zeros((5, 9), dtype=U8)))
    for name, f in (("encode_yuv_frames", lambda fr, fmt=sj.SRC_NV12, **k: sj.encode_yuv_frames(fr, fmt, **k)),
                    ("encode_yuv_sheets", lambda fr, fmt=sj.SRC_NV12, **k: sj.encode_yuv_sheets(fr, fmt, SHEET, **k))):
        nv = lambda: [(y(), uv()), (y(), uv())]
        yield f"{name}|empty", lambda f=f: f([])
        yield f"{name}|good_nv12", lambda f=f, nv=nv: f(nv())
        yield f"{name}|good_yuv420", lambda f=f: f([(y(), u(), u())], sj.SRC_YUV420)
        yield f"{name}|fmt_rgb", lambda f=f, nv=nv: f(nv(), sj.SRC_RGB)
        yield f"{name}|fmt_21", lambda f=f, nv=nv: f(nv(), 21)
        yield f"{name}|three_planes_nv12", lambda f=f: f([(y(), uv()), (y(), u(), u())])
        yield f"{name}|two_planes_yuv420", lambda f=f, nv=nv: f(nv(), sj.SRC_YUV420)
        yield f"{name}|not_a_pair", lambda f=f: f([y()])
        yield f"{name}|numpy_plane", lambda f=f: f([(y(), np.zeros((5, 18), np.uint8))])
        yield f"{name}|cpu_plane", lambda f=f: f([(y(), torch.zeros((5, 18), dtype=U8))])
        yield f"{name}|int16_plane", lambda f=f: f([(fake(torch.zeros((10, 18), dtype=torch.int16)), uv())])
        yield f"{name}|rank3_plane", lambda f=f: f([(fake(torch.zeros((10, 18, 1), dtype=U8)), uv())])
        yield f"{name}|plane_strides", lambda f=f: f([(y(), uv())[::-1], (y(), fake(torch.zeros((5, 36), dtype=U8)[:, ::2]))])
        yield f"{name}|orientation_length", lambda f=f, nv=nv: f(nv(), orientations=[1])
        yield f"{name}|orientation_str", lambda f=f, nv=nv: f(nv(), orientations=["a", "b"])
        yield f"{name}|both_targets", lambda f=f, nv=nv: f(nv(), target_size=1, target_psnr=2)
        yield f"{name}|target_length", lambda f=f, nv=nv: f(nv(), target_size=[1])
        yield f"{name}|quality_length", lambda f=f, nv=nv: f(nv(), quality=[1])
    nv = lambda: [(y(), uv()), (y(), uv())]
    yield "encode_yuv_frames|sizes_and_box", lambda: sj.encode_yuv_frames(nv(), sizes=[(2, 2)] * 2, box=(4, 4))
    yield "encode_yuv_frames|box_int", lambda: sj.encode_yuv_frames(nv(), box=4)
    yield "encode_yuv_frames|box_triple", lambda: sj.encode_yuv_frames(nv(), box=(4, 4, 4))
    yield "encode_yuv_sheets|sheet_none", lambda: sj.encode_yuv_sheets(nv(), sj.SRC_NV12, None)
    # the wrapper classes: every ordered pair, their own arguments, the fits
    for oname, outer in WRAPPERS.items():
        for iname, inner in WRAPPERS.items():
            yield f"nest|{oname}({iname})", lambda outer=outer, inner=inner: outer(inner([hwc(c=4)]))
        yield f"nest|{oname}(FloatPixels)", lambda outer=outer: outer(sj.FloatPixels([hwc(c=4, dtype=torch.float32)]))
        yield f"nest|FloatPixels({oname})", lambda outer=outer: sj.FloatPixels(outer([hwc(c=4)]))
    yield "nest|Resized.fit(Reduced)", lambda: sj.Resized.fit(sj.Reduced([hwc()], 2), (2, 2))
    yield "nest|Resized.fit(Oriented)", lambda: sj.Resized.fit(sj.Oriented([hwc()], 2), (2, 2))
    yield "nest|Resized.fit(Flattened)", lambda: sj.Resized.fit(sj.Flattened([hwc(c=4)]), (2, 2))
    yield "nest|Oriented.fit(Resized)", lambda: sj.Oriented.fit(sj.Resized([hwc()], (2, 2)), 6, (2, 2))
    yield "nest|Oriented.from_metadata(Reduced)", lambda: sj.Oriented.from_metadata(sj.Reduced([hwc()], 2), None)
    yield "nest|Flattened.fit(Oriented)", lambda: sj.Flattened.fit(sj.Oriented([hwc(c=4)], 6), (2, 2))
    yield "Reduced|factor_length", lambda: sj.Reduced([hwc()], [1, 2])
    yield "Reduced|factor_0", lambda: sj.Reduced([hwc(), hwc()], [1, 0])
    yield "Reduced|factor_bool_array", lambda: sj.Reduced([hwc(), hwc()], np.array([1, 8]))
    yield "Reduced|no_pictures", lambda: sj.Reduced(5, 2)
    yield "Resized|sizes_length", lambda: sj.Resized([hwc()], [(1, 1), (2, 2)])
    yield "Resized|sizes_int", lambda: sj.Resized([hwc()], 5)
    yield "Resized|size_float", lambda: sj.Resized([hwc()], [(1.0, 2)])
    yield "Resized|size_big", lambda: sj.Resized([hwc(), hwc()], [(1, 1), (65536, 1)])
    yield "Resized|one_pair_for_two", lambda: sj.Resized([hwc(), hwc()], (3, 2)).sizes
    yield "Resized.fit|box_int", lambda: sj.Resized.fit([hwc()], 5)
    yield "Resized.fit|layout", lambda: sj.Resized.fit([hwc()], (2, 2), layout="x")
    yield "Resized.fit|rank1", lambda: sj.Resized.fit([fake(torch.zeros(4, dtype=U8))], (2, 2))
    yield "Resized.fit|numbers", lambda: sj.Resized.fit([5], (2, 2))
    yield "Oriented|orientation_length", lambda: sj.Oriented([hwc()], [1, 2])
    yield "Oriented|orientation_0", lambda: sj.Oriented([hwc()], 0)
    yield "Oriented|orientation_float", lambda: sj.Oriented([hwc()], 2.0)
    yield "Oriented|sizes_length", lambda: sj.Oriented([hwc()], 1, [(1, 1), (2, 2)])
    yield "Oriented|bad_orientation_and_sizes", lambda: sj.Oriented([hwc()], 9, 5)
    yield "Oriented.fit|box_int", lambda: sj.Oriented.fit([hwc()], 6, 5)
    yield "Oriented.fit|layout", lambda: sj.Oriented.fit([hwc()], 6, (2, 2), layout="x")
    yield "Oriented.fit|orientation_and_box", lambda: sj.Oriented.fit([hwc()], 9, 5)
    yield "Oriented.from_metadata|length", lambda: sj.Oriented.from_metadata([hwc()], [META, META])
    yield "Oriented.from_metadata|entry", lambda: sj.Oriented.from_metadata([hwc()], [5])
    yield "Oriented.from_metadata|none", lambda: sj.Oriented.from_metadata([hwc()], None)[0].orientations
    yield "Flattened|background", lambda: sj.Flattened([hwc(c=4)], background="white")
    yield "Flattened|orientation_length", lambda: sj.Flattened([hwc(c=4)], orientations=[1, 2])
    yield "Flattened|sizes_length", lambda: sj.Flattened([hwc(c=4)], sizes=[(1, 1), (2, 2)])
    yield "Flattened|background_and_orientation", lambda: sj.Flattened([hwc(c=4)], background=5, orientations=9)
    yield "Flattened.fit|chw", lambda: sj.Flattened.fit([hwc(c=4)], (2, 2), layout="chw")
    yield "Flattened.fit|layout", lambda: sj.Flattened.fit([hwc(c=4)], (2, 2), layout="x")
    yield "Flattened.fit|box_int", lambda: sj.Flattened.fit([hwc(c=4)], 5)
    yield "Flatten|background_length", lambda: sj.Flatten((1, 2))
    yield "Flatten|background_int", lambda: sj.Flatten(5)
    yield "Flatten|background_range", lambda: sj.Flatten((0, 0, -1))
    yield "Flatten|premultiplied", lambda: sj.Flatten(premultiplied="yes")
    yield "Flatten|alpha_scale", lambda: sj.Flatten(alpha_scale=None)
    yield "Flatten|alpha_scale_inf", lambda: sj.Flatten(alpha_scale=float("inf"))
    yield "Sheet|cell_int", lambda: sj.Sheet(2, 2, 8)
    yield "Sheet|background_int", lambda: sj.Sheet(2, 2, (8, 8), background=5)
    yield "Sheet|background_length", lambda: sj.Sheet(2, 2, (8, 8), background=(1, 2))
    yield "Sheet|background_range", lambda: sj.Sheet(2, 2, (8, 8), background=(1, 2, 256))
    yield "sheet_size|not_a_sheet", lambda: sj.sheet_size(5)
    yield "sheet_places|not_a_sheet", lambda: sj.sheet_places(5, [(4, 4)])
    yield "sheet_places|empty", lambda: sj.sheet_places(SHEET, [])
    yield "sheet_places|sizes_length", lambda: sj.sheet_places(SHEET, [(4, 4)], sizes=[(1, 1), (2, 2)])
    yield "sheet_places|orientation_length", lambda: sj.sheet_places(SHEET, [(4, 4)], orientations=[1, 2])
    yield "sheet_places|sizes_str", lambda: sj.sheet_places(SHEET, [(4, 4)], sizes=["ab"])
    yield "fit_size|box_int", lambda: sj.fit_size(4, 4, 5)
    yield "FloatPixels|scale_length", lambda: sj.FloatPixels([], scale=(1, 2))
    yield "FloatPixels|bias_nan", lambda: sj.FloatPixels([], bias=float("nan"))
    yield "FloatPixels.normalized|std_length", lambda: sj.FloatPixels.normalized([], 0.5, (1, 2))
    # the private helpers the host tests call
    yield "_float_pixels|hwc", lambda: sj._float_pixels("who", sj.FloatPixels([]), False)
    yield "_flattened|chw", lambda: sj._flattened("who", sj.Flattened([hwc(c=4)]), True)
    yield "_reduced|ones", lambda: sj._reduced(sj.Reduced([hwc()], 1))[1]
    yield "_reduced|twos", lambda: sj._reduced(sj.Reduced([hwc()], 2))[1]
    yield "_resized|sizes", lambda: sj._resized(sj.Resized([hwc()], (2, 3)))[1]
    yield "_oriented|ones", lambda: sj._oriented(sj.Oriented([hwc()], 1))[1]
    yield "_oriented|sizes", lambda: type(sj._oriented(sj.Oriented([hwc()], 6, (2, 3)))[0]).__name__
    yield "_sheet_flatten|str", lambda: sj._sheet_flatten("who", "x", SHEET)
    yield "_chw_planes|empty", lambda: sj._chw_planes("who", [])[3]
    yield "_metadata_args|str", lambda: sj._metadata_args("who", 1, "chw")
    yield "_metadata_args|length", lambda: sj._metadata_args("who", 1, [None, None])
    yield "_ragged_frames|empty", lambda: sj._ragged_frames([], [], None, None, None, None)
    yield "_ragged_args|quant_length", lambda: sj._ragged_args("who", 2, [np.ones((2, 64))], None, None, 1, [1, 1], [(1, 1)] * 2)
    yield "_ragged_args|search_length", lambda: sj._ragged_args("who", 2, np.ones((2, 64)), None, [{}], 1, [1, 1], [(1, 1)] * 2)
    # which refusal wins when two rules are broken
    cpu = lambda: torch.zeros((4, 5, 3), dtype=U8)
    yield "two|encode_images|method9+cpu_tensor", lambda: sj.encode_images([cpu()], method=9)
    yield "two|encode_images_full|method9+cpu_tensor", lambda: sj.encode_images_full([cpu()], method=9)
    yield "two|riskiness_images|layout+Reduced", lambda: sj.riskiness_images(sj.Reduced([hwc()], 2), layout="x")
    yield "two|make_sheets|layout+Resized", lambda: sj.make_sheets(sj.Resized([hwc()], (2, 2)), SHEET, layout="x")
    yield "two|encode_images|quality_length+cpu_tensor", lambda: sj.encode_images([cpu()], quality=[1, 2])
    yield "two|encode_images_full|quality_length+cpu_tensor", lambda: sj.encode_images_full([cpu()], quality=[1, 2])
    yield "two|encode_images|both_targets+yuv_mode9", lambda: sj.encode_images([hwc()], target_size=1, target_psnr=2, yuv_mode=9)
    yield "two|encode_images|trellis_target+method7", lambda: sj.encode_images([hwc()], method=7, use_trellis=True, target_size=1)
    yield "two|encode_images|float_hwc+both_targets", lambda: sj.encode_images(sj.FloatPixels([]), target_size=1, target_psnr=2)
    yield "two|encode_images|flattened_chw+float_hwc", lambda: sj.encode_images(sj.Flattened(sj.FloatPixels([])), layout="chw")
    yield "two|encode_images|empty+quality_length", lambda: sj.encode_images([], quality=[1, 2])
    yield "two|encode_images_full|empty+yuv_mode9", lambda: sj.encode_images_full([], yuv_mode=9)
    yield "two|encode_images|auto_not_rgb+quality_length", lambda: sj.encode_images([hwc(c=4)], yuv_mode=sj.YUV_AUTO, method=4, quality=[1, 2])
    yield "two|encode_images|int16+second_numpy", lambda: sj.encode_images([hwc(dtype=torch.int16), np.zeros((4, 5, 3), np.uint8)])
    yield "two|encode_images|gray_mode+second_device", lambda: sj.encode_images(
        sj.FloatPixels([fake(torch.zeros((4, 5), dtype=torch.float32)), fake1(torch.zeros((4, 5), dtype=torch.float32))]), layout="chw")
    yield "two|encode_yuv_frames|fmt+empty", lambda: sj.encode_yuv_frames([], sj.SRC_RGB)
    yield "two|encode_yuv_frames|sizes_and_box+cpu_plane", lambda: sj.encode_yuv_frames(
        [(y(), torch.zeros((5, 18), dtype=U8))], sizes=[(2, 2)], box=(4, 4))
    yield "two|encode_yuv_frames|box+both_targets", lambda: sj.encode_yuv_frames(nv(), box=4, target_size=1, target_psnr=2)
    yield "two|make_sheets|flatten_str+layout", lambda: sj.make_sheets([hwc()], SHEET, layout="x", flatten="white")
    yield "two|encode_sheets|gray_mode+orientation_length", lambda: sj.encode_sheets(
        sj.FloatPixels([fake(torch.zeros((4, 5), dtype=torch.float32))]), SHEET, layout="chw", orientations=[1, 2])
    yield "two|reduce_images|factor9+layout", lambda: sj.reduce_images([hwc()], 9, layout="x")
    yield "two|resize_images|sizes+cpu_tensor", lambda: sj.resize_images([cpu()], 5)
    yield "two|flatten_images|layout_chw+rgb", lambda: sj.flatten_images([hwc()], layout="chw")


def _engine_cases():
    """the Engine methods' own length checks, on an engine that was never created: they stop before the handle is read"""
    def eng():
        e = _REAL_ENGINE.__new__(_REAL_ENGINE)
        e._h = C.c_void_p()            # (null: close() leaves it alone, and the library refuses it should a case get that far)
        e.device = 0
        return e
    plane = lambda: [fake(torch.zeros((4, 15), dtype=U8))]
    quant = np.ones((2, 64), np.uint8)
    one = lambda: ([plane()], [(5, 4)])
    two = lambda: ([plane(), plane()], [(5, 4), (5, 4)])
    caps = {"capacities": [4096, 4096]}
    # (method, the arguments between dims and yuv_mode for two frames, the same with a wrong length or None)
    full = [("encode_ragged_full", (), None), ("encode_ragged_full_packed", (), None), ("encode_ragged_packed", (), None),
            ("encode_ragged_reduced", ([2, 2],), ([2],)), ("encode_ragged_reduced_packed", ([2, 2],), ([2],)),
            ("encode_ragged_resized", ([(2, 2)] * 2,), ([(2, 2)],)), ("encode_ragged_resized_packed", ([(2, 2)] * 2,), ([(2, 2)],)),
            ("encode_ragged_oriented", ([(2, 2)] * 2, [1, 6]), ([(2, 2)], [1, 6])),
            ("encode_ragged_oriented_packed", ([(2, 2)] * 2, [1, 6]), ([(2, 2)], [1, 6])),
            ("encode_ragged_flattened", (sj.Flatten(), [(2, 2)] * 2, [1, 6]), (sj.Flatten(), [(2, 2)], [1, 6])),
            ("encode_ragged_flattened_packed", (sj.Flatten(), [(2, 2)] * 2, [1, 6]), (sj.Flatten(), [(2, 2)], [1, 6])),
            ("encode_ragged_yuv_resized", ([(2, 2)] * 2, [1, 6]), ([(2, 2)], [1, 6])),
            ("encode_ragged_yuv_resized_packed", ([(2, 2)] * 2, [1, 6]), ([(2, 2)], [1, 6]))]
    for name, extra, short in full:
        m = lambda name=name: getattr(eng(), name)
        yield f"Engine.{name}|no_frames", lambda m=m, extra=extra: m()(sj.SRC_RGB, [], [], *extra, sj.YUV_420, quant)
        yield f"Engine.{name}|planes_length", lambda m=m, extra=extra: m()(sj.SRC_RGB, [plane()], two()[1], *extra, sj.YUV_420, quant)
        yield f"Engine.{name}|quant_length", lambda m=m, extra=extra: m()(sj.SRC_RGB, *two(), *extra, sj.YUV_420, [quant], **caps)
        yield f"Engine.{name}|search_length", lambda m=m, extra=extra: m()(sj.SRC_RGB, *two(), *extra, sj.YUV_420, quant, search=[{}], **caps)
        if short is not None:
            yield f"Engine.{name}|extra_length", lambda m=m, short=short: m()(sj.SRC_RGB, *two(), *short, sj.YUV_420, quant, **caps)
        if name != "encode_ragged_packed":
            yield f"Engine.{name}|metadata_length", lambda m=m, extra=extra: m()(sj.SRC_RGB, *two(), *extra, sj.YUV_420, quant, metadata=[None], **caps)
            yield f"Engine.{name}|metadata_str", lambda m=m, extra=extra: m()(sj.SRC_RGB, *two(), *extra, sj.YUV_420, quant, metadata="x", **caps)
            yield f"Engine.{name}|metadata_entry", lambda m=m, extra=extra: m()(sj.SRC_RGB, *two(), *extra, sj.YUV_420, quant, metadata=[5, None], **caps)
        if "oriented" in name or "flattened" in name or "yuv" in name:
            yield f"Engine.{name}|orientation_length", lambda m=m, extra=extra: m()(
                sj.SRC_RGB, *two(), *extra[:-1], [1], sj.YUV_420, quant, **caps)
            yield f"Engine.{name}|sizes_str", lambda m=m, extra=extra: m()(
                sj.SRC_RGB, *two(), *extra[:-2], ["ab", "cd"], extra[-1], sj.YUV_420, quant, **caps)
        if name in ("encode_ragged_packed", "encode_ragged_full_packed"):
            yield f"Engine.{name}|capacity_length", lambda m=m, extra=extra: m()(sj.SRC_RGB, *two(), *extra, sj.YUV_420, quant, capacities=[4096])
    yield "Engine.reduce_ragged|factor_length", lambda: eng().reduce_ragged(sj.SRC_RGB, *two(), [2])
    yield "Engine.reduce_ragged|no_frames", lambda: eng().reduce_ragged(sj.SRC_RGB, [], [], [])
    yield "Engine.resize_ragged|sizes_length", lambda: eng().resize_ragged(sj.SRC_RGB, *two(), [(2, 2)])
    yield "Engine.resize_ragged|sizes_str", lambda: eng().resize_ragged(sj.SRC_RGB, *two(), ["ab", "cd"])
    yield "Engine.resize_ragged|planes_length", lambda: eng().resize_ragged(sj.SRC_RGB, [plane()], two()[1], [(2, 2)] * 2)
    for name, pre in (("orient_ragged", ()), ("flatten_ragged", (sj.Flatten(),)), ("resize_ragged_yuv", ())):
        m = lambda name=name: getattr(eng(), name)
        yield f"Engine.{name}|sizes_length", lambda m=m, pre=pre: m()(sj.SRC_RGB, *two(), *pre, [(2, 2)], [1, 6])
        yield f"Engine.{name}|sizes_str", lambda m=m, pre=pre: m()(sj.SRC_RGB, *two(), *pre, ["ab", "cd"], [1, 6])
        yield f"Engine.{name}|orientation_length", lambda m=m, pre=pre: m()(sj.SRC_RGB, *two(), *pre, [(2, 2)] * 2, [1])
        yield f"Engine.{name}|orientation_str", lambda m=m, pre=pre: m()(sj.SRC_RGB, *two(), *pre, None, ["a", "b"])
        yield f"Engine.{name}|no_frames", lambda m=m, pre=pre: m()(sj.SRC_RGB, [], [], *pre, None, None)
    yield "Engine.flatten_ragged|not_a_flatten", lambda: eng().flatten_ragged(sj.SRC_RGBA, *two(), (255, 255, 255))
    yield "Engine.sheet_ragged|sizes_length", lambda: eng().sheet_ragged(sj.SRC_RGB, *two(), SHEET, [(2, 2)])
    yield "Engine.sheet_ragged|not_a_sheet", lambda: eng().sheet_ragged(sj.SRC_RGB, *two(), 5)
    yield "Engine.sheet_ragged|no_frames", lambda: eng().sheet_ragged(sj.SRC_RGB, [], [], SHEET)
    yield "Engine.sheet_ragged|orientation_length", lambda: eng().sheet_ragged(sj.SRC_RGB, *two(), SHEET, None, [1])
    for name in ("encode_ragged_sheet", "encode_ragged_sheet_packed"):
        m = lambda name=name: getattr(eng(), name)
        yield f"Engine.{name}|no_frames", lambda m=m: m()(sj.SRC_RGB, [], [], SHEET, None, None, sj.YUV_420, quant)
        yield f"Engine.{name}|sizes_length", lambda m=m: m()(sj.SRC_RGB, *two(), SHEET, [(2, 2)], None, sj.YUV_420, quant)
        yield f"Engine.{name}|not_a_sheet", lambda m=m: m()(sj.SRC_RGB, *two(), 5, None, None, sj.YUV_420, quant)


_REAL_ENGINE = sj.Engine


def cases():
    """(label, call, whether sjpeg_amd.Engine is the guard while it runs) of every case, in the order of the file"""
    for label, call in _public_cases():
        yield label, call, True
    for label, call in _engine_cases():
        yield label, call, False


def answer(call, guarded):
    """ "ok", or "Class: text" of what the call raises; the result of a call that returns is not recorded but for small
    values (lists, tuples, numbers, names), which are: "ok: <repr>" """
    if guarded:
        sj.Engine = _GuardEngine
    try:
        got = call()
    except Exception as e:                       # noqa: BLE001 (the class is part of the record)
        return f"{type(e).__name__}: {e}"
    finally:
        sj.Engine = _REAL_ENGINE
    if isinstance(got, (list, tuple, int, float, str, type(None))) and len(repr(got)) < 200 and "tensor" not in repr(got) \
            and " object at " not in repr(got):
        return f"ok: {got!r}"
    return "ok"


def signatures():
    """name -> str(inspect.signature(...)) of every public function and class of the binding, and of every public method
    and classmethod of its classes (the ctypes structures, which have no signature of their own, excepted)"""
    out = {}

    def sig(name, obj):
        try:
            out[name] = str(inspect.signature(obj))
        except (TypeError, ValueError):
            pass

    for name, obj in sorted(vars(sj).items()):
        if name.startswith("_") or getattr(obj, "__module__", None) != sj.__name__:
            continue
        if inspect.isfunction(obj):
            sig(name, obj)
        elif inspect.isclass(obj) and not issubclass(obj, (C.Structure, BaseException)):
            sig(name, obj)
            for mname, member in sorted(vars(obj).items()):
                if mname.startswith("_"):
                    continue
                if isinstance(member, (classmethod, staticmethod)):
                    sig(f"{name}.{mname}", getattr(obj, mname))
                elif inspect.isfunction(member):
                    sig(f"{name}.{mname}", member)
    return out


def digest(labels):
    return hashlib.sha256("\n".join(labels).encode()).hexdigest()


def _split(a):
    """an answer "Class: caller: text" as ("Class: caller", "text"): the same text comes from many callers"""
    parts = a.split(": ", 2)
    return (": ".join(parts[:2]), parts[2]) if len(parts) == 3 else ("", a)


def _join(head, text):
    return head + ": " + text if head else text


def recorded():
    """(label -> answer, signatures) as the file holds them: every distinct head ("Class: caller") and every distinct text
    once, the cases as pairs of indices (head, text) in the order of cases(), whose labels the file knows by their digest"""
    with open(OUT) as f:
        d = json.load(f)
    labels = [label for label, _, _ in cases()]
    assert 2 * len(labels) == len(d["cases"]) and digest(labels) == d["labels_sha256"], "the table is not the recorded one"
    pairs = zip(d["cases"][0::2], d["cases"][1::2])
    return {label: _join(d["heads"][h], d["texts"][t]) for label, (h, t) in zip(labels, pairs)}, d["signatures"]


def main():
    heads, texts, row, labels, reached = [], [], [], [], 0
    for label, call, guarded in cases():
        assert label not in labels, label
        labels.append(label)
        a = answer(call, guarded)
        assert _join(*_split(a)) == a
        reached += a.startswith("ReachedEngine")
        for part, known in zip(_split(a), (heads, texts)):
            if part not in known:
                known.append(part)
            row.append(known.index(part))
    sigs = signatures()
    lines = lambda items: ",\n".join(json.dumps(x) for x in items)
    with open(OUT, "w") as f:
        f.write('{"heads": [\n' + lines(heads) + '\n],\n"texts": [\n' + lines(texts) + '\n],\n"labels_sha256": "%s",\n' % digest(labels))
        f.write('"cases": [\n' + ",\n".join(",".join(str(i) for i in row[k:k + 60]) for k in range(0, len(row), 60)) + '\n],\n')
        f.write('"signatures": {\n' + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sigs.items()) + "\n}}\n")
    print("wrote", len(labels), "cases (", reached, "went on to an Engine ),", len(heads), "heads,", len(texts), "texts,", len(sigs),
          "signatures,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
