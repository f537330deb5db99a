"""Records what the shaped ragged entries of the C layer answer to calls they refuse on the host -- the return code and
the text of sjpeg_hip_last_error() -- in tests/golden/c_messages.json: the four _full[_meta][_packed]_src entries, the
_reduced, _resized, _oriented, _flattened, _yuv_resized, _sheet and _sheet_flat encode entries with their _packed twins
and the seven shape entries (sjpeg_hip_reduce_ragged_src ... sjpeg_hip_sheet_ragged_flat_src), 25 in all -- and, behind
them in the file, the twelve families added since (video colour, 16-bit planes, linear light, unsharp, the two resample
families, Pillow's filters, compose): each one's encode entry, packed twin and shape entry, and
sjpeg_hip_compose_ragged_bytes, the one _bytes entry that lives beside them and answers a refusal with 0; 62 in all.
Every call is one that is refused before the engine is read, so no GPU is needed and the stand-in engine pointer of the other
*_host.py tests is never followed.  tests/test_c_messages_host.py replays the same calls (cases() below) on the current
build and wants the same answers, byte for byte.

The file is made with the library of the commit BEFORE a change to these entries, never with the change itself:

    SJPEG_AMD_LIB=<the parent's libsjpeg_amd.so> python tests/golden/make_c_messages.py

What is recorded, per entry:
  routes   every combination of the arguments that decide which body a call takes, and with it whose name a message
           carries: factors NULL / all 1 / one 2; sizes NULL / every frame's own / one smaller; orientations NULL / all
           1 / one 6; flatten NULL / given; meta NULL / given (one entry per frame).  Where an entry refuses a NULL
           (the shape entries' factors, sizes and flatten) that NULL is a fault, not a route.  The newer families' own
           axes -- colour, depth, light, unsharp, filter, compose -- and what becomes of sizes and orientations there
           are stated at NEWER_VALUES below.
  faults   FAULTS below: every way the entry can be refused on the host, alone -- and every pair of them that one call
           can hold (two faults that write the same argument cannot).  A pair is one call whichever of the two is named
           first, so it is recorded once; which of the two the entry reports pins the order of its checks.
A fault that needs an argument the route leaves NULL (an orientation of 0 without orientations) is not made on that
route; a format that an entry only refuses where it has to read it (a YUV-plane format on the resize entries) is made
on the routes that do not pass the call through.  ROUTE RULES below states which those are, on its own.

The stand-in engine is the pointer of the other *_host.py tests, which no refused call follows -- with one exception:
the _full_meta_ entries hang the call's checked metadata on the engine and take it off again around their remaining
checks, so on the routes that reach them WITH metadata a zeroed block stands in (as make_source_messages.py does for
the uniform entry), and every answer recorded there must be SJPEG_HIP_EINVAL: a call that got past its checks would
answer with a runtime error of the device instead.

Before each call a call of a known answer is made, so that an entry that returns its code without a message of its own
is recorded with that text and not with whatever came before.  The recording is stored as the other goldens are: the
distinct answers once, then per entry a number for every case's answer (run-length coded: [number, count, ...]; "how
the recording is stored" below) and a digest of its labels."""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import sjpeg_amd as sj  # noqa: E402
from sjpeg_amd import _binding, resample, unsharp, video  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "c_messages.json")
FAKE = 1 << 20                                   # the stand-in engine: never read by a refused call
LONG = 65536                                     # every array is this long: nframes 65536 finds its arrays allocated
DIMS = ((33, 17), (16, 16), (8, 50))
RGB, RGBA, GRAY, NV12 = 0, 2, 3, 6
EINVAL = -1                                      # SJPEG_HIP_EINVAL
CELL = (40, 50)                                  # holds every picture at its own size

# ---- the entries: name -> (kind, family, packed)
FAMILIES = {  # family -> (encode stem or None, shape entry or None, the arguments between params / frames and the rest, base format)
    "full": ("full", None, (), RGB),
    "full_meta": ("full_meta", None, (), RGB),
    "reduce": ("reduced", "sjpeg_hip_reduce_ragged_src", ("factors",), RGB),
    "resize": ("resized", "sjpeg_hip_resize_ragged_src", ("sizes",), RGB),
    "orient": ("oriented", "sjpeg_hip_orient_ragged_src", ("sizes", "orientations"), RGB),
    "flatten": ("flattened", "sjpeg_hip_flatten_ragged_src", ("flatten", "sizes", "orientations"), RGBA),
    "yuv": ("yuv_resized", "sjpeg_hip_resize_ragged_yuv_src", ("sizes", "orientations"), NV12),
    "sheet": ("sheet", "sjpeg_hip_sheet_ragged_src", ("sheet", "sizes", "orientations"), RGB),
    "sheet_flat": ("sheet_flat", "sjpeg_hip_sheet_ragged_flat_src", ("sheet", "flatten", "sizes", "orientations"), RGBA),
    # ... and the twelve families added since (NEWER below): their segments are those of sjpeg_amd/_binding.py's rows
    "yuv_converted": ("yuv_converted", "sjpeg_hip_convert_ragged_yuv_src", ("sizes", "orientations", "colour"), NV12),
    "sheet_yuv_colour": ("sheet_yuv_colour", "sjpeg_hip_sheet_ragged_yuv_colour_src", ("sheet", "sizes", "orientations", "colour"), NV12),
    "yuv16": ("yuv16", "sjpeg_hip_convert_ragged_yuv16_src", ("sizes", "orientations", "colour", "depth"), NV12),
    "sheet_yuv16": ("sheet_yuv16", "sjpeg_hip_sheet_ragged_yuv16_src", ("sheet", "sizes", "orientations", "colour", "depth"), NV12),
    "linear": ("linear", "sjpeg_hip_linear_ragged_src", ("flatten", "light", "sizes", "orientations"), RGBA),
    "sheet_linear": ("sheet_linear", "sjpeg_hip_sheet_ragged_linear_src", ("sheet", "flatten", "light", "sizes", "orientations"), RGBA),
    "unsharp": ("unsharp", "sjpeg_hip_unsharp_ragged_src", ("flatten", "light", "sizes", "orientations", "unsharp"), RGBA),
    "yuv_unsharp": ("yuv_unsharp", "sjpeg_hip_unsharp_ragged_yuv_src", ("sizes", "orientations", "colour", "depth", "unsharp"), NV12),
    "resampled": ("resampled", "sjpeg_hip_resample_ragged_src", ("flatten", "sizes", "orientations", "resample", "unsharp"), RGBA),
    "resampled_box": ("resampled_box", "sjpeg_hip_resample_box_ragged_src",
                      ("flatten", "sizes", "orientations", "resample", "box", "unsharp"), RGBA),
    "filtered": ("filtered", "sjpeg_hip_filter_ragged_src", ("flatten", "sizes", "orientations", "resample", "box", "filter"), RGBA),
    "composed": ("composed", "sjpeg_hip_compose_ragged_src",
                 ("flatten", "sizes", "orientations", "resample", "box", "filter", "compose", "overlays", "places"), RGBA),
}
OLDER = 9                                        # the families of the first recording: their 25 entries come first, unchanged
NEWER = list(FAMILIES)[OLDER:]
SHEETS = ("sheet", "sheet_flat", "sheet_yuv_colour", "sheet_yuv16", "sheet_linear")
YUV = ("yuv", "yuv_converted", "sheet_yuv_colour", "yuv16", "sheet_yuv16", "yuv_unsharp")
BYTES_ENTRY = "sjpeg_hip_compose_ragged_bytes"   # the one _bytes entry of ragged_shaped.cc: a refusal answers 0
BYTES_SEGMENTS = ("sizes", "orientations", "box", "compose")
ENTRIES = {}
for _fam, (_stem, _shape, _, _) in FAMILIES.items():
    ENTRIES["sjpeg_hip_encode_ragged_%s_src" % _stem] = ("encode", _fam, False)
    ENTRIES["sjpeg_hip_encode_ragged_%s_packed_src" % _stem] = ("encode", _fam, True)
    if _shape is not None:
        ENTRIES[_shape] = ("shape", _fam, False)
ENTRIES[BYTES_ENTRY] = ("bytes", "composed", False)
assert len(ENTRIES) == 25 + 3 * len(NEWER) + 1 and list(ENTRIES)[24] == "sjpeg_hip_sheet_ragged_flat_src"
# family -> the stem of sjpeg_hip_<stem>_bytes, which says what the made pictures take
BYTES_FN = {"reduce": "reduce_ragged", "resize": "resize_ragged", "orient": "orient_ragged", "flatten": "orient_ragged",
            "yuv": "resize_ragged_yuv", "sheet": "sheet_ragged", "sheet_flat": "sheet_ragged",
            "yuv_converted": "resize_ragged_yuv", "sheet_yuv_colour": "sheet_ragged", "yuv16": "resize_ragged_yuv", "sheet_yuv16": "sheet_ragged",
            "linear": "orient_ragged", "sheet_linear": "sheet_ragged", "unsharp": "orient_ragged", "yuv_unsharp": "resize_ragged_yuv",
            "resampled": "resample_ragged", "resampled_box": "resample_box_ragged", "filtered": "resample_box_ragged",
            "composed": "compose_ragged"}


def segments(c):
    """the names of the arguments between params (frames) and the rest of the entry a call is for"""
    return BYTES_SEGMENTS if c.kind == "bytes" else FAMILIES[c.family][2]


class Call:
    """one call's arguments, as plain values; invoke() turns them into the C ones"""

    def __init__(self, entry):
        self.entry = entry
        self.kind, self.family, self.packed = ENTRIES[entry]
        self.engine, self.format, self.nframes = FAKE, FAMILIES[self.family][3], 3
        self.frames, self.dims = True, [list(d) for d in DIMS]
        self.params, self.yuv_mode, self.method, self.qdelta, self.quant = True, 1, 0, 12, True
        self.search = None                       # (per_frame, index, target_mode, target_value)
        self.factors = self.sizes = self.orientations = None     # None or a list of three
        self.sheet, self.cell = True, CELL
        self.flatten = None                      # None or `premultiplied`
        self.meta = None                         # None or (per_frame, index of the entry with exif NULL and a size, or -1)
        self.out, self.capacity, self.offsets, self.d_sizes, self.out_stride = 1 << 16, 1 << 24, True, True, 1 << 20
        self.bytes_short, self.out_frames, self.out_format, self.nsheets = False, True, True, True
        # the newer families' segments: None, or a list per frame of the struct's fields in the header's order (always
        # per frame, so that a message names the frame); depth is one struct
        self.colour = self.depth = self.unsharp = self.filter = self.compose = None
        self.light = 0
        self.resample = [[4, 0] for _ in DIMS]                                       # (Lanczos)
        self.box = [[1.0, 1.0, w - 1.0, h - 1.0, 0.0] for w, h in DIMS]             # (cut one pixel in on each side, no reducing_gap)
        self.overlays, self.places = [[1 << 26, 4, 4, 16]], [[0, 1, 1, 3, 0]]      # (rgba, width, height, stride), (overlay, x, y, anchor, reserved)


# ---- ROUTE RULES: the routes of an entry, and whether a route passes the call through to the entry of fewer arguments
def _route_values(name):
    if name == "factors":
        return (("f-", None), ("f1", [1, 1, 1]), ("f2", [2, 1, 1]))
    if name == "sizes":
        return (("s-", None), ("s=", [list(d) for d in DIMS]), ("s<", [[20, 11]] + [list(d) for d in DIMS[1:]]))
    if name == "orientations":
        return (("o-", None), ("o1", [1, 1, 1]), ("o6", [6, 1, 1]))
    if name == "flatten":
        return (("a-", None), ("a+", 0))
    return (("m-", None), ("m+", (1, -1)))       # meta


# The newer families.  Their own arguments are the axes: colour NULL / the identity / a real matrix; depth NULL / given
# (the yuv16 entries refuse the NULL: a fault); light coded / linear; unsharp NULL / amount 0 / sharpening; filter NULL /
# kind 0 / a Gaussian blur; compose NULL / a canvas of every made picture's own size / a real canvas / a place on the
# picture's own canvas; flatten and meta as above.  sizes and orientations decide nothing there but how far a call that
# is passed on travels, so they are one axis of two values -- both NULL, or one size smaller and one orientation 6 --
# on the four families whose routes end in the _full_meta_ entries, and the second value everywhere else.
S_LT = [[20, 11]] + [list(d) for d in DIMS[1:]]
MADE = [[11, 20]] + [list(d) for d in DIMS[1:]]  # (what S_LT under orientation 6 makes, upright)
_comp = lambda cw, ch, px, py, nplaces: [cw, ch, 0, px, py, 0, 0.5, 0.5, 0, nplaces]    # (canvas, mode, px, py, reserved, cx, cy, first_place, nplaces)
NEWER_VALUES = {
    "shape": (("p-", {"sizes": None, "orientations": None}), ("p<", {"sizes": S_LT, "orientations": [6, 1, 1]})),
    "colour": (("c-", None), ("c=", [[0, 0, 0]] * 3), ("c7", [[1, 1, 0], [0, 0, 0], [1, 0, 0]])),      # (matrix, range, reserved)
    "depth": (("d-", None), ("d+", [2, 6, 0])),                                                          # (bytes, shift, reserved)
    "light": (("l0", 0), ("l1", 1)),
    "unsharp": (("u-", None), ("u0", [[0, 0, 0]] * 3), ("u+", [[128, 2, 0], [0, 0, 0], [64, 0, 0]])),   # (amount, threshold, reserved)
    "filter": (("k-", None), ("k0", [[0, 0, 0, 0.0, 0.0, 0]] * 3),                                      # (kind, threshold, percent, radii, reserved)
               ("kg", [[2, 0, 0, 1.0, 1.0, 0], [0, 0, 0, 0.0, 0.0, 0], [2, 0, 0, 1.0, 1.0, 0]])),
    "compose": (("x-", None), ("x=", [_comp(w, h, 0, 0, 0) for w, h in MADE]), ("x+", [_comp(64, 64, 2, 3, 0)] * 3),
                ("xp", [_comp(0, 0, 0, 0, 1)] * 3)),
}
NEWER_AXES = {
    "yuv_converted": ("shape", "colour"), "sheet_yuv_colour": ("colour",), "yuv16": ("colour",), "sheet_yuv16": ("colour",),
    "linear": ("shape", "flatten", "light"), "sheet_linear": ("flatten", "light"), "unsharp": ("shape", "flatten", "light", "unsharp"),
    "yuv_unsharp": ("shape", "colour", "depth", "unsharp"), "resampled": ("flatten", "unsharp"), "resampled_box": ("flatten", "unsharp"),
    "filtered": ("flatten", "filter"), "composed": ("flatten", "filter", "compose"),
}


def _newer_routes(kind, family):
    names = list(NEWER_AXES[family]) if kind != "bytes" else ["compose"]
    if kind == "encode":
        names.append("meta")
    axes = [[(n, lab, v) for lab, v in (NEWER_VALUES[n] if n in NEWER_VALUES else _route_values(n))] for n in names]
    for combo in itertools.product(*axes):
        route = dict(NEWER_VALUES["shape"][1][1])
        if family in ("yuv16", "sheet_yuv16"):
            route["depth"] = NEWER_VALUES["depth"][1][1]
        for n, _, v in combo:
            route.update(v if n == "shape" else {n: v})
        yield "".join(lab for _, lab, _ in combo), route


def routes(entry):
    """(label, {argument: value}) of every route of an entry"""
    kind, family, _ = ENTRIES[entry]
    if family in NEWER:
        yield from _newer_routes(kind, family)
        return
    names = [n for n in FAMILIES[family][2] if n != "sheet"]
    if kind == "encode" and family != "full":
        names.append("meta")
    axes = []
    for n in names:
        vals = _route_values(n)
        if kind == "shape" and (n == "flatten" or family in ("reduce", "resize")):
            vals = vals[1:]                      # (NULL is refused there: a fault)
        axes.append([(n, lab, v) for lab, v in vals])
    for combo in itertools.product(*axes):
        yield "".join(lab for _, lab, _ in combo) or "-", {n: v for n, _, v in combo}


def hangs_metadata(c):
    """is this a route on which a _full_meta_ entry is reached with metadata?"""
    # (a newer family: wherever there is metadata -- the stand-in block is no less safe than the stand-in pointer)
    return c.meta is not None and (c.family == "full_meta" or c.family in NEWER or passes_through(c))


def passes_through(c):
    """does the call, as its route stands, go to the _full_meta_ entries without reading its pictures?"""
    if c.kind != "encode" or c.family in ("full", "full_meta") or c.family in SHEETS or c.flatten is not None:
        return False
    if c.family in NEWER:                        # (what stands between the entry and the older one it ends in)
        plainly = {"yuv_converted": c.colour in (None, [[0, 0, 0]] * 3), "linear": c.light == 0,
                   "unsharp": c.light == 0 and c.unsharp in (None, [[0, 0, 0]] * 3),
                   "yuv_unsharp": c.colour in (None, [[0, 0, 0]] * 3) and c.depth is None and c.unsharp in (None, [[0, 0, 0]] * 3)}
        if not plainly.get(c.family, False):
            return False
    plain = lambda v, own: v is None or v == own
    return plain(c.factors, [1, 1, 1]) and plain(c.sizes, [list(d) for d in DIMS]) and plain(c.orientations, [1, 1, 1])


# ---- FAULTS: (name, the arguments it writes, where it can be made, what it does)
def _set(**kw):
    def apply(c):
        for k, v in kw.items():
            setattr(c, k, v)
    return apply


def _at1(name, value):
    def apply(c):
        getattr(c, name)[1] = value
    return apply


def _width0(c):
    c.dims[1][0] = 0


def _in(name, k, field, value):
    """field `field` of struct k of a segment"""
    def apply(c):
        getattr(c, name)[k] = list(getattr(c, name)[k])
        getattr(c, name)[k][field] = value
    return apply


def _depth(field, value):
    def apply(c):
        c.depth = list(c.depth)
        c.depth[field] = value
    return apply


def _canvas_4x4(c):
    c.compose[1] = list(c.compose[1])
    c.compose[1][0] = c.compose[1][1] = 4


enc = lambda c: c.kind == "encode"
shape = lambda c: c.kind == "shape"
called = lambda c: c.kind != "bytes"             # (the _bytes entry has neither engine nor buffer)
has = lambda name: (lambda c: getattr(c, name) is not None)
sheets = lambda c: c.family in SHEETS
takes = lambda name: (lambda c: name in segments(c))
both = lambda *fs: (lambda c: all(f(c) for f in fs))
given = lambda name: both(takes(name), has(name))
# the routes on which an RGB-like family reads the format: not where it hands the call on unread, and a sheet in coded
# light takes the YUV-plane formats as the sheet entries do
reads_rgb = lambda c: (c.family in ("reduce", "resize", "orient", "flatten", "linear", "unsharp", "resampled", "resampled_box", "filtered",
                                    "composed") and not passes_through(c)) or (c.family == "sheet_linear" and c.light != 0)
FAULTS = [
    ("engine_null", {"engine"}, called, _set(engine=None)),
    ("params_null", {"params"}, enc, _set(params=None)),
    ("frames_null", {"frames"}, lambda c: True, _set(frames=None)),
    ("sheet_null", {"sheet"}, sheets, _set(sheet=None)),
    ("flatten_null", {"flatten"}, both(shape, lambda c: c.family in ("flatten", "sheet_flat")), _set(flatten=None)),
    ("factors_null", {"factors"}, both(shape, takes("factors")), _set(factors=None)),
    ("sizes_null", {"sizes"}, both(shape, lambda c: c.family == "resize"), _set(sizes=None)),
    ("d_offsets_null", {"offsets"}, lambda c: c.packed, _set(offsets=None)),
    ("out_null", {"out"}, called, _set(out=None)),
    ("d_sizes_null", {"d_sizes"}, enc, _set(d_sizes=None)),
    ("out_frames_null", {"out_frames"}, shape, _set(out_frames=None)),
    ("out_format_null", {"out_format"}, shape, _set(out_format=None)),
    ("nsheets_null", {"nsheets"}, both(shape, sheets), _set(nsheets=None)),
    ("out_unaligned", {"out"}, lambda c: c.packed or c.kind == "shape", _set(out=(1 << 16) + 8)),
    ("capacity_2_63", {"capacity"}, lambda c: c.packed, _set(capacity=1 << 63)),
    ("nframes_0", {"nframes"}, lambda c: True, _set(nframes=0)),
    ("nframes_65536", {"nframes"}, lambda c: True, _set(nframes=LONG)),
    ("out_stride_0", {"out_stride"}, both(enc, sheets, lambda c: not c.packed), _set(out_stride=0)),
    ("factor_0", {"factors"}, has("factors"), _at1("factors", 0)),
    ("factor_9", {"factors"}, has("factors"), _at1("factors", 9)),
    ("orientation_0", {"orientations"}, has("orientations"), _at1("orientations", 0)),
    ("orientation_9", {"orientations"}, has("orientations"), _at1("orientations", 9)),
    ("format_-1", {"format"}, lambda c: True, _set(format=-1)),
    ("format_22", {"format"}, lambda c: True, _set(format=22)),
    ("format_not_yuv", {"format"}, lambda c: c.family in YUV, _set(format=RGB)),
    ("format_yuv_plane", {"format"}, reads_rgb, _set(format=NV12)),
    ("mode_against_gray", {"format", "yuv_mode"}, enc, _set(format=GRAY, yuv_mode=1)),
    ("mode_against_yuv", {"format", "yuv_mode"}, enc, _set(format=NV12, yuv_mode=3)),
    ("yuv_mode_5", {"yuv_mode"}, enc, _set(yuv_mode=5)),
    ("method_9", {"method"}, enc, _set(method=9)),
    ("qdelta_max_13", {"qdelta"}, enc, _set(qdelta=13)),
    ("quant_null", {"quant"}, enc, _set(quant=None)),
    ("auto_on_gray", {"format", "yuv_mode"}, enc, _set(format=GRAY, yuv_mode=0)),
    ("sharp_on_gray", {"format", "yuv_mode"}, enc, _set(format=GRAY, yuv_mode=2)),
    ("search_mode_0", {"search"}, enc, _set(search=(0, 0, 0, 1000.0))),
    ("search_nan", {"search"}, enc, _set(search=(0, 0, 1, float("nan")))),
    ("search_mode_0_at_1", {"search"}, enc, _set(search=(1, 1, 0, 1000.0))),
    ("search_nan_at_1", {"search"}, enc, _set(search=(1, 1, 1, float("nan")))),
    ("width_0_at_1", {"dims"}, lambda c: True, _width0),
    ("meta_exif_null", {"meta"}, has("meta"), _set(meta=(0, 0))),
    ("meta_exif_null_at_1", {"meta"}, has("meta"), _set(meta=(1, 1))),
    ("bytes_short", {"bytes"}, shape, _set(bytes_short=True)),
    ("above_cell", {"cell"}, both(sheets, has("sizes")), _set(cell=(8, 8))),
    ("flatten_no_alpha", {"format"}, has("flatten"), _set(format=RGB)),
    ("premultiplied_2", {"flatten"}, has("flatten"), _set(flatten=2)),
    # ... of the newer families' own segments
    ("colour_matrix_2_at_1", {"colour"}, given("colour"), _in("colour", 1, 0, 2)),
    ("colour_reserved_at_1", {"colour"}, given("colour"), _in("colour", 1, 2, 1)),
    ("depth_null", {"depth"}, lambda c: c.family in ("yuv16", "sheet_yuv16"), _set(depth=None)),
    ("depth_bytes_1", {"depth"}, given("depth"), _depth(0, 1)),
    ("depth_shift_9", {"depth"}, given("depth"), _depth(1, 9)),
    ("light_7", {"light"}, takes("light"), _set(light=7)),
    ("unsharp_reserved_at_1", {"unsharp"}, given("unsharp"), _in("unsharp", 1, 2, 1)),
    ("resample_null", {"resample"}, takes("resample"), _set(resample=None)),
    ("resample_filter_9_at_1", {"resample"}, takes("resample"), _in("resample", 1, 0, 9)),
    ("box_null", {"box"}, takes("box"), _set(box=None)),
    ("box_empty_at_1", {"box"}, takes("box"), _in("box", 1, 2, 1.0)),
    ("gap_half_at_1", {"box"}, takes("box"), _in("box", 1, 4, 0.5)),
    ("filter_kind_4_at_1", {"filter"}, given("filter"), _in("filter", 1, 0, 4)),
    # (a radius is read only where there is a kind)
    ("filter_radius_negative_at_0", {"filter"}, both(given("filter"), lambda c: c.filter[0][0] != 0), _in("filter", 0, 3, -1.0)),
    ("compose_reserved_at_1", {"compose"}, given("compose"), _in("compose", 1, 5, 1)),
    ("compose_mode_2_at_1", {"compose"}, given("compose"), _in("compose", 1, 2, 2)),
    ("canvas_4x4_at_1", {"compose"}, given("compose"), _canvas_4x4),
    ("compose_nplaces_9_at_1", {"compose"}, given("compose"), _in("compose", 1, 9, 9)),
    # (overlays and places are checked wherever there is a compose, used or not)
    ("overlays_null", {"overlays"}, both(takes("overlays"), has("compose")), _set(overlays=None)),
    ("overlay_rgba_null", {"overlays"}, both(takes("overlays"), has("compose")), _in("overlays", 0, 0, None)),
    ("overlay_stride_6", {"overlays"}, both(takes("overlays"), has("compose")), _in("overlays", 0, 3, 6)),
    ("places_null", {"places"}, both(takes("places"), has("compose")), _set(places=None)),
    ("place_anchor_5", {"places"}, both(takes("places"), has("compose")), _in("places", 0, 3, 5)),
    ("place_overlay_3", {"places"}, both(takes("places"), has("compose")), _in("places", 0, 0, 3)),
]


def cases(entry):
    """(label, Call) of every recorded case of an entry, in the order of the file"""
    for rlabel, route in routes(entry):
        base = Call(entry)
        for k, v in route.items():
            setattr(base, k, v)
        can = [f for f in FAULTS if f[2](base)]
        plan_bytes = _plan_bytes(base) if base.kind == "shape" else 0
        for group in itertools.chain(((f,) for f in can), itertools.combinations(can, 2)):
            if len(group) == 2 and group[0][1] & group[1][1]:
                continue
            c = Call(entry)
            for k, v in route.items():
                setattr(c, k, [list(x) if isinstance(x, list) else x for x in v] if isinstance(v, list) else v)
            c.overlays, c.places = [list(x) for x in c.overlays], [list(x) for x in c.places]
            c.plan_bytes = plan_bytes
            if hangs_metadata(base):
                c.engine = C.addressof(_a().block)
            for f in group:
                f[3](c)
            yield "%s|%s|%s" % (entry, rlabel, "+".join(f[0] for f in group)), c


# ---- the C arguments: arrays of LONG entries, made once, written before every call
class _Args:
    def __init__(self):
        self.frames = (sj.RaggedFrame * LONG)()
        self.factors = np.ones(LONG, np.uint8)
        self.sizes = np.ones((LONG, 2), np.int32)
        self.orientations = np.ones(LONG, np.uint8)
        self.search = (sj.SearchParams * LONG)()
        self.meta = (sj.Metadata * LONG)()
        self.quant = np.ones((LONG, 2, 64), np.uint8)
        self.out_frames = (sj.RaggedFrame * LONG)()
        self.modes = (C.c_int * LONG)()
        self.q_out = (C.c_float * LONG)()
        self.value_out = (C.c_float * LONG)()
        self.ints = (C.c_int * 2)()
        self.block = C.create_string_buffer(1 << 20)
        self.colour, self.depth, self.unsharp = (video._ColourStruct * LONG)(), video._DepthStruct(), (unsharp._UnsharpStruct * LONG)()
        self.resample, self.box = (resample._ResampleStruct * LONG)(), (resample._BoxStruct * LONG)()
        self.filter, self.compose = (resample._FilterStruct * LONG)(), (resample._ComposeStruct * LONG)()
        self.overlays, self.places = (resample._OverlayStruct * 1)(), (resample._PlaceStruct * 1)()
        for k in range(LONG):
            self.search[k].target_mode, self.search[k].target_value, self.search[k].passes = 1, 1000.0, 3
            self.search[k].tolerance, self.search[k].qmin, self.search[k].qmax = 1.0, 0.0, 100.0


_args = []


def _a():
    if not _args:
        _args.append(_Args())
    return _args[0]


def _frames(c):
    A = _a()
    for k in range(3):
        f = A.frames[k]
        f.width, f.height = c.dims[k]
        for i in range(3):
            f.plane[i] = (1 << 24) + (i << 20) + (k << 16)
            f.row_stride[i] = 1024
        f.out_offset, f.out_capacity = k << 20, 1 << 20
    return A.frames if c.frames else None


# the newer segments: the fields a list stands for, in the order of the struct in the header (`reserved`: its first byte)
def _write(st, fields, row):
    for field, v in zip(fields, row):
        if field == "reserved":
            st.reserved[0] = v
        else:
            setattr(st, field, v)


_FIELDS = {
    "colour": ("matrix", "range", "reserved"), "unsharp": ("amount", "threshold", "reserved"), "resample": ("filter", "reserved"),
    "filter": ("kind", "threshold", "percent", "radius_x", "radius_y", "reserved"),
    "compose": ("canvas_width", "canvas_height", "mode", "px", "py", "reserved", "cx", "cy", "first_place", "nplaces"),
    "overlays": ("rgba", "width", "height", "stride"), "places": ("overlay", "x", "y", "anchor", "reserved"),
}


def _newer_segment(c, name):
    """the C values of one of the newer segments: a value, or a pointer and its per-frame flag or count"""
    A, v = _a(), getattr(c, name)
    if name == "light":
        return [v]
    if name == "depth":
        if v is not None:
            _write(A.depth, ("bytes", "shift", "reserved"), v)
        return [C.addressof(A.depth) if v is not None else None]
    arr = getattr(A, name)
    for k, row in enumerate(v or ()):
        if name == "box":
            arr[k].box[:], arr[k].reducing_gap = row[:4], row[4]
        else:
            _write(arr[k], _FIELDS[name], row)
    # (overlays and places: one of each, counted; the others: one per frame)
    return [C.addressof(arr) if v is not None else None, 1]


def _segment(c, name):
    """the C values of one of the arguments between params (frames, for a shape entry) and the rest"""
    A, v = _a(), getattr(c, name)
    if name == "sheet":
        st = sj._SheetStruct(2, 1, c.cell[0], c.cell[1], 0, 0, (C.c_uint8 * 3)(0, 0, 0), 0)
        c._keep = getattr(c, "_keep", []) + [st]
        return [C.addressof(st) if v else None]
    if name == "flatten":
        fl = sj._FlattenStruct((C.c_uint8 * 3)(255, 255, 255), v or 0, 255.0, 0.0)
        c._keep = getattr(c, "_keep", []) + [fl]
        return [C.addressof(fl) if v is not None else None]
    if name not in ("factors", "sizes", "orientations"):
        return _newer_segment(c, name)
    arr = getattr(A, name)
    if v is not None:
        arr[:3] = v
    return [arr.ctypes.data if v is not None else None]


def _shape_args(c, names=None):
    return [a for name in (names or segments(c)) for a in _segment(c, name)]


def _plan_bytes(c):
    """what the entry's _bytes function says the route's pictures take (before any fault)"""
    symbol = "sjpeg_hip_%s_bytes" % BYTES_FN[c.family]
    return int(getattr(sj.lib(), symbol)(c.format, 3, _frames(c), *_shape_args(c, _binding.SHAPED[symbol][1][1:])))


def invoke(c):
    A, L = _a(), sj.lib()
    head = [c.engine, c.format, c.nframes, _frames(c)]
    mid = _shape_args(c)
    if c.kind == "bytes":
        return getattr(L, c.entry)(*(head[1:] + mid))
    if c.kind == "shape":
        assert c.plan_bytes > 0
        tail = [c.out, c.plan_bytes - 1 if c.bytes_short else 1 << 30, A.out_frames if c.out_frames else None]
        if c.family in SHEETS:
            tail.append(C.cast(A.ints, C.POINTER(C.c_int)) if c.nsheets else None)
        tail += [C.cast(C.byref(A.ints, 4), C.POINTER(C.c_int)) if c.out_format else None, None]
        return getattr(L, c.entry)(*(head + mid + tail))
    prm = sj.RaggedParams(c.yuv_mode, c.method, A.quant.ctypes.data if c.quant else None, 0, None, 0x78, c.qdelta, 1, None, 0)
    if c.search is not None:
        per_frame, k, mode, value = c.search
        for j in range(3):
            A.search[j].target_mode, A.search[j].target_value = 1, 1000.0
        A.search[k].target_mode, A.search[k].target_value = mode, value
        prm.search, prm.search_per_frame = A.search, per_frame
    meta = []
    if c.family != "full":
        for j in range(3):
            A.meta[j].exif, A.meta[j].exif_size = None, 0
        if c.meta is not None and c.meta[1] >= 0:
            A.meta[c.meta[1]].exif_size = 4
        meta = [C.addressof(A.meta) if c.meta is not None else None, c.meta[0] if c.meta is not None else 0]
    d_sizes = (1 << 12) if c.d_sizes else None
    if c.packed:
        out = [c.out, c.capacity, (1 << 13) if c.offsets else None, d_sizes]
    elif c.family in SHEETS:
        out = [c.out, c.out_stride, d_sizes]
    else:
        out = [c.out, d_sizes]
    return getattr(L, c.entry)(*(head + [C.byref(prm) if c.params else None] + mid + meta + out + [A.modes, A.q_out, A.value_out, None]))


def answer(c):
    """(return code, message) of a case, behind a call of a known answer"""
    L = sj.lib()
    assert L.sjpeg_hip_encode_ragged_src(None, 0, 1, 1, None, None, 0, None, None, 1, None, None, None) == -1
    rc = invoke(c)
    assert c.engine in (None, FAKE) or rc == EINVAL, (rc, L.sjpeg_hip_last_error().decode())
    assert (rc == 0) == (c.kind == "bytes"), (rc, L.sjpeg_hip_last_error().decode())     # (refused: a _bytes entry answers 0)
    return [rc, L.sjpeg_hip_last_error().decode()]


def run_lengths(row):
    out = []
    for i in row:
        if out and out[-2] == i:
            out[-1] += 1
        else:
            out += [i, 1]
    return out


def expand(runs):
    return [i for k in range(0, len(runs), 2) for i in [runs[k]] * runs[k + 1]]


def digest(labels):
    return hashlib.sha256("\n".join(labels).encode()).hexdigest()


# ---- how the recording is stored.  An answer is [code, name, text]: the message is names[name] + ": " + texts[text]
# (name -1: the text alone).  A case's number says which answer it got, in two steps.  Its PLACE is 2 + the answer's
# index -- or, for a pair of faults, 0 where that is the answer its first fault got alone on the same route and 1 where
# it is its second fault's.  Its number is 0 where its place is the one the same fault or pair had on the route before
# (the checks of an entry come in one order on nearly all its routes), else 1 + the place.  So the run-length coded row
# of an entry is mostly long runs of 0.
def _place_of(alone, route, pair, i):
    known = [alone.get((route, f)) for f in pair] if len(pair) == 2 else []
    return known.index(i) if i in known else 2 + i


def to_numbers(labels, row):
    alone, before, out = {}, {}, []
    for label, i in zip(labels, row):
        entry, route, faults = label.split("|")
        pair = faults.split("+")
        place = _place_of(alone, route, pair, i)
        out.append(0 if before.get(faults) == place else 1 + place)
        before[faults] = place
        if len(pair) == 1:
            alone[route, faults] = i
    return out


def from_numbers(labels, numbers):
    alone, before, row = {}, {}, []
    for label, k in zip(labels, numbers):
        entry, route, faults = label.split("|")
        pair = faults.split("+")
        place = before[faults] if k == 0 else k - 1
        before[faults] = place
        i = place - 2 if place >= 2 else alone[route, pair[place]]
        if len(pair) == 1:
            alone[route, faults] = i
        row.append(i)
    return row


def recorded_answers(recorded):
    """[[code, message]] of a loaded recording"""
    return [[rc, (recorded["names"][n] + ": " if n >= 0 else "") + recorded["texts"][t]] for rc, n, t in recorded["answers"]]


def main():
    answers, index, per_entry = [], {}, {}
    for entry in ENTRIES:
        row, labels = [], []
        for label, c in cases(entry):
            a = answer(c)
            key = (a[0], a[1])
            if key not in index:
                index[key] = len(answers)
                answers.append(a)
            row.append(index[key])
            labels.append(label)
        assert from_numbers(labels, to_numbers(labels, row)) == row
        per_entry[entry] = {"n": len(row), "labels": digest(labels), "answers": run_lengths(to_numbers(labels, row))}
    names, texts, split = [], [], []
    for rc, msg in answers:
        name, sep, text = msg.partition(": ")
        if not (sep and name.startswith("sjpeg_hip_")):
            name, text = None, msg
        for lst, v in ((names, name), (texts, text)):
            if v is not None and v not in lst:
                lst.append(v)
        split.append([rc, names.index(name) if name is not None else -1, texts.index(text)])
    recorded = {"names": names, "texts": texts, "answers": split, "cases": per_entry}
    assert recorded_answers(recorded) == answers
    with open(OUT, "w") as f:
        f.write('{"names": %s,\n"texts": [\n%s\n],\n' % (json.dumps(names), ",\n".join(json.dumps(t) for t in texts)))
        f.write('"answers": %s,\n"cases": {\n' % json.dumps(split, separators=(",", ":")))
        f.write(",\n".join('"%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in per_entry.items()) + "\n}}\n")
    print("wrote", sum(v["n"] for v in per_entry.values()), "cases,", len(answers), "distinct answers,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
