"""Records what the shaped ragged entries of the C layer answer to calls they refuse on the host -- the return code and
the text of sjpeg_hip_last_error() -- in tests/golden/c_messages.json: the four _full[_meta][_packed]_src entries, the
_reduced, _resized, _oriented, _flattened, _yuv_resized, _sheet and _sheet_flat encode entries with their _packed twins
and the seven shape entries (sjpeg_hip_reduce_ragged_src ... sjpeg_hip_sheet_ragged_flat_src), 25 in all.  Every call is
one that is refused before the engine is read, so no GPU is needed and the stand-in engine pointer of the other
*_host.py tests is never followed.  tests/test_c_messages_host.py replays the same calls (cases() below) on the current
build and wants the same answers, byte for byte.

The file is made with the library of the commit BEFORE a change to these entries, never with the change itself:

    SJPEG_AMD_LIB=<the parent's libsjpeg_amd.so> python tests/golden/make_c_messages.py

What is recorded, per entry:
  routes   every combination of the arguments that decide which body a call takes, and with it whose name a message
           carries: factors NULL / all 1 / one 2; sizes NULL / every frame's own / one smaller; orientations NULL / all
           1 / one 6; flatten NULL / given; meta NULL / given (one entry per frame).  Where an entry refuses a NULL
           (the shape entries' factors, sizes and flatten) that NULL is a fault, not a route.
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
}
ENTRIES = {}
for _fam, (_stem, _shape, _, _) in FAMILIES.items():
    ENTRIES["sjpeg_hip_encode_ragged_%s_src" % _stem] = ("encode", _fam, False)
    ENTRIES["sjpeg_hip_encode_ragged_%s_packed_src" % _stem] = ("encode", _fam, True)
    if _shape is not None:
        ENTRIES[_shape] = ("shape", _fam, False)
assert len(ENTRIES) == 25
BYTES_FN = {"reduce": "reduce", "resize": "resize", "orient": "orient", "flatten": "orient", "yuv": "resize_ragged_yuv",
            "sheet": "sheet", "sheet_flat": "sheet"}


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


def routes(entry):
    """(label, {argument: value}) of every route of an entry"""
    kind, family, _ = ENTRIES[entry]
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
    return c.meta is not None and (c.family == "full_meta" or passes_through(c))


def passes_through(c):
    """does the call, as its route stands, go to the entry of fewer arguments without reading its pictures?"""
    if c.kind == "shape" or c.family in ("full", "full_meta", "sheet", "sheet_flat") or c.flatten is not None:
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


enc = lambda c: c.kind == "encode"
shape = lambda c: c.kind == "shape"
has = lambda name: (lambda c: getattr(c, name) is not None)
sheets = lambda c: c.family in ("sheet", "sheet_flat")
takes = lambda name: (lambda c: name in FAMILIES[c.family][2])
both = lambda *fs: (lambda c: all(f(c) for f in fs))
FAULTS = [
    ("engine_null", {"engine"}, lambda c: True, _set(engine=None)),
    ("params_null", {"params"}, enc, _set(params=None)),
    ("frames_null", {"frames"}, lambda c: True, _set(frames=None)),
    ("sheet_null", {"sheet"}, sheets, _set(sheet=None)),
    ("flatten_null", {"flatten"}, both(shape, takes("flatten")), _set(flatten=None)),
    ("factors_null", {"factors"}, both(shape, takes("factors")), _set(factors=None)),
    ("sizes_null", {"sizes"}, both(shape, lambda c: c.family == "resize"), _set(sizes=None)),
    ("d_offsets_null", {"offsets"}, lambda c: c.packed, _set(offsets=None)),
    ("out_null", {"out"}, lambda c: True, _set(out=None)),
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
    ("format_not_yuv", {"format"}, lambda c: c.family == "yuv", _set(format=RGB)),
    ("format_yuv_plane", {"format"}, lambda c: c.family in ("reduce", "resize", "orient", "flatten") and not passes_through(c),
     _set(format=NV12)),
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


def _shape_args(c):
    """the arguments between params (frames, for a shape entry) and the rest"""
    A = _a()
    out = []
    for name in FAMILIES[c.family][2]:
        v = getattr(c, name)
        if name == "sheet":
            st = sj._SheetStruct(2, 1, c.cell[0], c.cell[1], 0, 0, (C.c_uint8 * 3)(0, 0, 0), 0)
            c._keep = getattr(c, "_keep", []) + [st]
            out.append(C.addressof(st) if v else None)
        elif name == "flatten":
            fl = sj._FlattenStruct((C.c_uint8 * 3)(255, 255, 255), v or 0, 255.0, 0.0)
            c._keep = getattr(c, "_keep", []) + [fl]
            out.append(C.addressof(fl) if v is not None else None)
        else:
            arr = getattr(A, name)
            if v is not None:
                arr[:3] = v
            out.append(arr.ctypes.data if v is not None else None)
    return out


def _plan_bytes(c):
    """what the entry's _bytes function says the route's pictures take (before any fault)"""
    L = sj.lib()
    fn = getattr(L, "sjpeg_hip_%s_ragged_bytes" % BYTES_FN[c.family]) if c.family != "yuv" else L.sjpeg_hip_resize_ragged_yuv_bytes
    rest = [a for n, a in zip(FAMILIES[c.family][2], _shape_args(c)) if n != "flatten"]
    return int(fn(c.format, 3, _frames(c), *rest))


def invoke(c):
    A, L = _a(), sj.lib()
    head = [c.engine, c.format, c.nframes, _frames(c)]
    mid = _shape_args(c)
    if c.kind == "shape":
        assert c.plan_bytes > 0
        tail = [c.out, c.plan_bytes - 1 if c.bytes_short else 1 << 30, A.out_frames if c.out_frames else None]
        if c.family in ("sheet", "sheet_flat"):
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
    elif c.family in ("sheet", "sheet_flat"):
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
            assert a[0] != 0, label
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
