"""Records what the entry points answer to pictures whose planes and strides break a rule of their source format --
the return code and the text of sjpeg_hip_last_error() -- for every format value -1..21, in
tests/golden/source_messages.json.  Every call here is one that is refused before any device work, so no GPU is
needed.  tests/test_source_layout_host.py replays the same calls (cases() below) on the current build and wants the
same answers, byte for byte.

The file is made with the library of the commit BEFORE a change to the checks, never with the change itself:

    SJPEG_AMD_LIB=<the parent's libsjpeg_amd.so> python tests/golden/make_source_messages.py

What the calls are made of is stated here on its own (FACTS), not read from the library under test.

How every call is kept a refused one, whatever the build does with the rule under test:
  ragged entries     three frames -- 0 in order, 1 the one under test, 2 of width 0 ("bad dimensions": the frames are
                     checked in turn, so frame 1 has been through all of its checks by then); the stand-in engine
                     pointer of the other *_host.py tests is never read
  uniform entry      sjpeg_hip_scan_histogram_src with 65536 frames, the last thing its checks refuse; they read the
                     engine's pixel transform just before, so a zeroed block stands in for the engine
  engine-less calls  sjpeg_hip_riskiness_sums and sjpeg_hip_sharp_yuv go on to device work when nothing is wrong: only
                     the cases that the rules of include/sjpeg_hip.h refuse are made (must_refuse below)
Before each call a call of a known answer is made, so that an entry point that returns its code without a message of
its own is recorded with that text and not with whatever came before."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import sjpeg_amd as sj  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "source_messages.json")
FORMATS = list(range(-1, 22))
WIDTHS = (16, 17)
H = 16
FAKE = C.c_void_p(1 << 20)
PLANES = (1 << 24, (1 << 24) + (1 << 20), (1 << 24) + (2 << 20))
ROW, FRAME = 1024, 1024 * H


def _cw(w):
    return (w + 1) // 2


# format -> (planes read, element size, one pitch, implied yuv_mode or 0, row bytes of plane i at width w)
FACTS = {
    0: (1, 1, False, 0, lambda i, w: 3 * w), 1: (1, 1, False, 0, lambda i, w: 4 * w), 2: (1, 1, False, 0, lambda i, w: 4 * w),
    3: (1, 1, False, 4, lambda i, w: w), 4: (3, 1, False, 3, lambda i, w: w),
    5: (3, 1, False, 1, lambda i, w: w if i == 0 else _cw(w)), 6: (2, 1, False, 1, lambda i, w: w if i == 0 else 2 * _cw(w)),
    7: (2, 1, False, 1, lambda i, w: w if i == 0 else 2 * _cw(w)),
    8: (3, 1, True, 0, lambda i, w: w), 9: (3, 4, True, 0, lambda i, w: 4 * w), 10: (3, 2, True, 0, lambda i, w: 2 * w),
    11: (3, 2, True, 0, lambda i, w: 2 * w),
    12: (1, 4, False, 0, lambda i, w: 12 * w), 13: (1, 2, False, 0, lambda i, w: 6 * w), 14: (1, 2, False, 0, lambda i, w: 6 * w),
    15: (1, 4, False, 0, lambda i, w: 4 * (4 * w - 1)), 16: (1, 2, False, 0, lambda i, w: 2 * (4 * w - 1)),
    17: (1, 2, False, 0, lambda i, w: 2 * (4 * w - 1)),
    18: (1, 4, False, 4, lambda i, w: 4 * w), 19: (1, 2, False, 4, lambda i, w: 2 * w), 20: (1, 2, False, 4, lambda i, w: 2 * w),
}
UNKNOWN = (1, 1, False, 0, lambda i, w: w)      # (-1 and 21: something to vary all the same)
RGB_BYTES = (0, 1, 2, 8)                        # what the two engine-less calls take


class Picture:
    """one picture's planes and strides; `overflow`: its output range wraps (the ragged encodes check it last)"""

    def __init__(self):
        self.plane, self.row, self.frame, self.overflow = list(PLANES), [ROW] * 3, [FRAME] * 3, False


def variants(fmt, w):
    """(name, Picture, broken): every way a picture of the format is bent; broken: a rule of sjpeg_hip.h is -- the
    planes that are read, the length of their rows, one pitch"""
    nplanes, esz, one_pitch, _, need = FACTS.get(fmt, UNKNOWN)
    yield "base", Picture(), False
    for i in range(3):
        p = Picture()
        p.plane[i] = None
        yield "null%d" % i, p, i < nplanes
        for sign in (1, -1):
            p = Picture()
            p.row[i] = sign * (need(min(i, nplanes - 1), w) - esz)
            yield "short%d%+d" % (i, sign), p, i < nplanes
            # exactly the need (every plane, so that one pitch holds): refused by what comes next
            p = Picture()
            p.row = [sign * need(min(k, nplanes - 1), w) if (k == i or one_pitch) else ROW for k in range(3)]
            p.overflow = True
            yield "exact%d%+d" % (i, sign), p, False
    for i in (1, 2):
        p = Picture()
        p.row[i] += 16
        yield "pitch%d" % i, p, one_pitch
        p = Picture()
        p.frame[i] += 16
        yield "framepitch%d" % i, p, one_pitch
    if esz > 1:
        for i in range(3):
            for what in ("plane", "row", "frame"):
                p = Picture()
                getattr(p, what)[i] += esz // 2
                yield "%s%d_off_element" % (what, i), p, i < nplanes


def _ragged_frames(p, w):
    f = (sj.RaggedFrame * 3)()
    for k in range(3):
        q = p if k == 1 else Picture()
        f[k].width, f[k].height = (0 if k == 2 else w), H
        for i in range(3):
            f[k].plane[i] = q.plane[i]
            f[k].row_stride[i] = q.row[i]
        f[k].out_offset, f[k].out_capacity = (2 ** 64 - 1, 2) if q.overflow else (4096 * k, 4096)
    return f


def _source(fmt, p):
    s = sj.Source()
    s.format = fmt
    for i in range(3):
        s.plane[i] = p.plane[i]
        s.row_stride[i] = p.row[i]
        s.frame_stride[i] = p.frame[i]
    return s


_keep = {}


def _tables():
    if "t" not in _keep:
        _keep["t"] = (sj.ScanTables * 1)(sj.make_tables(quality=75.0)[0])
        _keep["q"] = np.ones((1, 2, 64), np.uint8)
        _keep["engine"] = C.create_string_buffer(1 << 20)
    return _keep


def call_ragged(fmt, mode, p, w):
    return sj.lib().sjpeg_hip_encode_ragged_src(FAKE, fmt, mode, 3, _ragged_frames(p, w), C.cast(_tables()["t"], C.c_void_p), 0, None,
                                                None, 1, C.c_void_p(1 << 16), C.c_void_p(1 << 12), None)


def call_full(fmt, mode, p, w):
    prm = sj.RaggedParams(mode, 4, _tables()["q"].ctypes.data, 0, None, 0x78, 12, 1, None, 0)
    return sj.lib().sjpeg_hip_encode_ragged_full_src(FAKE, fmt, 3, _ragged_frames(p, w), C.byref(prm), 1 << 16, 1 << 12, None, None,
                                                     None, None)


def call_risk_ragged(fmt, mode, p, w):
    return sj.lib().sjpeg_hip_riskiness_ragged_src(FAKE, fmt, 3, _ragged_frames(p, w), None, 1 << 22, None)


def call_histogram(fmt, mode, p, w):
    src = _source(fmt, p)
    return sj.lib().sjpeg_hip_scan_histogram_src(C.cast(_tables()["engine"], C.c_void_p), C.byref(src), w, H, mode, 65536, 1 << 22, None)


def call_risk_sums(fmt, mode, p, w):
    src = _source(fmt, p)
    proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
    return C.cast(sj.lib().sjpeg_hip_riskiness_sums, proto)(C.addressof(src), w, H, 1, 1 << 20, 1 << 21, None)


def call_sharp(fmt, mode, p, w):
    L = sj.lib()
    src = _source(fmt, p)
    L.sjpeg_hip_sharp_workspace.restype = C.c_size_t
    L.sjpeg_hip_sharp_workspace.argtypes = [C.c_int, C.c_int, C.c_int]
    proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                        C.c_void_p, C.c_size_t, C.c_void_p)
    return C.cast(L.sjpeg_hip_sharp_yuv, proto)(C.addressof(src), w, H, 1, 1 << 20, 1 << 21, 1 << 22, 256, 64, 1 << 23,
                                                L.sjpeg_hip_sharp_workspace(w, H, 1), None)


def must_refuse(entry, fmt, name, broken):
    """the engine-less calls: is this case one that sjpeg_hip.h refuses?  (sjpeg_hip_riskiness_sums takes the strides
    of the packed formats on the caller's word: only its planar cases count)"""
    if fmt not in RGB_BYTES or name == "null0":
        return True
    if fmt != 8 and (entry == "risk_sums" or not name.startswith("short0")):
        return False
    return broken


def cases(fmt):
    """(label, call) of every recorded case of a format, in the order of the file"""
    natural = FACTS.get(fmt, UNKNOWN)[3] or sj.YUV_420
    for w in WIDTHS:
        # every yuv_mode value on a picture in order (2: none of the engine's), then every variant at the format's own
        for mode in (sj.YUV_420, sj.YUV_444, sj.YUV_400, 2):
            yield "ragged|m%d|w%d|base" % (mode, w), lambda mode=mode, w=w: call_ragged(fmt, mode, Picture(), w)
            yield "histogram|m%d|w%d|base" % (mode, w), lambda mode=mode, w=w: call_histogram(fmt, mode, Picture(), w)
        for name, p, broken in variants(fmt, w):
            yield "ragged|m%d|w%d|%s" % (natural, w, name), lambda p=p, w=w: call_ragged(fmt, natural, p, w)
            yield "histogram|m%d|w%d|%s" % (natural, w, name), lambda p=p, w=w: call_histogram(fmt, natural, p, w)
            for mode in (sj.YUV_420, sj.YUV_444, sj.YUV_400, sj.YUV_AUTO, sj.YUV_SHARP):
                yield "full|m%d|w%d|%s" % (mode, w, name), lambda p=p, mode=mode, w=w: call_full(fmt, mode, p, w)
            yield "risk_ragged|w%d|%s" % (w, name), lambda p=p, w=w: call_risk_ragged(fmt, 0, p, w)
            if must_refuse("risk_sums", fmt, name, broken):
                yield "risk_sums|w%d|%s" % (w, name), lambda p=p, w=w: call_risk_sums(fmt, 0, p, w)
            if must_refuse("sharp", fmt, name, broken):
                yield "sharp|w%d|%s" % (w, name), lambda p=p, w=w: call_sharp(fmt, 0, p, w)


def answer(call):
    """(return code, message) of a case, behind a call of a known answer"""
    L = sj.lib()
    assert L.sjpeg_hip_encode_ragged_src(None, 0, 1, 1, None, None, 0, None, None, 1, None, None, None) == -1
    rc = call()
    return [rc, L.sjpeg_hip_last_error().decode()]


def main():
    answers, index, per_format = [], {}, {}
    for fmt in FORMATS:
        row = []
        for label, call in cases(fmt):
            a = answer(call)
            assert a[0] != 0, (fmt, label)
            key = (a[0], a[1])
            if key not in index:
                index[key] = len(answers)
                answers.append(a)
            row.append(index[key])
        per_format[str(fmt)] = row
    with open(OUT, "w") as f:
        f.write('{"answers": [\n' + ",\n".join(json.dumps(a) for a in answers) + '\n],\n"cases": {\n')
        f.write(",\n".join('"%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in per_format.items()) + "\n}}\n")
    print("wrote", sum(len(v) for v in per_format.values()), "cases,", len(answers), "distinct answers,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
