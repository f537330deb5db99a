"""The real reference's answers to the calls the live tests make, stored under tests/golden (size and MD5 of every
byte string / array it returned, integers as they are) so that those tests need no reference build: `Replay`
answers every recorded call of oracle.refso.Ref's interface the tests use; `Recorder` wraps the live reference and collects its answers (tests/golden/make_reference_answers.py).

A call is identified by the method name and a digest of its arguments (arrays by dtype, shape and bytes;
numbers exactly), so a test whose inputs change no longer finds its answers and fails until they are recorded
again."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_answers.json")


def call_key(name, args, kwargs):
    h = hashlib.sha1(name.encode())

    def feed(v):
        if isinstance(v, np.ndarray):
            a = np.ascontiguousarray(v)
            h.update(f"a{a.dtype.str}{a.shape}".encode())
            h.update(a.tobytes())
        elif isinstance(v, (bytes, bytearray)):
            h.update(b"y%d:" % len(v) + bytes(v))
        elif isinstance(v, (list, tuple)):
            h.update(b"[%d" % len(v))
            for x in v:
                feed(x)
            h.update(b"]")
        elif isinstance(v, (bool, np.bool_)):
            h.update(b"b%d" % int(v))
        elif isinstance(v, (int, np.integer)):
            h.update(b"i%d" % int(v))
        elif isinstance(v, (float, np.floating)):
            h.update(b"f" + float(v).hex().encode())
        elif v is None:
            h.update(b"n")
        else:
            raise TypeError(f"reference_answers: cannot key an argument of type {type(v).__name__}")

    feed(list(args))
    for k in sorted(kwargs):
        h.update(k.encode())
        feed(kwargs[k])
    return h.hexdigest()


# the Ref methods the tests call, and the two entry points of its .lib they call directly
METHODS = ("encode", "encode_param", "encode_src", "encode_search", "get_block", "fdct", "riskiness", "compress")


def _estimate_quality_key(ptr, chroma):
    return call_key("ref_estimate_quality", (np.frombuffer(C.string_at(ptr, 64), np.uint8), int(chroma)), {})


class Answer:
    """A recorded answer of bytes or an array: its size (dtype and shape) and MD5.  Equal to the bytes / array that
    has them; `(got == answer).all()` works as it does with the array itself."""
    __array_ufunc__ = None                        # (ndarray == Answer defers to Answer.__eq__)

    def __init__(self, rec):
        self.rec = rec

    def __eq__(self, other):
        return np.bool_(describe(other) == self.rec)

    def __ne__(self, other):
        return np.bool_(not self.__eq__(other))

    def __repr__(self):
        return f"<reference answer {self.rec}>"


def describe(v):
    """What is stored of an answer: ints as they are, bytes / arrays by size (dtype, shape) and MD5, a riskiness
    answer (SjpegYUVMode, risk) as the mode and the risk's float.hex()."""
    if v is None:
        return {"kind": "none"}
    if isinstance(v, (bytes, bytearray)):
        return {"kind": "bytes", "size": len(v), "md5": hashlib.md5(bytes(v)).hexdigest()}
    if isinstance(v, np.ndarray):
        a = np.ascontiguousarray(v)
        return {"kind": "array", "dtype": a.dtype.str, "shape": list(a.shape), "md5": hashlib.md5(a.tobytes()).hexdigest()}
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        return {"kind": "int", "value": int(v)}
    if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], (int, np.integer)) and isinstance(v[1], float):
        return {"kind": "riskiness", "mode": int(v[0]), "risk": float(v[1]).hex()}
    return {"kind": "other", "repr": repr(v)}


class _ReplayLib:
    def __init__(self, answers):
        self._answers = answers

    def ref_estimate_quality(self, ptr, chroma):
        return self._answers.get(_estimate_quality_key(ptr, chroma))

    def ref_force_slow_c(self, flag):
        """(the live tests reset the reference's fDCT path after use; the answers were recorded on its default)"""


class Replay:
    def __init__(self, path=PATH):
        with open(path) as f:
            self._answers = json.load(f)
        self.lib = _ReplayLib(self)

    def get(self, key):
        if key not in self._answers:
            raise KeyError("no recorded reference answer for this call: re-record tests/golden/reference_answers.json "
                           "with tests/golden/make_reference_answers.py")
        rec = self._answers[key]
        if rec["kind"] == "none":
            return None
        if rec["kind"] == "int":
            return rec["value"]
        if rec["kind"] == "riskiness":
            return int(rec["mode"]), float.fromhex(rec["risk"])      # (the tuple refso.Ref.riskiness returns)
        return Answer(rec)

    def __getattr__(self, name):
        if name not in METHODS:
            raise AttributeError(name)
        return lambda *args, **kwargs: self.get(call_key(name, args, kwargs))


class _RecordLib:
    def __init__(self, rec):
        self._rec = rec

    def ref_estimate_quality(self, ptr, chroma):
        v = self._rec.ref.lib.ref_estimate_quality(ptr, chroma)
        self._rec.answers[_estimate_quality_key(ptr, chroma)] = describe(v)
        return v

    def ref_force_slow_c(self, flag):
        self._rec.ref.lib.ref_force_slow_c(flag)


class Recorder:
    def __init__(self, ref):
        self.ref = ref
        self.answers = {}
        self.lib = _RecordLib(self)

    def __getattr__(self, name):
        if name not in METHODS:
            raise AttributeError(name)

        def call(*args, **kwargs):
            v = getattr(self.ref, name)(*args, **kwargs)
            self.answers[call_key(name, args, kwargs)] = describe(v)
            return v
        return call

    def save(self, path=PATH):
        with open(path, "w") as f:
            json.dump(self.answers, f, sort_keys=True, separators=(",", ":"))
            f.write("\n")
