"""Host-only (no GPU): the binding's table of C argument types (sjpeg_amd/_binding.py) against include/sjpeg_hip.h, and
the layout function of the shaped ragged calls against the header's parameter names.  The header is read here, by a
reader of its own: every sjpeg_hip_* prototype of the C part, its return type and its parameters."""
import ctypes as C
import os
import re

import pytest

import sjpeg_amd as sj
from sjpeg_amd import _binding

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sjpeg_hip.h")
SCALARS = {"int": C.c_int, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int64_t": C.c_int64,
           "float": C.c_float, "double": C.c_double}


def _split(params):
    """the parameters of a prototype, split at the commas outside brackets"""
    out, depth, at = [], 0, 0
    for i, ch in enumerate(params):
        depth += ch in "(["
        depth -= ch in ")]"
        if ch == "," and depth == 0:
            out.append(params[at:i])
            at = i + 1
    return [p.strip() for p in out + [params[at:]]]


def _class(decl):
    """what a declaration (a parameter with its name, or a return type) is to ctypes: "pointer" or a scalar type"""
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in re.findall(r"\w+", decl) if w not in ("const", "unsigned", "struct")]
    return SCALARS[words[0]]


def _prototypes():
    """name -> (return type's class or None for void, [(parameter's class, its name)]) of every sjpeg_hip_* prototype"""
    text = open(HEADER).read().split("namespace sjpeg")[0]
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    found = {}
    for m in re.finditer(r"([\w \t\*]+?)\b(sjpeg_hip_\w+)\s*\(", text):
        depth, end = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[end], 0)
            end += 1
        if not text[end:].lstrip().startswith(";"):
            continue
        ret = m.group(1).strip()
        params = _split(" ".join(text[m.end():end - 1].split()))
        if params == ["void"]:
            params = []
        names = [re.findall(r"\w+", re.sub(r"\[[^\]]*\]", "", p))[-1] for p in params]
        assert m.group(2) not in found, m.group(2)
        found[m.group(2)] = (None if ret == "void" else C.c_char_p if ret == "const char*" else _class(ret),
                             [(_class(p), name) for p, name in zip(params, names)])
    return found


PROTOTYPES = _prototypes()
EXPORTED = [name for name in sj.EXPORTED_C_SYMBOLS if name.startswith("sjpeg_hip_")]
POINTERS = (C._Pointer, C.c_void_p, C.c_char_p)


def _bound_class(t):
    return "pointer" if issubclass(t, POINTERS) else t


def test_the_reader_finds_every_exported_entry():
    assert len(EXPORTED) == len(set(EXPORTED)) == 178
    assert sorted(PROTOTYPES) == sorted(EXPORTED)
    assert _bound_class(C.c_size_t) is _bound_class(C.c_uint64)        # (one class: the same ctypes type here)


def test_every_row_of_the_table_is_an_exported_entry():
    assert sorted(_binding.TABLE) == sorted(sj.EXPORTED_C_SYMBOLS)


@pytest.mark.parametrize("name", EXPORTED)
def test_bound_types_are_the_header_s(name):
    fn = getattr(sj.lib(), name)
    ret, params = PROTOTYPES[name]
    assert fn.argtypes is not None
    assert [_bound_class(t) for t in fn.argtypes] == [c for c, _ in params]
    assert fn.restype is ret or (ret is not None and _bound_class(fn.restype) is _bound_class(ret))
    assert (fn.restype, list(fn.argtypes)) == (_binding.TABLE[name][0], list(_binding.TABLE[name][1]))


# ---- the layout function

@pytest.mark.parametrize("name", sorted(_binding.SHAPED))
def test_layout_puts_every_segment_where_the_header_has_it(name):
    row = _binding.SHAPED[name]
    header_names = [n for _, n in PROTOTYPES[name][1]]
    values = {piece: tuple((piece, k) for k in range(len(_binding.PIECES[piece]))) for piece in row[1]}
    values.update({piece: v[0] for piece, v in values.items() if len(v) == 1})
    args = _binding.layout(row, values)
    assert len(args) == len(getattr(sj.lib(), name).argtypes) == len(header_names)
    assert len(set(args)) == len(args)
    segments = [p for p in row[1] if p not in ("head", "bytes_head", "params", "pictures", "sheets", "unpacked", "packed", "strided")]
    for piece in segments + ["params"] * ("params" in row[1]):
        assert args[header_names.index(piece)] == (piece, 0), piece
        if len(_binding.PIECES[piece]) == 2:         # (its count or per-frame flag stands right behind it)
            assert args[header_names.index(piece) + 1] == (piece, 1), piece
    # the head and the tail by the header's names too
    assert header_names[:3] == (["engine", "format", "nframes"] if "head" in row[1] else ["format", "nframes", "frames"])
    assert args[header_names.index("frames")] == ("head" if "head" in row[1] else "bytes_head", header_names.index("frames"))
    if "head" in row[1]:
        tail = row[1][-1]
        assert header_names[-1] == "stream" and args[-1] == (tail, len(_binding.PIECES[tail]) - 1)


@pytest.mark.parametrize("name", ["sjpeg_hip_encode_ragged_composed_packed_src", "sjpeg_hip_orient_ragged_bytes",
                                  "sjpeg_hip_sheet_ragged_yuv16_src"])
def test_layout_refuses_missing_unknown_and_misshapen_values(name):
    row = _binding.SHAPED[name]
    values = {piece: (0,) * len(_binding.PIECES[piece]) if len(_binding.PIECES[piece]) > 1 else 0 for piece in row[1]}
    assert len(_binding.layout(row, values)) == len(getattr(sj.lib(), name).argtypes)
    with pytest.raises(KeyError, match="missing.*sizes"):
        _binding.layout(row, {k: v for k, v in values.items() if k != "sizes"})
    with pytest.raises(KeyError, match="unknown.*factors"):
        _binding.layout(row, dict(values, factors=0))
    with pytest.raises(ValueError, match="takes"):
        _binding.layout(row, dict(values, **{row[1][0]: (0,)}))
