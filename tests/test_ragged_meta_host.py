"""Per-picture metadata in ragged batches, the part that needs no GPU: the symbols and their prototypes, and
sjpeg_hip_metadata_size against the header builders for every kind of metadata and every refusal of the reference
(src/headers.cc:72-180)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sjpeg_amd as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sjpeg_hip_metadata_size", "sjpeg_hip_encode_ragged_full_meta_src", "sjpeg_hip_encode_ragged_full_meta_packed_src")
NOTE = b'xmpNote:HasExtendedXMP="' + b"0" * 32 + b'"'


def _err():
    return sj.lib().sjpeg_hip_last_error().decode()


def _bytes(n, seed=1):
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8).tobytes()


def _xmp(n, note=True):
    head = b"<x:xmpmeta " + (NOTE if note else b"") + b">"
    return head + b"a" * (n - len(head))


def test_symbols_and_prototypes():
    text = open(os.path.join(ROOT, "include", "sjpeg_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in sj.EXPORTED_C_SYMBOLS
        fn = getattr(sj.lib(), name)
        assert fn.restype is C.c_int and fn.argtypes is not None
    full = list(sj.lib().sjpeg_hip_encode_ragged_full_src.argtypes)
    assert list(sj.lib().sjpeg_hip_encode_ragged_full_meta_src.argtypes) == full[:5] + [C.c_void_p, C.c_int] + full[5:]
    packed = list(sj.lib().sjpeg_hip_encode_ragged_full_packed_src.argtypes)
    assert list(sj.lib().sjpeg_hip_encode_ragged_full_meta_packed_src.argtypes) == packed[:5] + [C.c_void_p, C.c_int] + packed[5:]
    assert sj.lib().sjpeg_hip_abi_version() == 18
    assert "No per-picture metadata" not in text


CASES = {
    "none": dict(),
    "app": dict(app_markers=b"\xff\xe3\x00\x0a" + _bytes(8)),
    "exif": dict(exif=_bytes(900, 2)),
    "exif_largest": dict(exif=_bytes(65527, 3)),
    "iccp": dict(iccp=_bytes(3000, 4)),
    "iccp_two_chunks": dict(iccp=_bytes(70000, 5)),
    "xmp": dict(xmp=_xmp(400, note=False)),
    "xmp_65502": dict(xmp=_xmp(65502)),
    "xmp_65503": dict(xmp=_xmp(65503)),
    "xmp_200000": dict(xmp=_xmp(200000)),
    "xmp_split": dict(xmp=_xmp(90000), xmp_split_point=4000),
    "all": dict(app_markers=b"\xff\xe3\x00\x0a" + _bytes(8), exif=_bytes(64, 6), iccp=_bytes(700, 7), xmp=_xmp(1500, note=False)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_size_is_what_the_header_builder_inserts(name):
    kw = CASES[name]
    quant = np.full((2, 64), 16, np.uint8)
    with_meta = sj.make_header_meta(96, 64, sj.YUV_420, quant, None, **kw)
    bare = sj.make_header_ex(96, 64, sj.YUV_420, quant, None)
    assert with_meta is not None
    assert sj.PictureMetadata(**kw).size() == len(with_meta) - len(bare)
    # ... and the bytes are the bare header's with the block behind SOI + APP0
    n = len(with_meta) - len(bare)
    assert with_meta == bare[:20] + with_meta[20:20 + n] + bare[20:]


def test_null_metadata_has_size_zero():
    n = C.c_size_t(7)
    assert sj.lib().sjpeg_hip_metadata_size(None, C.byref(n)) == 0 and n.value == 0
    assert sj.PictureMetadata().size() == 0


INVALID = {
    "exif_65528": (dict(exif=_bytes(65528)), "exif"),
    "iccp_256_chunks": (dict(iccp=b"\x01" * (255 * 65519 + 1)), "iccp"),
    "xmp_no_note": (dict(xmp=_xmp(65505, note=False)), "xmp"),     # (65504 bytes still fit one APP1 segment)
    "xmp_note_behind_split": (dict(xmp=_xmp(70000), xmp_split_point=40), "xmp"),
    "xmp_note_unterminated": (dict(xmp=b"<x:xmpmeta " + NOTE[:-1] + b"'>" + b"a" * 70000), "xmp"),
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_metadata_is_refused_with_its_field(name):
    kw, field = INVALID[name]
    quant = np.full((2, 64), 16, np.uint8)
    assert sj.make_header_meta(16, 16, sj.YUV_420, quant, None, **kw) is None      # (the header builder refuses it too)
    m = sj.PictureMetadata(**kw)._struct()
    n = C.c_size_t(7)
    assert sj.lib().sjpeg_hip_metadata_size(C.byref(m), C.byref(n)) == -1          # SJPEG_HIP_EINVAL
    assert n.value == 0
    assert _err().startswith("sjpeg_hip_metadata_size: " + field + ":"), _err()


@pytest.mark.parametrize("field", ["app_markers", "exif", "iccp", "xmp"])
def test_null_pointer_with_a_size_is_refused(field):
    m = sj.Metadata()
    setattr(m, field + "_size", 5)
    n = C.c_size_t(7)
    assert sj.lib().sjpeg_hip_metadata_size(C.byref(m), C.byref(n)) == -1
    assert _err().startswith("sjpeg_hip_metadata_size: " + field + ":"), _err()
    assert sj.lib().sjpeg_hip_metadata_size(C.byref(m), None) == -1


def test_meta_calls_check_their_arguments_before_the_engine():
    lib = sj.lib()
    m = sj.PictureMetadata(exif=b"x")._struct()
    rc = lib.sjpeg_hip_encode_ragged_full_meta_src(None, sj.SRC_RGB, 1, None, None, C.cast(C.byref(m), C.c_void_p), 0, None, None,
                                                   None, None, None, None)
    assert rc == -1 and "sjpeg_hip_encode_ragged_full_meta_src: engine == NULL" in _err()
    rc = lib.sjpeg_hip_encode_ragged_full_meta_packed_src(None, sj.SRC_RGB, 1, None, None, C.cast(C.byref(m), C.c_void_p), 0, None, 0,
                                                          None, None, None, None, None, None)
    assert rc == -1 and "sjpeg_hip_encode_ragged_full_meta_packed_src: engine == NULL" in _err()
    # meta == NULL is the call without metadata: its message
    rc = lib.sjpeg_hip_encode_ragged_full_meta_src(None, sj.SRC_RGB, 1, None, None, None, 0, None, None, None, None, None, None)
    assert rc == -1 and "sjpeg_hip_encode_ragged_full_src: engine == NULL" in _err()


def test_python_metadata_arguments():
    import inspect
    for fn in (sj.encode_images, sj.compress_images, sj.Engine.encode_ragged_full, sj.Engine.encode_ragged_full_packed):
        assert inspect.signature(fn).parameters["metadata"].default is None, fn.__name__
    assert list(inspect.signature(sj.PictureMetadata).parameters) == ["app_markers", "exif", "iccp", "xmp", "xmp_split_point"]
    with pytest.raises(sj.SjpegError, match="one metadata entry per image"):
        sj._metadata_args("encode_images", 2, [sj.PictureMetadata()])
    with pytest.raises(sj.SjpegError, match="metadata entry 1: .*exif"):
        sj._metadata_args("encode_images", 2, [None, sj.PictureMetadata(exif=b"\0" * 65530)])
    arr, per_frame, sizes, _ = sj._metadata_args("encode_images", 3, sj.PictureMetadata(exif=b"abcd"))
    assert per_frame == 0 and len(arr) == 1 and sizes == [4 + 10] * 3
