"""Writes tests/golden/ragged_meta.json: what the REFERENCE's sjpeg::Encode() makes of small pictures with every kind of
EncoderParam a ragged batch call describes AND metadata -- methods 0, 4 and 8, SJPEG_YUV_AUTO / 420 / 400, no target, a
PSNR target, size targets.  Runs where the reference is built (oracle/_ref/libsjpeg_ref.so), on the CPU; compiles
tests/cxx/ref_param_meta_shim.cc against it into oracle/_ref/ (out of git).  Each case records the picture's recipe
(oracle/synth.py generator, seed, size), the parameters, a seeded recipe of the metadata bytes, and the size and MD5 of
the reference's output.  tests/test_ragged_meta.py rebuilds pictures and metadata from the recipes (metadata_of below).

Before anything is written, two properties of the reference's outputs are asserted:
  - without a size target, the output with metadata is the output without it with the metadata block spliced in behind
    byte 20 (SOI + APP0);
  - at least three size-target cases are NOT that splice: the search counted the metadata and chose another quality.  A
    search that ignores the metadata cannot give those answers.

    python tests/golden/make_ragged_meta.py
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "ragged_meta.json")

XMP_NOTE = b'xmpNote:HasExtendedXMP="' + b"0" * 32 + b'"'


def metadata_of(recipe):
    """The metadata bytes of a recipe {seed, app, exif, iccp, xmp, xmp_split}: dict(app_markers, exif, iccp, xmp,
    xmp_split_point).  app: payload bytes of one APP3 segment (0: none); exif / iccp: random bytes; xmp: an ASCII packet of
    that length, with the extension note in front when it is longer than one segment takes."""
    rng = np.random.RandomState(int(recipe["seed"]))
    app = b""
    if recipe.get("app", 0):
        n = int(recipe["app"])
        app = b"\xff\xe3" + bytes([(n + 2) >> 8, (n + 2) & 255]) + rng.randint(0, 256, n).astype(np.uint8).tobytes()
    exif = rng.randint(0, 256, int(recipe.get("exif", 0))).astype(np.uint8).tobytes()
    iccp = rng.randint(0, 256, int(recipe.get("iccp", 0))).astype(np.uint8).tobytes()
    n = int(recipe.get("xmp", 0))
    xmp = b""
    if n:
        head = b"<x:xmpmeta " + (XMP_NOTE if n > 65502 else b"") + b">"
        xmp = head + (rng.randint(0, 26, n - len(head)) + 97).astype(np.uint8).tobytes()
    return dict(app_markers=app, exif=exif, iccp=iccp, xmp=xmp, xmp_split_point=int(recipe.get("xmp_split", 0)))


def picture_of(case):
    sys.path.insert(0, ROOT)
    from oracle import synth
    return getattr(synth, case["gen"])(case["w"], case["h"], case["seed"])


def _cases():
    """methods 0 / 4 / 8 x SJPEG_YUV_AUTO (0) / 420 (1) / 400 (4) x no target / PSNR / size, and more size targets"""
    metas = [dict(seed=11, iccp=3000), dict(seed=12, exif=900, xmp=400), dict(seed=13, app=120, iccp=700, exif=64),
             dict(seed=14, xmp=1500), dict(seed=15, exif=2400, app=40)]
    pics = [("g_struct", 96, 64), ("g_noise", 97, 61), ("g_struct", 250, 130), ("g_struct", 64, 64), ("g_noise", 17, 13)]
    cases = []
    k = 0
    for method in (0, 4, 8):
        for yuv in (0, 1, 4):
            for target in ("none", "psnr", "size", "size"):
                gen, w, h = pics[k % len(pics)]
                c = dict(gen=gen, w=w, h=h, seed=4000 + k, quality=75.0, method=method, yuv_mode=yuv, target_mode=0,
                         target_value=0.0, passes=1, tolerance=1.0, qmin=0.0, qmax=100.0, meta=metas[k % len(metas)])
                if target == "psnr":
                    c.update(target_mode=2, target_value=36.0, passes=6)
                elif target == "size":
                    # a few kilobytes above the metadata: what is left for the picture depends on counting it
                    msize = sum(int(c["meta"].get(f, 0)) for f in ("app", "exif", "iccp", "xmp"))
                    c.update(target_mode=1, target_value=float(msize + 1200 + w * h // 8), passes=6)
                cases.append(c)
                k += 1
    # extended XMP (two APP1 kinds) in an unsearched frame
    cases.append(dict(gen="g_struct", w=64, h=64, seed=4100, quality=75.0, method=4, yuv_mode=1, target_mode=0,
                      target_value=0.0, passes=1, tolerance=1.0, qmin=0.0, qmax=100.0, meta=dict(seed=16, xmp=70000)))
    return cases


def _shim():
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    so = os.path.join(ref_dir, "libref_param_meta.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-I" + os.path.join(os.environ.get("REF", "/root/reference"), "src"),
                           os.path.join(ROOT, "tests", "cxx", "ref_param_meta_shim.cc"), "-o", so, "-L" + ref_dir,
                           "-l:libsjpeg_ref.so", "-Wl,-rpath," + ref_dir])
    lib = C.CDLL(so, mode=os.RTLD_LOCAL | os.RTLD_NOW)
    u8p = C.POINTER(C.c_uint8)
    lib.ref_pm_encode.restype = C.c_size_t
    lib.ref_pm_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float] + \
                                 [C.c_char_p, C.c_size_t] * 4 + [C.c_int, C.POINTER(u8p)]
    lib.ref_pm_free.argtypes = [u8p]
    return lib


def _encode(lib, img, c, meta):
    out = C.POINTER(C.c_uint8)()
    method = c["method"]
    n = lib.ref_pm_encode(img.ctypes.data, c["w"], c["h"], 3 * c["w"], c["quality"], c["yuv_mode"],
                          int(method not in (0, 3)), int(method >= 3), int(method >= 7), c["target_mode"],
                          c["target_value"], c["passes"], c["tolerance"], c["qmin"], c["qmax"],
                          meta["app_markers"] or None, len(meta["app_markers"]), meta["exif"] or None, len(meta["exif"]),
                          meta["iccp"] or None, len(meta["iccp"]), meta["xmp"] or None, len(meta["xmp"]),
                          meta["xmp_split_point"], C.byref(out))
    assert n > 0, c
    data = bytes((C.c_ubyte * n).from_address(C.addressof(out.contents)))
    lib.ref_pm_free(out)
    return data


def main():
    lib = _shim()
    none = dict(app_markers=b"", exif=b"", iccp=b"", xmp=b"", xmp_split_point=0)
    cases, not_splice = _cases(), 0
    for c in cases:
        img = np.ascontiguousarray(picture_of(c))
        meta = metadata_of(c["meta"])
        got = _encode(lib, img, c, meta)
        bare = _encode(lib, img, c, none)
        # the metadata block: what a plain encode of the picture gains behind byte 20 (SOI + APP0)
        plain = dict(c, method=0, yuv_mode=1, target_mode=0, passes=1)
        with_meta, without = _encode(lib, img, plain, meta), _encode(lib, img, plain, none)
        block = with_meta[20:20 + len(with_meta) - len(without)]
        assert with_meta == without[:20] + block + without[20:]
        is_splice = got == bare[:20] + block + bare[20:]
        if c["target_mode"] != 1:
            assert is_splice, ("the reference's output with metadata is not the splice", c)
        else:
            c["splice"] = is_splice
            not_splice += 0 if is_splice else 1
        c["size"] = len(got)
        c["md5"] = hashlib.md5(got).hexdigest()
    assert not_splice >= 3, f"only {not_splice} size-target cases tell a search that counts the metadata from one that does not"
    with open(OUT, "w") as f:
        json.dump(dict(comment="made by tests/golden/make_ragged_meta.py from the reference's sjpeg::Encode()", cases=cases), f,
                  indent=1)
    print(f"wrote {OUT}: {len(cases)} cases, {not_splice} size-target cases that are not the splice")


if __name__ == "__main__":
    main()
