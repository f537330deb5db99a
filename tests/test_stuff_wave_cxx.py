"""The lane's part of stuff_chunks_wave on the host, nothing loaded into python: tests/cxx/stuff_wave_emul.cc runs
sjpeg_amd/csrc/stuff_wave_body.h -- the kernel's own source -- for the 64 lanes of a wave in both orders and holds every
store to the kernel's invariant: every byte of the body written exactly once, none outside it, the output the plain
stitch's.  Its streams are every stream of tests/stitch_cases.py that the band route uses (written to a file here) and the
program's own exhaustive and designed ones.  A stand-alone program with its own main, built with the host compiler, under AddressSanitizer and
UndefinedBehaviorSanitizer (the stream lies in a heap buffer of exactly the words the kernel may read)."""
import os
import struct
import subprocess

import stitch_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sjpeg_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _padded(case):
    """the un-stuffed bytes of a band case, the last byte padded with 1-bits"""
    raw = bytearray(case._raw.tobytes())
    raw[-1] |= (1 << (8 * len(raw) - case.total_bits)) - 1
    return bytes(raw)


def _streams(path):
    cases = list(sc.band_cases()) + [sc.big_band_case()]
    with open(path, "wb") as out:
        out.write(struct.pack("<I", len(cases)))
        for c in cases:
            raw, name = _padded(c), c.name.encode()
            out.write(struct.pack("<IIQ", len(name), len(c.header), len(raw)) + name + raw)
    return len(cases)


def test_the_wave_stuffing_kernels_own_source_on_the_cpu(tmp_path):
    n = _streams(str(tmp_path / "streams.bin"))
    exe = str(tmp_path / "stuff_wave_emul")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-w", *SANITIZE, "-I" + CSRC, os.path.join(ROOT, "tests", "cxx", "stuff_wave_emul.cc"),
                           "-o", exe])
    out = subprocess.run([exe, str(tmp_path / "streams.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0 and "stuff wave emulation ok" in out.stdout, out.stdout
    assert "(%d of the band route)" % n in out.stdout, out.stdout
