"""The EXIF Orientation reader and its reset on the host: sjpeg_amd/csrc/exif_orientation.cc is plain C++ and is built
here by the host compiler alone, with tests/cxx/exif_orientation_test.cc, under AddressSanitizer and
UndefinedBehaviorSanitizer.  The program takes every payload of tests/golden/exif_orientation.json, every truncation of
each and every single-byte change of the first 64 bytes, each in a heap buffer of exactly its size: the answer is in
0..8 and nothing is read out of bounds."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exif_orientation_reads_inside_the_payload(tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "exif_orientation.json")) as f:
        cases = json.load(f)["cases"]
    listing = tmp_path / "payloads.txt"
    listing.write_text("".join("%d %s %s\n" % (c["orientation"], c["hex"] or "-", c["reset_hex"] or "-") for c in cases))
    exe = str(tmp_path / "exif_orientation_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "sjpeg_amd", "csrc", "exif_orientation.cc"),
                           os.path.join(ROOT, "tests", "cxx", "exif_orientation_test.cc"), "-o", exe])
    out = subprocess.run([exe, str(listing)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "exif orientation ok" in out.stdout, out.stdout
    variants = sum(len(c["hex"]) // 2 + 256 * min(64, len(c["hex"]) // 2) for c in cases)
    assert "%d payloads, %d variants" % (len(cases), variants) in out.stdout, out.stdout
