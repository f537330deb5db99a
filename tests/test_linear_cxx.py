"""The arithmetic of the resize in linear light on the host: tests/cxx/light_math_test.cc includes the header the kernel
includes (sjpeg_amd/csrc/light_math.h) and checks the table's sum, check values and strict monotony, the inverse against
the counting definition for random sums and at both edges of every midpoint at the areas 1, 2, 7, 65535 and 65535 x
65535, the identity for all 256 bytes, ties going up and the three known answers.  A stand-alone program with its own
main, built with the host compiler, under UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_light_table_and_inverse(tmp_path):
    exe = str(tmp_path / "light_math_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           "-static-libubsan", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "sjpeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "light_math_test.cc"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "light math ok" in out.stdout, out.stdout
    # five areas: 4096 random sums each and up to six sums around each of the 255 midpoints
    n = int(re.search(r"(\d+) inverses", out.stdout).group(1))
    assert 5 * 4096 + 5 * 255 * 4 <= n <= 5 * 4096 + 5 * 255 * 6, out.stdout
