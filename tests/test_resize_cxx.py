"""The arithmetic of the ragged resize on the host: tests/cxx/resize_math_test.cc includes the header the kernel
includes (sjpeg_amd/csrc/resize_math.h) and walks the cells of every axis 1..70 -> 1..W and of the longest one, and the
rounding against the plain 64-bit division at both edges of every quotient.  A stand-alone program with its own main,
built with the host compiler, under UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resize_cells_and_rounding(tmp_path):
    exe = str(tmp_path / "resize_math_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           "-static-libubsan", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "sjpeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "resize_math_test.cc"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "resize math ok" in out.stdout, out.stdout
    # every cell of every axis, and 512 sums for each of the 5 + 300 areas: all were visited
    cells = sum(n_dst for n_src in range(1, 71) for n_dst in range(1, n_src + 1)) + 1 + 256 + 65534 + 65535
    assert "%d cells, %d roundings" % (cells, 305 * 512) in out.stdout, out.stdout
