"""The eight orientations on the host: tests/cxx/orient_math_test.cc includes the header the kernel and the planner
include (sjpeg_amd/csrc/orient_math.h) and walks every orientation over every picture of 1..9 x 1..9 and the two longest
ones -- a bijection, inverted by the inverse function, equal to the table written out a second time.  A stand-alone
program with its own main, built with the host compiler, under UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_orientations_are_bijections_and_equal_the_table(tmp_path):
    exe = str(tmp_path / "orient_math_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           "-static-libubsan", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "sjpeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "orient_math_test.cc"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "orient math ok" in out.stdout, out.stdout
    samples = 8 * (sum(w * h for w in range(1, 10) for h in range(1, 10)) + 2 * 65535)
    assert "%d samples" % samples in out.stdout, out.stdout
