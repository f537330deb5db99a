"""The rounding of the ragged reduction on the host: tests/cxx/reduce_round_test.cc includes the header the kernel
includes (sjpeg_amd/csrc/reduce_round.h) and walks every factor 1..8 and every sum in 0..255 s^2 against
(sum + s^2 / 2) / s^2.  A stand-alone program with its own main, built with the host compiler, under
UndefinedBehaviorSanitizer (an overflowing product would show)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reduce_rounding_for_every_factor_and_sum(tmp_path):
    exe = str(tmp_path / "reduce_round_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           "-static-libubsan", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "sjpeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "reduce_round_test.cc"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "reduce rounding ok" in out.stdout, out.stdout
    # 1 + sum over s of 255 s^2 sums: every one was visited
    assert "%d sums" % sum(255 * s * s + 1 for s in range(1, 9)) in out.stdout, out.stdout
