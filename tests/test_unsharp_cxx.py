"""The unsharp mask on the host, nothing loaded into python: tests/cxx/unsharp_math_test.cc holds the header the kernel,
the host and the tests share (sjpeg_amd/csrc/unsharp_math.h) to a 64-bit restatement with a true floor division, to the
identities and to the known answers; tests/cxx/unsharp_plan_test.cc holds the plan of sjpeg_amd/csrc/unsharp_plan.cc to
the made pictures it describes and walks the kernel's rule -- tile, clamped staging, window, store -- over heap buffers
of exactly the pictures' bytes.  Stand-alone programs with their own main, built with the host compiler, under
AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_the_formula_the_identities_and_the_known_answers(tmp_path):
    exe = str(tmp_path / "unsharp_math_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *SANITIZE, "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "sjpeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "unsharp_math_test.cc"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    # 9 amounts x 7 thresholds and the 256 thresholds of amount 0, each over 256 values of p and 4081 of S
    assert out.returncode == 0 and "unsharp math ok: %d samples" % ((9 * 7 + 256) * 256 * 4081) in out.stdout, out.stdout


def test_the_plan_and_the_kernels_rule_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "unsharp_plan_test")
    csrc = os.path.join(ROOT, "sjpeg_amd", "csrc")
    hip_include = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *SANITIZE, "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + hip_include, "-D__HIP_PLATFORM_AMD__", os.path.join(csrc, "unsharp_plan.cc"),
                           os.path.join(ROOT, "tests", "cxx", "unsharp_plan_test.cc"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout
    m = re.search(r"unsharp plan ok: (\d+) samples", out.stdout)
    assert m and int(m.group(1)) > 300000, out.stdout
