"""The arithmetic of alpha flattening on the host: tests/cxx/flatten_math_test.cc includes the header the kernel and the
tests' model share (sjpeg_amd/csrc/flatten_math.h) and holds both formulas, over all 2^24 triples (alpha, sample,
background), and the division-free / 255, over 0..65535, to the plain 64-bit division; then the end values.  A
stand-alone program with its own main, built with the host compiler, under UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flatten_formulas_over_every_triple(tmp_path):
    exe = str(tmp_path / "flatten_math_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           "-static-libubsan", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "sjpeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "flatten_math_test.cc"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "flatten math ok" in out.stdout, out.stdout
    assert "%d quotients, %d triples" % (65536, 1 << 24) in out.stdout, out.stdout


def test_flat_plans_under_the_sanitizers(tmp_path):
    """the flatten in resize_plan.cc and sheet_plan.cc (tests/cxx/flatten_plan_test.cc): a flat plan is the plan of the
    same frames as RGB pictures, every refusal names what it refuses -- under AddressSanitizer and
    UndefinedBehaviorSanitizer, every array in a heap buffer of exactly its size"""
    exe = str(tmp_path / "flatten_plan_test")
    csrc = os.path.join(ROOT, "sjpeg_amd", "csrc")
    hip_include = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + hip_include, "-D__HIP_PLATFORM_AMD__",
                           os.path.join(csrc, "sheet_plan.cc"), os.path.join(csrc, "resize_plan.cc"),
                           os.path.join(csrc, "yuv_resize_plan.cc"),
                           os.path.join(ROOT, "tests", "cxx", "flatten_plan_test.cc"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "flatten plan ok: 1200 plans, 16 formats refused by name" in out.stdout, out.stdout
