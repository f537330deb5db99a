"""10-bit video on the host, nothing loaded into python: tests/cxx/yuv16_round_test.cc holds the deep rounding of
sjpeg_amd/csrc/resize_math.h to plain 64-bit division at every rounding boundary; tests/cxx/yuv16_plan_test.cc plans deep
batches with sjpeg_amd/csrc/yuv_resize_plan.cc and walks the bytes the kernel's staging rule reads, every source row in a
buffer of exactly its size; and the two programs that pin the arithmetic and the plan of the 8-bit path still pass as
they are.  Stand-alone programs with their own main, built with the host compiler, under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sjpeg_amd", "csrc")
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _run(tmp_path, name, sources, words):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *SANITIZE, "-w", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           "-I" + HIP_INCLUDE, "-D__HIP_PLATFORM_AMD__", *sources,
                           os.path.join(ROOT, "tests", "cxx", name + ".cc"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0 and words in out.stdout, out.stdout


def test_the_deep_rounding_against_plain_division(tmp_path):
    _run(tmp_path, "yuv16_round_test", [], "yuv16 rounding ok: ")


def test_the_plan_and_the_bytes_the_kernel_reads(tmp_path):
    _run(tmp_path, "yuv16_plan_test", [os.path.join(CSRC, "yuv_resize_plan.cc")], "yuv16 plan ok: 1440 plans")


def test_the_8_bit_arithmetic_and_plan_programs_are_untouched_and_pass(tmp_path):
    """resize_round kept its form and yuv_resize_plan its signature: the two programs build and pass as they are"""
    _run(tmp_path, "resize_math_test", [], "resize math ok: ")
    _run(tmp_path, "yuv_resize_plan_test", [os.path.join(CSRC, "yuv_resize_plan.cc")], "yuv resize plan ok: 640 plans")
