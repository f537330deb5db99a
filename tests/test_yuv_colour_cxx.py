"""The video colour conversion on the host, nothing loaded into python: tests/cxx/yuv_colour_math_test.cc holds the
header the kernel, the host and the tests' model share (sjpeg_amd/csrc/yuv_colour_math.h) to a 64-bit floor division over
all 2^24 triples of each source; tests/cxx/yuv_colour_plan_test.cc holds the plan of sjpeg_amd/csrc/yuv_colour_plan.cc to
the planes it describes and walks what the kernel's lanes touch.  Stand-alone programs with their own main, built with
the host compiler, under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_the_formula_over_every_triple(tmp_path):
    exe = str(tmp_path / "yuv_colour_math_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *SANITIZE, "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "sjpeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "yuv_colour_math_test.cc"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0 and "yuv colour math ok: %d triples" % (4 << 24) in out.stdout, out.stdout


def test_the_plans_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "yuv_colour_plan_test")
    csrc = os.path.join(ROOT, "sjpeg_amd", "csrc")
    hip_include = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *SANITIZE, "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + hip_include, "-D__HIP_PLATFORM_AMD__",
                           os.path.join(csrc, "sheet_plan.cc"), os.path.join(csrc, "resize_plan.cc"),
                           os.path.join(csrc, "yuv_resize_plan.cc"), os.path.join(csrc, "yuv_colour_plan.cc"),
                           os.path.join(ROOT, "tests", "cxx", "yuv_colour_plan_test.cc"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0 and "yuv colour plan ok: 720 plans" in out.stdout, out.stdout
