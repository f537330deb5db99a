"""The planning of the YUV-plane resize on the host: sjpeg_amd/csrc/yuv_resize_plan.cc is plain C++ and is built here by
the host compiler alone, with tests/cxx/yuv_resize_plan_test.cc, under AddressSanitizer and UndefinedBehaviorSanitizer.
The program plans batches of all four formats with every array in a heap buffer of exactly its size and holds each
plan to the layout sjpeg_hip.h documents; nothing is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_yuv_resize_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "yuv_resize_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + HIP_INCLUDE, "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "sjpeg_amd", "csrc", "yuv_resize_plan.cc"),
                           os.path.join(ROOT, "tests", "cxx", "yuv_resize_plan_test.cc"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "yuv resize plan ok: 640 plans" in out.stdout, out.stdout
