"""The planning of the contact sheets on the host: sjpeg_amd/csrc/sheet_plan.cc and the two plans it reuses
(resize_plan.cc, yuv_resize_plan.cc) are plain C++ and are built here by the host compiler alone, with
tests/cxx/sheet_plan_test.cc, under AddressSanitizer and UndefinedBehaviorSanitizer.  The program plans batches of
RGB-like, gray and all four YUV-plane formats with every array in a heap buffer of exactly its size and holds each plan
to the placement and the layout sjpeg_hip.h documents; nothing is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_sheet_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "sheet_plan_test")
    csrc = os.path.join(ROOT, "sjpeg_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + HIP_INCLUDE, "-D__HIP_PLATFORM_AMD__",
                           os.path.join(csrc, "sheet_plan.cc"), os.path.join(csrc, "resize_plan.cc"),
                           os.path.join(csrc, "yuv_resize_plan.cc"),
                           os.path.join(ROOT, "tests", "cxx", "sheet_plan_test.cc"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "sheet plan ok: " in out.stdout, out.stdout
    assert int(out.stdout.split("sheet plan ok: ")[1].split()[0]) >= 300, out.stdout
