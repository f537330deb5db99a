"""The host code behind per-picture metadata that needs no device -- the metadata checks and sizes, the header assembly
(sjpeg_amd/csrc/jpeg_host.cc) -- under AddressSanitizer and UndefinedBehaviorSanitizer: tests/cxx/metadata_host_test.cc,
a stand-alone program with its own main, built with the host compiler and run on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_metadata_host_code_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "metadata_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",      # (the runtimes inside the program)
                           "-ffp-contract=off", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "sjpeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "metadata_host_test.cc"),
                           os.path.join(ROOT, "sjpeg_amd", "csrc", "jpeg_host.cc"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "metadata host checks ok" in out.stdout, out.stdout
