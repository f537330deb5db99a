"""Resampling with Pillow's filters on the host, nothing loaded into python: tests/cxx/resample_math_test.cc holds the
header the kernel, the host and the tests share (sjpeg_amd/csrc/resample_math.h) and sjpeg_hip_resample_table to the
tables recorded in tests/golden/resample_pillow.npz, to the two bounds over the grid sjpeg_hip.h names and to the known
answers; tests/cxx/resample_plan_test.cc holds the plan of sjpeg_amd/csrc/resample_plan.cc -- ksize, sizes, layout,
bytes, tables shared per key, the refusals -- and walks the kernel's rule over heap buffers of exactly the pictures'
bytes.  Stand-alone programs with their own main, built with the host compiler, under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sjpeg_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
# the plan, and the two files its checks of a flatten and its format names come from
PLAN = [os.path.join(CSRC, name) for name in ("resample_plan.cc", "resize_plan.cc", "yuv_resize_plan.cc")]


def _build(tmp_path, name):
    exe = str(tmp_path / name)
    hip_include = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *SANITIZE, "-w", "-I" + os.path.join(ROOT, "include"), "-I" + hip_include,
                           "-D__HIP_PLATFORM_AMD__", *PLAN, os.path.join(ROOT, "tests", "cxx", name + ".cc"), "-o", exe])
    return exe


def test_the_recorded_tables_the_bounds_and_the_known_answers(tmp_path):
    d = np.load(os.path.join(ROOT, "tests", "golden", "resample_pillow.npz"))
    path = str(tmp_path / "tables.bin")
    with open(path, "wb") as f:
        for k, (filt, n_in, n_out) in enumerate(d["tables"]):
            bounds, K = d["bounds_%d" % k], d["K_%d" % k]
            assert bounds.shape == (n_out, 2) and K.shape[0] == n_out and bounds.dtype == np.int32 and K.dtype == np.int32
            np.array([filt, n_in, n_out, K.shape[1]], np.int32).tofile(f)
            bounds.tofile(f)
            K.tofile(f)
    out = subprocess.run([_build(tmp_path, "resample_math_test"), path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0 and "resample math ok: %d recorded tables" % len(d["tables"]) in out.stdout, out.stdout
    assert "grid: %d tables, max |K| 5392348, max sum 1377229532" % (5 * 74 * 74) in out.stdout, out.stdout


def test_the_plan_and_the_kernels_rule_under_the_sanitizers(tmp_path):
    out = subprocess.run([_build(tmp_path, "resample_plan_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout
    m = re.search(r"resample plan ok: (\d+) samples", out.stdout)
    assert m and int(m.group(1)) > 90000, out.stdout


def test_the_kernels_own_source_on_the_cpu(tmp_path):
    """resample.hip's kernel compiled for the host and run by threads: tests/cxx/resample_kernel_emul.cc says how"""
    src = open(os.path.join(CSRC, "resample.hip")).read()
    body = src[:src.index("namespace sjpeg_internal {")]
    assert "resample_kernel" in body and "hipLaunchKernelGGL" not in body
    body = body.replace("__attribute__((address_space(1)))", "").replace("#include <hip/hip_runtime.h>", "")
    with open(str(tmp_path / "resample_kernel_body.inc"), "w") as f:
        f.write(body)
    exe = str(tmp_path / "resample_kernel_emul")
    hip_include = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", *SANITIZE, "-w", "-I" + os.path.join(ROOT, "include"), "-I" + hip_include,
                           "-I" + str(tmp_path), "-I" + CSRC, "-D__HIP_PLATFORM_AMD__", *PLAN, os.path.join(ROOT, "tests", "cxx", "resample_kernel_emul.cc"),
                           "-o", exe, "-lpthread"])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0 and "resample kernel emulation ok" in out.stdout, out.stdout
    assert len(re.findall(r"format \d+: \d+ samples equal", out.stdout)) == 3, out.stdout
