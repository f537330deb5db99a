"""Pillow's filters on the host, nothing loaded into python: tests/cxx/pillow_filter_math_test.cc holds
pillow_filter_math.h's weights to what tests/pillow_filter_model.py computes for a sweep of radii and sigmas, and the
uint32 bound for every r <= 63; tests/cxx/pillow_filter_plan_test.cc holds the plan of
sjpeg_amd/csrc/pillow_filter_plan.cc to its descriptors, its tile counts and every refusal by its words;
tests/cxx/pillow_filter_kernel_emul.cc runs pillow_filter.hip's own source by threads against the closed form.
Stand-alone programs with their own main, built with the host compiler, under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import re
import struct
import subprocess

import numpy as np

import pillow_filter_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sjpeg_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _compile(tmp_path, name, std, sources=(), extra=()):
    exe = str(tmp_path / name)
    hip_include = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    subprocess.check_call(["g++", "-std=" + std, "-O1", "-g", "-ffp-contract=off", *SANITIZE, "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + hip_include, "-I" + os.path.join(ROOT, "tests", "cxx"), "-D__HIP_PLATFORM_AMD__", *extra,
                           *[os.path.join(CSRC, s) for s in sources], os.path.join(ROOT, "tests", "cxx", name + ".cc"), "-o", exe, "-lpthread"])
    return exe


def _weights(path):
    """axes and what the model computes for them, as pillow_filter_math_test.cc reads them"""
    rows = []
    radii = [0.0, 0.3, 2.7, 0.5, 1.0, 5.0, 63.0, 63.9, 1e-4, 1.5, 3.3, 4.0] + [float(v) for v in np.arange(0.0, 63.99, 0.0371)]
    for kind in (pm.BOX, pm.GAUSSIAN, pm.UNSHARP):
        for radius in radii:
            r, ww, fw, passes = pm.axis_weights(pm.BOX if kind == pm.BOX else pm.GAUSSIAN, radius)
            rows.append(struct.pack("<if4I", kind, radius, r, ww, fw, passes))
    with open(path, "wb") as out:
        out.write(struct.pack("<i", len(rows)) + b"".join(rows))
    return len(rows)


def test_the_weights_and_the_bound_under_the_sanitizers(tmp_path):
    n = _weights(str(tmp_path / "weights.bin"))
    exe = _compile(tmp_path, "pillow_filter_math_test", "c++17")
    out = subprocess.run([exe, str(tmp_path / "weights.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0 and "pillow filter math ok: %d axes equal to the model's" % n in out.stdout, out.stdout


def test_the_plan_and_its_refusals_under_the_sanitizers(tmp_path):
    exe = _compile(tmp_path, "pillow_filter_plan_test", "c++17", ["pillow_filter_plan.cc"])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0 and "pillow filter plan ok" in out.stdout, out.stdout


def test_the_filter_kernels_own_source_on_the_cpu(tmp_path):
    """pillow_filter.hip's kernel compiled for the host and run by threads: tests/cxx/pillow_filter_kernel_emul.cc says how"""
    src = open(os.path.join(CSRC, "pillow_filter.hip")).read()
    body = src[:src.index("namespace sjpeg_internal {")]
    assert "pillow_filter_kernel" in body and "hipLaunchKernelGGL" not in body
    body = body.replace("__attribute__((address_space(1)))", "").replace("#include <hip/hip_runtime.h>", "")
    with open(str(tmp_path / "pillow_filter_kernel_body.inc"), "w") as f:
        f.write(body)
    exe = _compile(tmp_path, "pillow_filter_kernel_emul", "c++20", ["pillow_filter_plan.cc"], ["-I" + str(tmp_path), "-I" + CSRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0 and "pillow filter kernel emulation ok" in out.stdout, out.stdout
    assert len(re.findall(r"format \d+: \d+ samples equal", out.stdout)) == 2, out.stdout
