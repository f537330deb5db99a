"""The compose stage on the host, nothing loaded into python: tests/cxx/compose_math_test.cc holds compose_math.h's
blend to its other statement for all 256^3 triples and its sizes and places to what tests/compose_model.py computes in
Python doubles; tests/cxx/compose_plan_test.cc holds the plan of sjpeg_amd/csrc/compose_plan.cc to its descriptors, its
tile counts and every refusal by its words; tests/cxx/compose_kernel_emul.cc runs compose.hip's own source lane by lane
and holds every load and store to an aligned dword inside its row.  Stand-alone programs with their own main, built
with the host compiler, under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import struct
import subprocess

import compose_model as cm

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


def _cases(path):
    """pictures, boxes and centerings, and what the model computes for them, as compose_math_test.cc reads them"""
    rows = []
    shapes = [(3, 2, 5, 5), (2, 3, 6, 5), (5, 5, 6, 1), (1920, 1080, 256, 256), (1000, 1, 10, 10), (4, 2, 8, 4), (1, 1, 1, 1), (65535, 1, 65535, 65535)]
    shapes += [(w, h, bw, bh) for w in (1, 2, 3, 7, 90, 641) for h in (1, 3, 5, 50, 480) for bw in (1, 6, 40, 255) for bh in (1, 5, 40, 256)]
    for w, h, bw, bh in shapes:
        for cx, cy in ((0.5, 0.5), (0.0, 1.0), (0.3, 0.7), (-1.0, 2.0)):
            ow, oh = cm.contain_size(w, h, (bw, bh))
            px, py = cm.pad_place(ow, oh, (bw, bh), (cx, cy)) if ow >= 1 and oh >= 1 else (0, 0)
            rows.append(struct.pack("<4i2d4i", w, h, bw, bh, cx, cy, ow, oh, px, py))
    with open(path, "wb") as out:
        out.write(struct.pack("<i", len(rows)) + b"".join(rows))
    return len(rows)


def test_the_blend_the_sizes_and_the_places_under_the_sanitizers(tmp_path):
    n = _cases(str(tmp_path / "cases.bin"))
    exe = _compile(tmp_path, "compose_math_test", "c++17")
    out = subprocess.run([exe, str(tmp_path / "cases.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0 and "compose math ok: %d sizes and places equal to the model's" % n in out.stdout, out.stdout


def test_the_plan_and_its_refusals_under_the_sanitizers(tmp_path):
    exe = _compile(tmp_path, "compose_plan_test", "c++17", ["compose_plan.cc"])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0 and "compose plan ok" in out.stdout, out.stdout


def test_the_compose_kernels_own_source_on_the_cpu(tmp_path):
    """compose.hip's kernel compiled for the host and run lane by lane: tests/cxx/compose_kernel_emul.cc says how"""
    src = open(os.path.join(CSRC, "compose.hip")).read()
    body = src[:src.index("namespace sjpeg_internal {")]
    assert "compose_kernel" in body and "hipLaunchKernelGGL" not in body
    body = body.replace("__attribute__((address_space(1)))", "").replace("#include <hip/hip_runtime.h>", "")
    with open(str(tmp_path / "compose_kernel_body.inc"), "w") as f:
        f.write(body)
    exe = _compile(tmp_path, "compose_kernel_emul", "c++20", ["compose_plan.cc"], ["-I" + str(tmp_path), "-I" + CSRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0 and "compose kernel emulation ok" in out.stdout, out.stdout
    assert out.stdout.count("aligned dwords inside their rows") == 2, out.stdout
