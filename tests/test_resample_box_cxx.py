"""The box entries on the host, nothing loaded into python: tests/cxx/resample_box_plan_test.cc holds resample_math.h's
decision -- factors, safe box, multipliers, inner box, the refusals -- to what tests/resample_box_model.py decides for
random frames, its reduce and box-aware tables to the pictures Pillow 12.2.0 recorded in
tests/golden/resample_pillow_box.npz, and the plan of sjpeg_amd/csrc/resample_plan.cc to the fixed points, the stages of
a mixed batch and the refusals by their words; tests/cxx/resample_box_kernel_emul.cc runs resample_box.hip's own source
by threads.  Stand-alone programs with their own main, built with the host compiler, under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import re
import struct
import subprocess

import numpy as np

import resample_box_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sjpeg_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
PLAN = [os.path.join(CSRC, name) for name in ("resample_plan.cc", "resize_plan.cc", "yuv_resize_plan.cc")]
CODES = {"box": 1, "gap": 2, "factor": 3, "tall": 4}
RESIZE_BOX, RESIZE_GAP = 1, 2


def _compile(tmp_path, name, std, extra=()):
    exe = str(tmp_path / name)
    hip_include = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    subprocess.check_call(["g++", "-std=" + std, "-O1", "-g", *SANITIZE, "-w", "-I" + os.path.join(ROOT, "include"), "-I" + hip_include,
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-D__HIP_PLATFORM_AMD__", *extra, *PLAN,
                           os.path.join(ROOT, "tests", "cxx", name + ".cc"), "-o", exe, "-lpthread"])
    return exe


def _decisions(path):
    """random frames and what the model decides for them, as resample_box_plan_test.cc reads them"""
    rng = np.random.default_rng(21)
    rows, seen = [], set()
    for k in range(600):
        f, W, H = int(rng.integers(0, 5)), int(rng.integers(1, 500)), int(rng.integers(1, 500))
        w2, h2 = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        if k % 50 == 0:
            W, w2 = 60000, 20
        if k % 50 == 1:
            W, H, h2 = 2, 400, 30
        l, t = (float(rng.uniform(0, W - 0.5)), float(rng.uniform(0, H - 0.5))) if k % 2 else (0.0, 0.0)
        box = [l, t, float(rng.uniform(l + 0.25, W)) if k % 3 else float(W), float(rng.uniform(t + 0.25, H)) if k % 3 else float(H)]
        if k % 40 == 7:
            box[int(rng.integers(0, 4))] += [-1000.0, 1000.0][int(rng.integers(0, 2))]
        gap = [0.0, 1.0, 2.0, 3.0, 1.37, 0.5][int(rng.integers(0, 6 if k % 10 == 0 else 5))]
        code, ints, m, inner = 0, [0] * 8, [0] * 4, [0.0] * 4
        try:
            (fx, fy), safe, (rw, rh), inner = bm.decide(f, W, H, (w2, h2), box, gap if gap != 0 else None)
            ex, ey = safe[2] - safe[0] - (rw - 1) * fx, safe[3] - safe[1] - (rh - 1) * fy
            ints, m = [fx, fy, *safe, rw, rh], [bm.multiplier(n) for n in (fx * fy, ex * fy, fx * ey, ex * ey)]
            seen.add("reduced" if fx > 1 or fy > 1 else "plain")
        except bm.Refused as e:
            code = CODES[e.args[0]]
            seen.add(e.args[0])
        rows.append(struct.pack("<5i4ddi8i4I4d", f, W, H, w2, h2, *box, gap, code, *ints, *m, *inner))
    assert seen == {"reduced", "plain", "box", "gap", "factor", "tall"}, seen
    with open(path, "wb") as out:
        out.write(struct.pack("<i", len(rows)) + b"".join(rows))
    return len(rows)


def _pictures(path):
    """the recorded Image.resize(box=, reducing_gap=) cases of the fixture"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "resample_pillow_box.npz"))
    rows = []
    for k, call in enumerate(g["calls"]):
        if call not in (RESIZE_BOX, RESIZE_GAP):
            continue
        src, want, (f, w2, h2, _), d = g["in_%d" % k], g["out_%d" % k], g["ints"][k], g["doubles"][k]
        c = 1 if src.ndim == 2 else src.shape[2]
        rows.append(struct.pack("<6i5d", f, src.shape[1], src.shape[0], c, w2, h2, *d) + src.tobytes() + want.tobytes())
    with open(path, "wb") as out:
        out.write(struct.pack("<i", len(rows)) + b"".join(rows))
    return len(rows)


def test_the_decision_the_arithmetic_and_the_plan_under_the_sanitizers(tmp_path):
    nd, npic = _decisions(str(tmp_path / "decisions.bin")), _pictures(str(tmp_path / "pictures.bin"))
    assert npic >= 16
    exe = _compile(tmp_path, "resample_box_plan_test", "c++17")
    out = subprocess.run([exe, str(tmp_path / "decisions.bin"), str(tmp_path / "pictures.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=600)
    assert out.returncode == 0 and "resample box plan ok: %d decisions, %d pictures equal to Pillow's" % (nd, npic) in out.stdout, out.stdout


def test_the_box_kernels_own_source_on_the_cpu(tmp_path):
    """resample_box.hip's kernel compiled for the host and run by threads: tests/cxx/resample_box_kernel_emul.cc says how"""
    src = open(os.path.join(CSRC, "resample_box.hip")).read()
    body = src[:src.index("namespace sjpeg_internal {")]
    assert "resample_box_kernel" in body and "hipLaunchKernelGGL" not in body
    body = body.replace("__attribute__((address_space(1)))", "").replace("#include <hip/hip_runtime.h>", "")
    with open(str(tmp_path / "resample_box_kernel_body.inc"), "w") as f:
        f.write(body)
    exe = _compile(tmp_path, "resample_box_kernel_emul", "c++20", ["-I" + str(tmp_path), "-I" + CSRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0 and "resample box kernel emulation ok" in out.stdout, out.stdout
    assert len(re.findall(r"format \d+ flat \d: \d+ samples equal", out.stdout)) == 5, out.stdout
