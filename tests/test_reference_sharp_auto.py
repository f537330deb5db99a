"""The product against the real reference's recorded answers (tests/golden/reference_answers.json) -- not against the
oracle -- for SJPEG_YUV_SHARP, SjpegRiskiness, SJPEG_YUV_AUTO, SjpegCompress and the searches with sharp and auto
sampling: the pictures of tests/sharp_auto_cases.py, which tests/test_oracle.py walks with the oracle, one per call
through the host API, in ragged calls, through the other source layouts and reduced.  Every comparison is exact (bytes;
the verdict and the float risk).  A test collects every picture that differs and fails with the whole list."""
import os

import numpy as np
import pytest
import torch

import sjpeg_amd as sj
import sharp_auto_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def risk_table():
    with open(os.path.join(sj.CSRC, "riskiness.bin"), "rb") as f:
        tab = f.read()
    assert len(tab) == 117649
    sj.set_riskiness_table(tab)
    return tab


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


def _dev(img):
    return torch.from_numpy(np.array(img)).cuda()


def _none(failures):
    assert not failures, (len(failures), failures[:20])


# ---- a. one picture per call: the host API

def _one_per_call(reference, pictures, calls):
    failures, n = [], 0
    for p in pictures:
        if "sharp" in calls and not sj.SjpegEncode(p.img, p.q, p.method, sj.YUV_SHARP) == cases.ref_sharp(reference, p):
            failures.append(("sharp", cases.what(p)))
        if "riskiness" in calls:
            got, want = sj.SjpegRiskiness(p.img), cases.ref_riskiness(reference, p)
            if got != want:
                failures.append(("riskiness", cases.what(p), got, want))
        if "auto" in calls and not sj.SjpegEncode(p.img, p.q, p.method, sj.YUV_AUTO) == cases.ref_auto(reference, p):
            failures.append(("auto", cases.what(p)))
        if "compress" in calls and not sj.SjpegCompress(p.img, 75.0) == cases.ref_compress(reference, p):
            failures.append(("compress", cases.what(p)))
        n += 1
    _none(failures)
    return n


@pytest.mark.parametrize("kind", cases.KINDS)
def test_one_picture_per_call(reference, risk_table, kind):
    n = _one_per_call(reference, [p for p in cases.pictures() if p.kind == kind], ("sharp", "riskiness", "auto", "compress"))
    assert n >= 30                               # (the six kinds together are the 260 pictures)


def test_one_picture_per_call_quality_100(reference, risk_table):
    # every quantizer 1: one level in any sample of the sharp conversion changes the bytes
    assert _one_per_call(reference, cases.q100_pictures(), ("sharp", "auto")) == 40


def test_one_picture_per_call_wide(reference, risk_table):
    assert _one_per_call(reference, cases.wide_pictures(), ("sharp", "riskiness")) == 3


# ---- b. ragged calls over the list

def _batches(pictures):
    """The list cut into batches of one (q, method)."""
    out = {}
    for p in pictures:
        out.setdefault((p.q, p.method), []).append(p)
    return sorted(out.items())


@pytest.mark.parametrize("yuv_mode", [sj.YUV_SHARP, sj.YUV_AUTO])
def test_ragged_encode_images(engine, reference, risk_table, yuv_mode):
    ref = cases.ref_sharp if yuv_mode == sj.YUV_SHARP else cases.ref_auto
    failures = []
    batches = _batches(cases.pictures() + cases.q100_pictures())
    assert len(batches) == 10
    for (q, m), ps in batches:
        got = sj.encode_images([_dev(p.img) for p in ps], q, yuv_mode, engine=engine, method=m, use_trellis=m >= 7)
        assert len(got) == len(ps)
        failures += [(yuv_mode, cases.what(p)) for p, g in zip(ps, got) if not g == ref(reference, p)]
    _none(failures)


def test_ragged_compress_images(engine, reference, risk_table):
    ps = cases.pictures()
    got = sj.compress_images([_dev(p.img) for p in ps], engine=engine)
    _none([cases.what(p) for p, g in zip(ps, got) if not g == cases.ref_compress(reference, p)])
    got = sj.riskiness_images([_dev(p.img) for p in ps], engine=engine)
    _none([(cases.what(p), g, cases.ref_riskiness(reference, p)) for p, g in zip(ps, got)
           if g != cases.ref_riskiness(reference, p)])


def _quant(q):
    m = np.zeros((2, 64), np.uint8)
    sj.lib().sjpeg_hip_quality_matrices(float(q), m.ctypes.data)
    return m


@pytest.mark.parametrize("yuv_mode", cases.SEARCH_YUV_MODES)
def test_ragged_search_one_call_per_method(engine, reference, risk_table, yuv_mode):
    """Engine.encode_ragged_full: every search case of one method (4, or 7 with the trellis) in ONE call, each picture
    with its own quality, target, passes and tolerance."""
    failures = []
    for trellis in (False, True):
        ss = [s for s in cases.search_cases() if s.trellis == trellis]
        assert len(ss) >= 10
        planes = [[_dev(s.img).reshape(s.h, 3 * s.w)] for s in ss]
        search = [sj.SearchParams(s.target_mode, s.target, s.passes, s.tolerance, 0.0, 100.0) for s in ss]
        out, sizes, offs, modes, _, _ = engine.encode_ragged_full(sj.SRC_RGB, planes, [(s.w, s.h) for s in ss], yuv_mode,
                                                                  [_quant(s.q) for s in ss], 7 if trellis else 4,
                                                                  search=search)
        engine.wait()
        torch.cuda.synchronize()
        host, sz = out.cpu().numpy(), sizes.cpu().numpy()
        for s, o, n in zip(ss, offs, sz):
            if not host[o:o + int(n)].tobytes() == cases.ref_search(reference, s, yuv_mode):
                failures.append((yuv_mode, cases.what(s)))
    _none(failures)


@pytest.mark.parametrize("yuv_mode", cases.SEARCH_YUV_MODES)
def test_ragged_search_encode_images_full(engine, reference, risk_table, yuv_mode):
    """encode_images_full with target_size= / target_psnr=: one call per (target kind, passes, tolerance, trellis)."""
    groups = {}
    for s in cases.search_cases():
        groups.setdefault((s.target_mode, s.passes, s.tolerance, s.trellis), []).append(s)
    failures, n = [], 0
    for (tm, passes, tol, trellis), ss in sorted(groups.items()):
        target = {"target_size" if tm == sj.TARGET_SIZE else "target_psnr": [s.target for s in ss]}
        got = sj.encode_images_full([_dev(s.img) for s in ss], [s.q for s in ss], yuv_mode, 4, trellis, passes=passes,
                                    tolerance=tol, engine=engine, **target)
        failures += [(yuv_mode, cases.what(s)) for s, g in zip(ss, got) if not g == cases.ref_search(reference, s, yuv_mode)]
        n += len(got)
    assert n == 80
    _none(failures)


# ---- c. the other source layouts: the same pictures, the same recorded answers (every integer 0..255 is exact in
# float32, float16 and bfloat16, so with scale 1 and bias 0 the encoder sees the same bytes)

def _alpha(p, order):
    a = np.random.RandomState(p.w * 1000 + p.h).randint(0, 256, (p.h, p.w, 1)).astype(np.uint8)     # (arbitrary, never read)
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([p.img[:, :, order], a], 2))).cuda()


def _chw_images(layout, ps):
    """(images for layout="chw", or FloatPixels of them)"""
    if layout == "rgba":
        return [_alpha(p, [0, 1, 2]).permute(2, 0, 1)[:3] for p in ps]
    planar = [_dev(p.img).permute(2, 0, 1).contiguous() for p in ps]
    last = [_dev(p.img) for p in ps]
    if layout == "planar-u8":
        return planar
    if layout == "planar-f32":
        return sj.FloatPixels([t.float() for t in planar], 1.0, 0.0)
    if layout == "last-f32":
        return sj.FloatPixels([t.float().permute(2, 0, 1) for t in last], 1.0, 0.0)
    if layout == "last-f16":
        return sj.FloatPixels([t.half().permute(2, 0, 1) for t in last], 1.0, 0.0)
    assert layout == "planar-bf16"
    return sj.FloatPixels([t.bfloat16() for t in planar], 1.0, 0.0)


def _layout_pictures():
    ps = cases.q100_pictures()                   # (40 pictures, the twelve fixed sizes among them)
    assert [(p.w, p.h) for p in ps[:12]] == cases.FIXED_SIZES
    return ps


@pytest.mark.parametrize("layout", ["rgba", "planar-u8", "planar-f32", "last-f32", "last-f16", "planar-bf16"])
def test_other_layouts(engine, reference, risk_table, layout):
    ps = _layout_pictures()
    images = _chw_images(layout, ps)
    risk = sj.riskiness_images(images, engine=engine, layout="chw")
    _none([(layout, cases.what(p), g, cases.ref_riskiness(reference, p)) for p, g in zip(ps, risk)
           if g != cases.ref_riskiness(reference, p)])
    got = sj.compress_images(images, engine=engine, layout="chw")
    _none([(layout, cases.what(p)) for p, g in zip(ps, got) if not g == cases.ref_compress(reference, p)])


def test_other_layouts_bgra(engine, reference, risk_table):
    ps = _layout_pictures()
    keep = [_alpha(p, [2, 1, 0]) for p in ps]
    planes = [[t.reshape(p.h, 4 * p.w)] for t, p in zip(keep, ps)]
    dims = [(p.w, p.h) for p in ps]
    sums = engine.riskiness_ragged(sj.SRC_BGRA, planes, dims).cpu().numpy()
    risk = [sj.riskiness_verdict(sums[k], w, h) for k, (w, h) in enumerate(dims)]
    _none([(cases.what(p), g, cases.ref_riskiness(reference, p)) for p, g in zip(ps, risk)
           if g != cases.ref_riskiness(reference, p)])
    # compress_images' call (SJPEG_YUV_AUTO, method 4, quality 75) on the BGRA planes
    out, sizes, offs, modes = engine.encode_ragged_auto(sj.SRC_BGRA, planes, dims, sj.YUV_AUTO, _quant(75.0), 4)
    engine.wait()
    torch.cuda.synchronize()
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    assert modes == [r[0] for r in risk]
    _none([cases.what(p) for p, o, n in zip(ps, offs, sz)
           if not host[o:o + int(n)].tobytes() == cases.ref_compress(reference, p)])


# ---- d. reduced pictures: the box average of a 2 x 2 replicate is the picture itself

def test_reduced_replicates(engine, reference, risk_table):
    ps = cases.even_pictures(10)
    big = [_dev(np.repeat(np.repeat(p.img, 2, 0), 2, 1)) for p in ps]
    got = sj.compress_images(sj.Reduced(big, 2), engine=engine)
    _none([cases.what(p) for p, g in zip(ps, got) if not g == cases.ref_compress(reference, p)])
