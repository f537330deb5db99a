"""Directed tests of the entropy phase and the stitch behind it: pictures designed symbol by symbol
(tests/entropy_cases.py) coded with Huffman tables of the CALLER's, family by family, every byte and every count
compared with the plain coder of tests/entropy_model.py -- which tests/test_entropy_model_host.py pins on the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import entropy_cases as ec
import entropy_model as em
import sjpeg_amd as sj

pytestmark = pytest.mark.gpu

FAMILIES = ["std"] + ec.AC_FAMILIES + ["dc_long"]
GUARD = 0xA5


@pytest.fixture(scope="module")
def engine():
    return sj.Engine(0)


class Loaded:
    """a picture on the device, with its symbols walked once"""

    def __init__(self, case, oracle):
        self.case = case
        self.frames = torch.from_numpy(case.rgb).cuda().unsqueeze(0)
        self.planes = [self.frames[0].view(case.h, case.w * 3)]
        self.symbols = case.symbols(oracle)
        self.tables0, self.quant = sj.make_tables(quant=case.quant)


@pytest.fixture(scope="module")
def pictures(oracle):
    return [Loaded(c, oracle) for c in ec.directed_pictures()]


def _tables(pic, dc, ac, flags=0):
    """the picture's quantizer with the caller's code words"""
    t = sj.ScanTables()
    C.memmove(C.byref(t), C.byref(pic.tables0), C.sizeof(t))
    for c in range(2):
        t.dc_codes[c][:] = [int(v) for v in dc[c]]
        t.ac_codes[c][:] = [int(v) for v in ac[c]]
    t.flags = flags
    return t


def _header(pic, dc, ac):
    c = pic.case
    return sj.make_header_ex(c.w, c.h, c.yuv_mode, pic.quant, em.huffman_specs(sj, dc, ac))


def _applies(mode):
    """a gray picture codes with table 0 alone"""
    return ("luma",) if mode == em.YUV_400 else ec.APPLY


def _want(pic, dc, ac):
    body, tr = em.encode_symbols(pic.symbols, dc, ac)
    return _header(pic, dc, ac) + body + b"\xff\xd9", tr


@pytest.mark.parametrize("family", FAMILIES)
def test_uniform_and_ragged_entries_code_every_picture_with_the_callers_tables(engine, oracle, pictures, family):
    for mode in (em.YUV_400, em.YUV_444, em.YUV_420):
        pics = [p for p in pictures if p.case.yuv_mode == mode]
        for apply in _applies(mode):
            dc, ac = ec.family_codes(oracle, family, apply)
            wants = [_want(p, dc, ac)[0] for p in pics]
            tables = [_tables(p, dc, ac) for p in pics]
            headers = [_header(p, dc, ac) for p in pics]
            # the ragged entry, one table set per frame, every frame at sjpeg_hip_frame_bound
            out, sizes, offs = engine.encode_ragged(sj.SRC_RGB, [p.planes for p in pics], [(p.case.w, p.case.h) for p in pics],
                                                    mode, tables, headers)
            sizes, host = sizes.cpu().numpy(), out.cpu().numpy()
            for k, p in enumerate(pics):
                assert sizes[k] != 0, (family, apply, p.case.name)
                assert host[offs[k]:offs[k] + int(sizes[k])].tobytes() == wants[k], (family, apply, p.case.name, "ragged")
            # the uniform entry, picture by picture
            res = [engine.encode_frames(p.frames, tables[k], headers[k], mode) for k, p in enumerate(pics)]
            for k, (p, (o, s)) in enumerate(zip(pics, res)):
                n = int(s[0].item())
                assert n != 0 and bytes(o[0, :n].cpu().numpy()) == wants[k], (family, apply, p.case.name, "uniform")
            if family == "std":
                for k, p in enumerate(pics[::7]):
                    assert wants[7 * k] == oracle.encode_matrices(p.case.rgb, p.case.quant, yuv_mode=mode), p.case.name


@pytest.mark.parametrize("family", FAMILIES)
def test_a_capacity_one_byte_short_gives_size_zero_and_the_exact_capacity_the_bytes(engine, oracle, pictures, family):
    for mode in (em.YUV_400, em.YUV_444, em.YUV_420):
        pics = [p for p in pictures if p.case.yuv_mode == mode]
        dc, ac = ec.family_codes(oracle, family, "both")
        wants = [_want(p, dc, ac)[0] for p in pics]
        tables = [_tables(p, dc, ac) for p in pics]
        headers = [_header(p, dc, ac) for p in pics]
        for short in (1, 0):
            caps = [len(w) - short for w in wants]
            offs, at = [], 64
            for c in caps:
                offs.append(at)
                at += ((c + 15) & ~15) + 64
            out = torch.full((at,), GUARD, dtype=torch.uint8, device="cuda")
            _, sizes, _ = engine.encode_ragged(sj.SRC_RGB, [p.planes for p in pics], [(p.case.w, p.case.h) for p in pics],
                                               mode, tables, headers, capacities=caps, out=out, offsets=offs)
            sizes, host = sizes.cpu().numpy(), out.cpu().numpy()
            inside = np.zeros(at, bool)
            for k, p in enumerate(pics):
                inside[offs[k]:offs[k] + caps[k]] = True
                if short:
                    assert sizes[k] == 0, (family, p.case.name)
                else:
                    assert host[offs[k]:offs[k] + int(sizes[k])].tobytes() == wants[k], (family, p.case.name)
            assert (host[~inside] == GUARD).all(), (family, mode, short)


def test_neighbouring_frames_of_one_launch_differ_in_their_tables(engine, oracle, pictures):
    """encode_source_multi: one table family per frame, so that neighbours differ in n_safe and in the ZRL's length"""
    for name in ("bound-gray", "zrl-gray", "zrl-yb", "bound-yb", "dense-420-2seg"):
        p = next(q for q in pictures if q.case.name == name)
        fams = [f for f in FAMILIES if f != "dc_long"]
        fams = fams[::2] + fams[1::2]                       # safe:0, safe:2 .. beside zrl:2 .. and back
        n = len(fams)
        codes = [ec.family_codes(oracle, f, "both") for f in fams]
        frames = p.frames.expand(n, -1, -1, -1).contiguous()
        src, _keep = sj.make_source(sj.SRC_RGB, [frames.view(n, p.case.h, p.case.w * 3)])
        out, sizes = engine.encode_source_multi(src, n, p.case.w, p.case.h, [_tables(p, dc, ac) for dc, ac in codes],
                                                [_header(p, dc, ac) for dc, ac in codes], p.case.yuv_mode)
        sizes, host = sizes.cpu().numpy(), out.cpu().numpy()
        for k, (dc, ac) in enumerate(codes):
            assert host[k, :int(sizes[k])].tobytes() == _want(p, dc, ac)[0], (name, fams[k])


def test_symbol_statistics_equal_the_models_counts(engine, oracle, pictures):
    for p in pictures:
        if not p.case.name.startswith(("atlas", "dc")):
            continue
        tr = em.encode_symbols(p.symbols, *oracle.default_codes())[1]
        got = engine.scan_symbol_stats(p.frames, p.tables0, p.case.yuv_mode).cpu().numpy().view(np.uint32)[0]
        assert (got.astype(np.int64) == tr.stats()).all(), p.case.name


@pytest.mark.parametrize("family", ["long", "zrl:16", "safe:0"])
def test_counted_bits_equal_the_models(engine, oracle, pictures, family):
    for mode in (em.YUV_400, em.YUV_444, em.YUV_420):
        pics = [p for p in pictures if p.case.yuv_mode == mode]
        dc, ac = ec.family_codes(oracle, family, "both")
        want = [em.encode_symbols(p.symbols, dc, ac)[1].counted_bits for p in pics]
        got = engine.scan_counted_bits_ragged(sj.SRC_RGB, [p.planes for p in pics], [(p.case.w, p.case.h) for p in pics],
                                              mode, [_tables(p, dc, ac) for p in pics]).cpu().numpy()
        assert got.tolist() == want, family


@pytest.mark.parametrize("n", [0, 3, 9])
def test_replay_classifies_blocks_by_the_coding_tables(engine, oracle, pictures, n):
    """a KEEP statistics pass under the standard tables, then REPLAY under safe[n]: lean or checked is a matter of the
    tables the blocks are CODED with"""
    for p in pictures:
        if not p.case.name.startswith("bound"):
            continue
        mode = p.case.yuv_mode
        std = _tables(p, *oracle.default_codes(), flags=sj.QUANT_KEEP)
        engine.scan_symbol_stats(p.frames, std, mode)
        dc, ac = ec.family_codes(oracle, f"safe:{n}", "both")
        want, tr = _want(p, dc, ac)
        assert tr.block_checked.any() and not tr.block_checked.all()
        out, sizes = engine.encode_frames(torch.zeros_like(p.frames), _tables(p, dc, ac, flags=sj.QUANT_REPLAY),
                                          _header(p, dc, ac), mode)
        assert bytes(out[0, :int(sizes[0].item())].cpu().numpy()) == want, (p.case.name, n)


def _trellis_levels(oracle, case, ac_lengths):
    """the picture's blocks through orc_trellis_block, one by one, its rate priced with ac_lengths[2][256]"""
    qz = [oracle.finalize_quant(case.quant[tb]) for tb in range(2)]
    comps = em.MCU_COMPONENTS[case.yuv_mode]
    out = []
    for my in range(case.h // 8):
        for mx in range(case.w // 8):
            coef = oracle.fdct(oracle.get_samples(case.yuv_mode, case.rgb, mx, my)).reshape(-1, 64)
            for k, comp in enumerate(comps):
                tb = 0 if comp == 0 else 1
                out.append(oracle.trellis_block(coef[k], qz[tb], ac_lengths[tb]))
    return np.array(out, np.int16)


# every run of the gray atlas with the symbol in quarter 0, one picture of each other quarter and of the chroma atlas, and
# the bound pictures: 8 070 blocks, each through orc_trellis_block in Python
TRELLIS_PICTURES = ("atlas-gray-q0-", "atlas-gray-q1-run9", "atlas-gray-q2-run15", "atlas-gray-q3-run4", "atlas-yb-q1-run3",
                    "atlas-yb-q0-run12", "bound-")
_std_levels = {}


def _standard_trellis_levels(oracle, case):
    if case.name not in _std_levels:
        _std_levels[case.name] = _trellis_levels(oracle, case, oracle.default_codes()[1])
    return _std_levels[case.name]


@pytest.mark.parametrize("family", ["zrl:16", "eob:16", "long"])
def test_trellis_prices_with_the_callers_lengths(engine, oracle, pictures, family):
    """SJPEG_HIP_QUANT_TRELLIS with trellis_len of a family (the coding tables standard): the levels are those of
    orc_trellis_block block by block, coded by the model.  (The coefficient tap has no trellis kind: the levels are
    seen through the bytes.)"""
    _, fam_ac = ec.family_codes(oracle, family, "both")
    std_dc, std_ac = oracle.default_codes()
    moved = 0
    for p in pictures:
        c = p.case
        if not c.name.startswith(TRELLIS_PICTURES):
            continue
        t = _tables(p, std_dc, std_ac, flags=sj.QUANT_TRELLIS)
        for tb in range(2):
            t.trellis_len[tb][:] = [int(v) & 0xFF for v in fam_ac[tb]]
        header = sj.make_header(c.w, c.h, c.yuv_mode, p.quant)
        out, sizes = engine.encode_frames(p.frames, t, header, c.yuv_mode)
        got = bytes(out[0, :int(sizes[0].item())].cpu().numpy())
        levels = _trellis_levels(oracle, c, fam_ac)
        assert got == header + em.encode_scan(levels, c.yuv_mode, std_dc, std_ac)[0] + b"\xff\xd9", (family, c.name)
        # the family's lengths decide differently from the standard ones somewhere
        moved += int((levels != _standard_trellis_levels(oracle, c)).any(axis=1).sum())
    assert moved > 0, family


def test_fibonacci_counts_through_the_products_own_optimiser(engine, oracle):
    """no caller's table: the optimiser itself has to cut a code of depth 23 to 16 bits"""
    qm = oracle.quality_matrices(ec.FIB_QUALITY)
    img = ec.fibonacci_picture(tuple(int(v) for v in qm[0]))
    for method in (1, 2):
        want = oracle.encode_method(img, ec.FIB_QUALITY, em.YUV_400, method)
        assert sj.SjpegEncode(img, ec.FIB_QUALITY, method, sj.YUV_400) == want, (method, sj.last_error())
    got = sj.encode_images([torch.from_numpy(img).cuda()], ec.FIB_QUALITY, sj.YUV_400, engine=engine, method=1)
    assert got[0] == oracle.encode_method(img, ec.FIB_QUALITY, em.YUV_400, 1)


def test_dc_codes_of_up_to_16_bits_in_front_of_11_bit_differences(engine, oracle, pictures):
    """dc_long: len + n reaches 12 + 9, 14 + 10 and 16 + 11 = 27 bits, the most a baseline table allows"""
    for apply in ec.APPLY:
        dc, ac = ec.family_codes(oracle, "dc_long", apply)
        for p in pictures:
            if not p.case.name.startswith("dc") or (p.case.yuv_mode == em.YUV_400 and apply != "luma"):
                continue
            want, tr = _want(p, dc, ac)
            t = 0 if apply == "luma" else 1
            assert tr.dc_counts[t][11] > 0 or p.case.name == "dc-rc" and t == 0
            out, sizes = engine.encode_frames(p.frames, _tables(p, dc, ac), _header(p, dc, ac), p.case.yuv_mode)
            assert bytes(out[0, :int(sizes[0].item())].cpu().numpy()) == want, (apply, p.case.name)
