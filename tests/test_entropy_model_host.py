"""The plain entropy coder of tests/entropy_model.py pinned on the oracle, then the coverage the directed pictures of
tests/entropy_cases.py must reach -- asserted on the model's trace alone.  CPU only."""
import functools

import numpy as np
import pytest

import entropy_cases as ec
import entropy_model as em
from oracle import synth

# AC symbols that need not occur as the first symbol of a quarter other than 0 (only sizes of 9 and above may be
# listed, where no plan reaches them): none -- every one of the 160 occurs there in both tables
EXEMPT_FIRST_OF_QUARTER = ()


def _random_pictures():
    """40 pictures of the kinds tests/test_gpu_parity.py draws: noise, the structured picture, saturated noise"""
    rs = np.random.RandomState(4711)
    out = []
    for i in range(40):
        w, h = int(rs.randint(1, 201)), int(rs.randint(1, 151))
        kind = i % 3
        img = (synth.g_noise, synth.g_struct, synth.g_noise)[kind](w, h, 1000 + i)
        if kind == 2:
            img = np.where(img > 127, 255, 0).astype(np.uint8)
        out.append((img, (em.YUV_420, em.YUV_444, em.YUV_400)[(i // 3) % 3], (5, 30, 60, 75, 90, 98, 100)[i % 7]))
    return out


def _optimal_codes(oracle, freq, yuv_mode):
    """the codes the oracle's method 1 derives from a picture's own statistics (4:0:0: table 1 stays standard)"""
    dc, ac = oracle.default_codes()
    for t in range(1 if yuv_mode == em.YUV_400 else 2):
        bits, syms, _ = oracle.build_optimal(freq[t, 256:], 12)
        dc[t] = oracle.build_huffman(bits, syms, 12)
        bits, syms, _ = oracle.build_optimal(freq[t, :256], 256)
        ac[t] = oracle.build_huffman(bits, syms, 256)
    return dc, ac


@functools.lru_cache(maxsize=None)
def _trace(oracle, case, family, apply):
    dc, ac = ec.family_codes(oracle, family, apply)
    return em.encode_symbols(case.symbols(oracle), dc, ac)


def test_model_equals_the_oracle_with_default_and_optimal_codes_on_random_pictures(oracle):
    dc, ac = oracle.default_codes()
    for img, mode, q in _random_pictures():
        qm = oracle.quality_matrices(q)
        zz = oracle.scan_coeffs(img, qm, yuv_mode=mode)
        body, tr = em.encode_scan(zz, mode, dc, ac)
        assert body == em.scan_body(oracle.encode(img, q, mode)), (img.shape, mode, q)
        freq = oracle.symbol_stats(img, qm, yuv_mode=mode)
        assert (tr.stats() == freq).all(), (img.shape, mode, q)
        assert tr.block_bits.sum() == tr.segment_bits.sum() and tr.unstuffed_len == (int(tr.block_bits.sum()) + 7) // 8
        assert tr.stuffed_len == len(body) == tr.unstuffed_len + tr.ff_bytes
        assert tr.part_bits.sum() == tr.block_bits.sum()
        odc, oac = _optimal_codes(oracle, freq, mode)
        body, _ = em.encode_scan(zz, mode, odc, oac)
        assert body == em.scan_body(oracle.encode_method(img, q, mode, 1)), (img.shape, mode, q)


@pytest.mark.parametrize("group", ["atlas-gray", "atlas-yb", "dc", "zrl", "bound", "dense"])
def test_model_equals_the_oracle_on_the_directed_pictures(oracle, group):
    cases = {"atlas-gray": lambda: ec.atlas("gray"), "atlas-yb": lambda: ec.atlas("yb"), "dc": ec.dc_pictures,
             "zrl": ec.zrl_pictures, "bound": ec.bound_pictures, "dense": ec.dense_pictures}[group]()
    for c in cases:
        body, tr = _trace(oracle, c, "std", "both")
        assert body == em.scan_body(oracle.encode_matrices(c.rgb, c.quant, yuv_mode=c.yuv_mode)), c.name
        freq = oracle.symbol_stats(c.rgb, c.quant, yuv_mode=c.yuv_mode)
        assert (tr.stats() == freq).all(), c.name
        odc, oac = _optimal_codes(oracle, freq, c.yuv_mode)
        body, _ = em.encode_symbols(c.symbols(oracle), odc, oac)
        assert body == em.scan_body(oracle.encode_full(c.rgb, c.quant, yuv_mode=c.yuv_mode, method=1)), c.name


def test_codes_from_lengths_equals_build_huffman(oracle):
    dc, ac = oracle.default_codes()
    for t in range(2):                                     # the standard tables rebuild from their own lengths
        assert (em.codes_from_lengths(em.lengths_of(ac[t]), 256)[2] == ac[t]).all()
        assert (em.codes_from_lengths(em.lengths_of(dc[t]), 12)[2] == dc[t]).all()
    tables = [(ec.ac_family(f), 256) for f in ec.AC_FAMILIES] + [(ec.DC_LONG, 12), ({s: 16 for s in range(12)}, 12)]
    for lengths, size in tables:
        bits, syms, codes = em.codes_from_lengths(lengths, size)
        assert (codes == oracle.build_huffman(bits, syms, size)).all()
        assert em.lengths_of(codes) == lengths
        b2, s2 = em.description_of(codes)
        assert (b2 == bits).all() and (s2 == syms).all()
        # a valid baseline table: no code is all ones
        assert all((int(c) >> 16) != (1 << (int(c) & 0xFF)) - 1 for c in codes if int(c) & 0xFF)


def test_families_have_the_lengths_they_are_named_for(oracle):
    for n in range(11):
        codes = em.codes_from_lengths(ec.ac_family(f"safe:{n}"), 256)[2]
        assert em.n_safe_of(codes) == n
        assert all((int(codes[k]) & 0xFF) + k == 16 for k in range(1, n + 1))
    for zl in range(1, 17):
        codes = em.codes_from_lengths(ec.ac_family(f"zrl:{zl}"), 256)[2]
        assert int(codes[0xF0]) & 0xFF == zl
        assert zl == 1 or int(codes[0xF0]) >> 16 != 0       # a pattern a wrong shift would move
    for l in (1, 8, 16):
        assert int(em.codes_from_lengths(ec.ac_family(f"eob:{l}"), 256)[2][0]) & 0xFF == l
    dc, ac = ec.family_codes(oracle, "long", "both")
    assert all(int(c) & 0xFF == 16 for c in dc.reshape(-1))
    assert all(int(ac[t][s]) & 0xFF == 16 for t in range(2) for s in ec.AC_SYMBOLS)
    dc, ac = ec.family_codes(oracle, "dc_long", "both")
    assert [int(dc[0][n]) & 0xFF for n in (9, 10, 11)] == [12, 14, 16]
    assert em.n_safe_of(oracle.default_codes()[1][0]) == 7  # the standard tables: levels up to 127 are lean


# ---------------------------------------------------------------------------------------------- coverage conditions

def test_every_ac_symbol_occurs_and_opens_a_quarter(oracle):
    for t, colour in ((0, "gray"), (1, "yb")):
        counts = np.zeros(256, np.int64)
        first, merged = set(), set()
        for c in ec.atlas(colour) + ec.zrl_pictures():
            tr = _trace(oracle, c, "std", "both")[1]
            counts += tr.ac_counts[t]
            first |= {s for s, q in tr.first_of_quarter[t]}
            merged |= tr.first_of_merged[t]
        assert [hex(s) for s in ec.AC_SYMBOLS if counts[s] == 0] == []
        regular = set(ec.AC_SYMBOLS[2:])
        missing = sorted(regular - first - set(EXEMPT_FIRST_OF_QUARTER))
        assert missing == [], [hex(s) for s in missing]
        assert all((s & 15) >= 9 for s in EXEMPT_FIRST_OF_QUARTER)
        assert len(first & regular) >= 150
        assert len(merged & regular) >= 100                 # ... and inside a merged part


def test_every_dc_size_occurs_with_either_sign(oracle):
    signs = np.zeros((2, 12, 2), np.int64)
    for c in ec.dc_pictures():
        tr = _trace(oracle, c, "std", "both")[1]
        signs += tr.dc_signs
        assert len(tr.segment_bits) >= 3                   # the walk crosses segment boundaries
    for t in range(2):
        assert signs[t, 0, 0] > 0
        assert (signs[t, 1:, :] > 0).all(), signs[t].tolist()


@pytest.mark.parametrize("zl", range(1, 17))
def test_zrl_chains_start_at_many_bit_offsets(oracle, zl):
    for t in range(2):
        seen = {1: set(), 2: set(), 3: set()}
        quarters = {1: set(), 2: set(), 3: set()}
        for c in ec.zrl_pictures():
            for (tt, k, z, off, q) in _trace(oracle, c, f"zrl:{zl}", "both")[1].zrl_chains:
                if tt == t:
                    assert z == zl
                    seen[k].add(off)
                    quarters[k].add(q)
        for k in (1, 2, 3):
            assert len(seen[k]) >= 16, (t, zl, k, sorted(seen[k]))
            if k * zl > 32:
                assert 0 in seen[k] and 31 in seen[k], (t, zl, k, sorted(seen[k]))
        assert quarters == {1: {1, 2, 3}, 2: {2, 3}, 3: {3}}


def test_three_zrls_of_the_standard_luma_table_pass_32_bits(oracle):
    """the one case of the standard tables with k * zl > 32: luma, 3 x 11 bits"""
    _, ac = oracle.default_codes()
    assert int(ac[0][0xF0]) & 0xFF == 11
    offs = {off for c in ec.zrl_pictures() for (t, k, z, off, q) in _trace(oracle, c, "std", "both")[1].zrl_chains
            if t == 0 and k == 3}
    assert 0 in offs and 31 in offs and len(offs) >= 16


@pytest.mark.parametrize("n", range(11))
def test_levels_on_both_sides_of_every_bound_share_a_segment(oracle, n):
    for t, c in enumerate(ec.bound_pictures()):
        tr = _trace(oracle, c, f"safe:{n}", "both")[1]
        assert tr.n_safe[t] == n
        seg_blocks = 246
        both = 0
        for s in range(len(tr.segment_bits)):
            mine = [i for i in range(s * seg_blocks, min((s + 1) * seg_blocks, len(tr.block_size))) if tr.block_table[i] == t]
            at = [i for i in mine if tr.block_size[i] == n]
            above = [i for i in mine if tr.block_size[i] == n + 1]
            # the model calls the first lean and the second checked
            assert all(not tr.block_checked[i] for i in at) and all(tr.block_checked[i] for i in above)
            both += bool(at) and (bool(above) or n == 10)  # (no baseline level has 11 bits)
        assert both >= 1, (c.name, n)
        # ... and so every part of such a block
        assert (tr.part_checked == tr.block_checked[tr.part_block]).all()
        assert not (tr.part_merged & tr.part_checked).any()  # a checked block merges nothing
    # the large level alone in quarter 3, small ones elsewhere
    tr = _trace(oracle, ec.bound_pictures()[0], "std", "both")[1]
    zz = ec.bound_pictures()[0].coeffs(oracle)
    assert any(abs(int(b[50])) >= 64 and 0 < np.abs(b[1:50]).max() <= 1 for b in zz)


def test_long_codes_fill_pool_rows_windows_and_slots(oracle):
    rows, long_segments, over_slot = 0, 0, 0
    for c in ec.dense_pictures():
        body, tr = _trace(oracle, c, "long", "both")
        assert tr.n_safe == (0, 0)
        rows += int((tr.part_checked & ((tr.part_bits + 31) // 32 > 8)).sum())
        long_segments += sum(1 for w in tr.segment_words() if w > 2 * em.WINDOW_WORDS)
        # at a capacity of just the stream (no header), a segment's slot is three quarters of its share
        slot = em.slot_words(len(body) + 2, len(tr.segment_bits))
        over_slot += sum(1 for w in tr.segment_words() if w > slot)
        assert tr.block_bits.max() <= em.MAX_BLOCK_BITS
    assert rows >= 1 and long_segments >= 1 and over_slot >= 1


def test_fibonacci_picture_forces_the_optimiser_to_cut_its_codes(oracle):
    qm = oracle.quality_matrices(ec.FIB_QUALITY)
    img = ec.fibonacci_picture(tuple(int(v) for v in qm[0]))
    freq = oracle.symbol_stats(img, qm, yuv_mode=em.YUV_400)
    assert ec.huffman_depth(freq[0, :256]) > 16
    bits, _, _ = oracle.build_optimal(freq[0, :256], 256)
    assert max(k + 1 for k in range(16) if bits[k]) == 16
    dc, ac = _optimal_codes(oracle, freq, em.YUV_400)
    body, _ = em.encode_scan(oracle.scan_coeffs(img, qm, yuv_mode=em.YUV_400), em.YUV_400, dc, ac)
    assert body == em.scan_body(oracle.encode_method(img, ec.FIB_QUALITY, em.YUV_400, 1))
